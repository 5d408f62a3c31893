// What a context remembers of its previous pano_stitch_multiband, the rules for forgetting it, and
// the choice of the next stitch's route (stitch.hip), as plain C++: no device code, so a host
// program can include it alone (tests/test_stitch_mode_host.py walks every input of the choice).
#pragma once
#include <stdint.h>

#include "../../include/pano360.h"

#define GEOM_BUFS 11              // stitch.hip: geometry_buffers
#define STITCH_SIG 13             // stitch.hip: stitch_signature

struct StitchMemo {
    // what the previous stitch's layout needed: the next one's launch bounds (device layout)
    pano_layout lay;
    int sig[STITCH_SIG];            // the shape of the stitch `lay` belongs to
    bool valid;
    bool verified;                  // lay was read back (device summary) or made on the host
    int used_need;                  // that stitch's warp ran on the need flags
    bool trusted_pending;           // a trusted stitch's summary has not been compared yet
    // kept geometry (PANO_TRUST_GEOMETRY): the previous stitch of this context went through whole
    // with these buffers and no other call has entered the context since
    bool geom_valid;
    const void *geom_bufs[GEOM_BUFS];
    int count[2];                   // stitches that went through on the device layout / fell back
};

// Another call may have written the buffers a stitch left its geometry in, or they were made in
// another stream's order or for other options: a kept-geometry repeat must not read them.
static inline void stitch_memo_void_geometry(StitchMemo &m) { m.geom_valid = false; }
// The previous layout is no bound for the next one (it did not fit, a trusted stitch broke its
// promise, the tile grid changed): the next stitch lays out on the host.
static inline void stitch_memo_void_layout(StitchMemo &m) { m.valid = m.verified = false; }

enum StitchRoute {
    ROUTE_HOST = 0,                 // regions to the host, layout there, one wait
    ROUTE_DEVICE,                   // layout kernel sized by the previous layout with slack; waits, checks
    ROUTE_TRUSTED,                  // layout kernel with the verified layout's own bounds; nobody waits
    ROUTE_KEPT                      // warp, blur and collapse on the geometry the previous stitch left
};

struct StitchFacts {
    int async;                      // PANO_OPT_STITCH_ASYNC: 0, 1, or 2 (tests: bounds the layout exceeds)
    bool interior;                  // interior shortcut with at least one blurred level
    bool grid32;                    // the matrix-core blur's tile grid
    bool memo_valid, sig_equal;     // a stitch of this very shape left its layout behind
    bool prev_records;              // ... with at least one record
    bool arenas_given;              // args->planes, blurred and tile_flags
    int request;                    // args->trust_layout in: PANO_TRUST_NONE / _LAYOUT / _GEOMETRY
    bool verified, pending;         // memo.verified, memo.trusted_pending
    bool geom_was_valid;            // memo.geom_valid when the call entered
    bool list_kept;                 // the work list in the context's buffers is this table's
    bool bufs_equal;                // args' buffers are memo.geom_bufs
};

struct StitchMode {
    int route;                      // StitchRoute
    bool verify_first;              // a pending trusted summary is checked before anything is queued
};

static inline StitchMode stitch_mode(const StitchFacts &f) {
    // The layout on the device: for the default form of the stitch - interior shortcut,
    // matrix-core blur - once a stitch of this shape has gone through and left its needs behind.
    const bool device = f.async != 0 && f.interior && f.grid32 && f.memo_valid && f.sig_equal &&
                        f.prev_records && f.arenas_given;
    const bool want_keep = f.request == PANO_TRUST_GEOMETRY;
    const bool want_trust = f.request == PANO_TRUST_LAYOUT || want_keep;
    // a trusted stitch needs the verified layout of the same shape ...
    const bool trusted = want_trust && device && f.verified && f.async == 1;
    // ... and a kept one the geometry and the work list where the previous stitch left them
    const bool kept = want_keep && trusted && f.geom_was_valid && f.list_kept && f.bufs_equal;
    StitchMode m;
    m.route = kept ? ROUTE_KEPT : trusted ? ROUTE_TRUSTED : device ? ROUTE_DEVICE : ROUTE_HOST;
    m.verify_first = f.pending && !(want_trust && device);
    return m;
}
