// Many frames in one launch (lens.hip, photo.hip, view.hip): the records of a batch - frames,
// camera pairs, views, of mixed sizes - carry a TileSlot; record i's workgroups are those from
// its block0 on, its tiles row by row, so a launch's grid is the sum of its records' tile counts
// and a workgroup finds its record in the prefix of those counts.  A call of more than CHUNK
// records is cut into launches of CHUNK, each with a prefix of its own.
#pragma once
#include "common.h"

struct TileSlot {
    int block0, tiles_x;            // the record's first workgroup in its launch, workgroups per tile row
};

// The record of this workgroup - the last of the launch's n whose block0 <= blockIdx.x - and the
// index of the workgroup's tile inside it.  Workgroup-uniform: the records are read with scalar
// loads.  Rec has a TileSlot member `slot`.
template <class Rec>
__device__ __forceinline__ const Rec &batch_record(const Rec *__restrict__ table, int n, int &tile) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= table[mid].slot.block0)
            lo = mid;
        else
            hi = mid - 1;
    }
    tile = (int)blockIdx.x - table[lo].slot.block0;
    return table[lo];
}

// Record i of a call whose launches take CHUNK records each, w x h items in tiles of TW x TH,
// neither side above MAX_SIDE: fills its slot, adds its tiles to its launch's workgroup count
// (blocks[i / CHUNK], zero before record 0) and returns their number.
template <int MAX_SIDE, int TW, int TH, int CHUNK>
static inline int batch_assign(TileSlot &slot, int *blocks, int i, int w, int h) {
    static_assert((int64_t)CHUNK * ((MAX_SIDE + TW - 1) / TW) * ((MAX_SIDE + TH - 1) / TH) <= 0x7fffffff,
                  "block0 and a launch's grid are ints");
    slot.tiles_x = ceil_div(w, TW);
    const int tiles = slot.tiles_x * ceil_div(h, TH);
    slot.block0 = blocks[i / CHUNK];
    blocks[i / CHUNK] += tiles;
    return tiles;
}

// A call of several kernels over the same frames (align.hip, deghost.hip) uploads ONE table with a
// section of records per launch: the records of a launch, its workgroups, and where its records
// start in the uploaded table.
template <class Rec>
struct BatchSection {
    std::vector<Rec> recs;
    int blocks = 0;
    int first = 0;
};

// Appends D, w x h items in tiles of TW x TH, to a section of at most CHUNK records.
template <int MAX_SIDE, int TW, int TH, int CHUNK, class Rec>
static inline void batch_section_add(BatchSection<Rec> &S, Rec D, int w, int h) {
    batch_assign<MAX_SIDE, TW, TH, CHUNK>(D.slot, &S.blocks, (int)S.recs.size(), w, h);
    S.recs.push_back(D);
}

// Queues `kernel` for section S of the table at `dev` on stream `s`; an empty section is no launch.
#define BATCH_LAUNCH_SECTION(kernel, S, threads, dev, s)                                                   \
    do {                                                                                                   \
        if (!(S).recs.empty()) {                                                                           \
            hipLaunchKernelGGL(kernel, dim3((unsigned)(S).blocks), dim3(threads), 0, s, (dev) + (S).first, \
                               (int)(S).recs.size());                                                      \
            PANO_LAUNCH_CHECK(#kernel);                                                                    \
        }                                                                                                  \
    } while (0)

// The call: the whole table goes up to the context's buffer `id` at once, then launch(records,
// count, grid) queues kernel `name` for every `chunk` records of it: a launch's first record on
// the device, how many it takes and its workgroups.
template <class Rec, class Launch>
static inline int batch_run(pano_ctx *ctx, int id, const std::vector<Rec> &table, int chunk, const int *blocks,
                            hipStream_t s, const char *name, Launch launch) {
    if (int rc = pano_buf_upload(ctx, id, table.data(), table.size() * sizeof(Rec), s)) return rc;
    const int n = (int)table.size();
    for (int first = 0; first < n; first += chunk) {
        launch((const Rec *)ctx->buf[id].p + first, n - first < chunk ? n - first : chunk, blocks[first / chunk]);
        PANO_LAUNCH_CHECK(name);
    }
    return PANO_OK;
}
