// Shared host/device helpers for libpano360_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/pano360.h"
#include "stitch_mode.h"

// ---- error plumbing --------------------------------------------------------
void pano_set_error(const char *fmt, ...);

#define PANO_REQUIRE(cond, ...)          \
    do {                                 \
        if (!(cond)) {                   \
            pano_set_error(__VA_ARGS__); \
            return PANO_EINVAL;          \
        }                                \
    } while (0)

#define PANO_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            pano_set_error("%s failed: %s", #call, hipGetErrorString(e_));     \
            return PANO_EHIP;                                                  \
        }                                                                      \
    } while (0)

#define PANO_LAUNCH_CHECK(name)                                                \
    do {                                                                       \
        hipError_t e_ = hipGetLastError();                                     \
        if (e_ != hipSuccess) {                                                \
            pano_set_error("launch of %s failed: %s", name,                    \
                           hipGetErrorString(e_));                             \
            return PANO_EHIP;                                                  \
        }                                                                      \
    } while (0)

// ---- per-kernel timing (HIP events on the launch stream; off by default) ----
enum PanoKernelId {
    PK_ADD_WEIGHTS = 0,
    PK_WARP,
    PK_OWNERSHIP,
    PK_BLUR_ROWS,
    PK_BLUR_COLS,
    PK_COMPOSE,
    PK_LINEAR,
    PK_NOBLEND,
    PK_CROP_HEIGHTS,
    PK_CROP_ROWS,
    PK_PYR_DOWN,
    PK_OWNERSHIP_CAMS,
    PK_OWNED_BOXES,
    PK_WARP_WINDOWS,
    PK_BLEND_CAMERAS,
    PK_OWNED_SPANS,
    PK_INTERIOR,
    PK_TILE_FLAGS,
    PK_OVERLAP,
    PK_BLUR_MFMA,
    PK_SIFT_EXTREMA,
    PK_SIFT_ORIENT,
    PK_SIFT_DESCRIBE,
    PK_SCALE_STEP,
    PK_KNN2,
    PK_BLUR_LEAN,
    PK_BLUR_LEAN5,
    PK_RANSAC_SCORE,
    PK_RANSAC_FINISH,
    PK_MATCH_PACK,
    PK_BA_RESIDUAL,
    PK_BA_PAIRS,
    PK_BA_ASSEMBLE,
    PK_JPEG_DESTUFF,
    PK_JPEG_SCAN,
    PK_JPEG_INTERVALS,
    PK_JPEG_HUFF_SYNC,
    PK_JPEG_HUFF_WRITE,
    PK_JPEG_DC,
    PK_JPEG_IDCT,
    PK_JPEG_PIXELS,
    PK_JPEG_ENC_BLOCKS,
    PK_JPEG_ENC_COUNT,
    PK_JPEG_ENC_SCAN,
    PK_JPEG_ENC_EMIT,
    PK_JPEG_ENC_STUFF,
    PK_PNG_FILTER,
    PK_DEFLATE_CODE,
    PK_DEFLATE_SCAN,
    PK_DEFLATE_EMIT,
    PK_DEFLATE_LENGTHS,
    PK_PHOTO_STATS,
    PK_BA_REFINE,
    PK_ALIGN_GREY,
    PK_ALIGN_BITMAP,
    PK_ALIGN_SEARCH,
    PK_ALIGN_APPLY,
    PK_DEGHOST_HIST,
    PK_DEGHOST_RAW,
    PK_DEGHOST_CLEAN,
    PK_DEGHOST_APPLY,
    PK_COUNT
};
// ---- the context (include/pano360.h: pano_ctx) ------------------------------------
// Everything the library remembers between calls lives here: device and stream, the
// option switches, the timing registry, the blur's work-list buffers and the operand
// tables of the tap sets it has seen.  One context per host thread; nothing is shared
// between contexts.
struct PanoTapSet {                 // one set of Gaussian apertures (pano_multiband_blur)
    uint64_t key;                   // hash of the apertures and the tap values
    int n, ntaps[PANO_MAX_LEVELS];
    float *taps;                    // dev: the caller's padded tables, back to back
    unsigned char *tables;          // dev: matrix-core operand tables (built on first use)
    uint64_t used;                  // last use (eviction order)
    float *host;                    // the values themselves: a hash hit is confirmed by comparing them
    size_t floats;
    hipEvent_t ready;               // recorded behind the upload and the table build
    hipStream_t built_on;           // the stream those were queued on
};

struct PanoSiftGraph {               // detect.hip: one captured launch sequence of pano_sift_detect
    uint64_t key;                   // hash of sizes, switches, buffer addresses, tap values
    hipGraphExec_t exec;            // null: not captured (yet, or the capture failed)
    int seen;                       // 0 new, 1 ran launch by launch once, 2 capture attempted
    uint64_t used;                  // last use (eviction order)
};

// A buffer the context owns (device memory, or pinned host memory), grown on demand and never
// shrunk.  A stage that needs one adds an id here and calls pano_buf_reserve; pano_ctx_destroy
// frees them all.
struct PanoBuf {
    void *p;
    size_t cap;                     // bytes
    bool pinned;                    // hipHostMalloc rather than hipMalloc
};
enum PanoBufId {
    // matrix-core blur: the work list (unsorted, sorted) and its counter
    BUF_ITEM_LIST = 0,
    BUF_ITEM_COUNTER,
    // pano_stitch_multiband without its host round trip (stitch.hip): the device-side layout's
    // summary (pinned: the layout kernel writes it, the host reads it), device copies of the patch
    // rectangles and resident flags
    BUF_LAY_SUM_HOST,
    BUF_LAY_RECTS,
    BUF_LAY_HAVE,
    // pano_sift_extrema: the list of scale-space extrema between its two kernels (+ its counter)
    BUF_SIFT_RAW,
    // pano_jpeg_encode (jpeg_enc.hip): the raw stream and its stuffing scan, the stuffed stream,
    // and its pinned host copy (what the call returns)
    BUF_ENC_DEV,
    BUF_ENC_OUT,
    BUF_ENC_HOST,
    // pano_poisson_blend (poisson.hip): the solver's vectors, partial sums and per-channel
    // scalars, and the pinned host copy of those scalars (the convergence readback)
    BUF_POISSON_DEV,
    BUF_POISSON_HOST,
    // pano_seam_flood (graphcut.hip), tiled path: the class being flooded and its "changed" word
    // (device), and the pinned host word the batches' "done" is read into
    BUF_SEAM_DEV,
    BUF_SEAM_HOST,
    // pano_deflate (png_enc.hip): the zeroed stream the emission ORs into, and its pinned host
    // copy (what the call returns)
    BUF_PNG_DEV,
    BUF_PNG_HOST,
    // pano_fill_u8 (fill.hip): the "any pixel valid" word and the float32 levels >= 1 (fill_layout.h)
    BUF_FILL_DEV,
    // pano_lens_undistort_u8 (lens.hip): the batch's frame records
    BUF_LENS_DEV,
    // pano_photo_stats / pano_photo_apply_u8 (photo.hip): the batch's records, and the statistics'
    // per-workgroup partial sums
    BUF_PHOTO_DEV,
    BUF_PHOTO_PARTIALS,
    // pano_align_mtb (align.hip): the records of a pass's launches
    BUF_ALIGN_DEV,
    // pano_deghost_u8 (deghost.hip): the records of a pass's launches
    BUF_DEGHOST_DEV,
    // pano_seam_route_flood (seam_route.hip): the class being flooded, its "changed" word and the
    // group table (device), and the pinned host words "done" is read into; pano_seam_route: the
    // planes between its stages (device) and the pinned host copy of the pair matrix
    BUF_ROUTE_STATE,
    BUF_ROUTE_HOST,
    BUF_ROUTE_PLANES,
    BUF_ROUTE_PAIRS_HOST,
    // pano_flow_* (flow.hip): the records of a call's launches
    BUF_FLOW_DEV,
    PANO_BUF_COUNT
};
// Makes `b` hold at least `need` bytes.  A buffer that is large enough is left alone; otherwise it
// is freed and `need + slack` bytes are allocated, and a failure leaves {nullptr, 0} behind.  The
// old contents are lost, and NOTHING here waits for queued work that still uses them: a caller
// whose stream may not be idle synchronises first, and only when `need > b.cap`.
int pano_buf_reserve(PanoBuf &b, size_t need, bool pinned, size_t slack = 0);
// pano_buf_reserve of the context's device buffer `id` when kernels queued on `stream` may still
// use the old one: waits for the stream first, and only when the buffer exists and must grow.
int pano_buf_reserve_sync(pano_ctx *ctx, int id, size_t need, hipStream_t stream);
// ... and then queues the copy of `bytes` bytes of pageable host memory into it.
int pano_buf_upload(pano_ctx *ctx, int id, const void *host, size_t bytes, hipStream_t stream);

struct pano_ctx {
    int device;
    hipStream_t stream;
    int opt[PANO_OPT_COUNT];
    bool timing_on;
    std::vector<hipEvent_t> t_begin[PK_COUNT], t_end[PK_COUNT];
    PanoBuf buf[PANO_BUF_COUNT];    // (by PanoBufId)
    // matrix-core blur: whose list / tile flags the work-list buffers currently hold
    int blur_cm;                    // reach (k-steps) of the blur levels the next work list is for; 0 = unknown
    const pano_patch *prepared_table, *flags_table;
    int prepared_n, flags_n;
    // whose work list BUF_ITEM_LIST holds (stays when a blur has consumed `prepared_table`; an option
    // switch or a re-allocation clears it): what a kept-geometry repeat may re-use
    const pano_patch *list_table;
    int list_n;
    std::vector<PanoTapSet> tap_sets;
    uint64_t tick;
    // pano_stitch_multiband: the regions' copy has landed / the record table has left the
    // caller's pinned buffer
    hipEvent_t ev_regions, ev_upload, ev_fork, ev_join, ev_copy;
    hipStream_t side;               // second stream of pano_stitch_multiband
    bool upload_pending;
    // pano_stitch_multiband without its host round trip (stitch.hip): the host values the device
    // copies of the patch rectangles and resident flags were made from
    std::vector<int32_t> lay_rects_host;
    std::vector<uint8_t> lay_have_host;
    StitchMemo memo;                // what the previous stitch left for the next (stitch_mode.h)
    bool in_stitch;                 // the stitch's own nested calls do not void the kept geometry
    bool sift_capturing;            // pano_sift_detect is capturing a launch sequence (detect.hip)
    // pano_sift_detect: the captured launch sequences, one per set of buffers (detect.hip)
    std::vector<PanoSiftGraph> sift_graphs;
};

int pano_ctx_enter(pano_ctx *ctx);
void pano_sift_graphs_free(pano_ctx *ctx);   // detect.hip
int pano_sift_raw_reserve(pano_ctx *ctx, int rows, int cols);   // sift.hip: the extrema list's size
int pano_zero_i32(hipStream_t s, int *p, int n);   // detect.hip: p[0 .. n) = 0, as a kernel
int pano_ctx_side_stream(pano_ctx *ctx);     // makes ctx->side and the fork / join events
// Device copy of a host tap table set (and, with `tables`, its matrix-core operand tables'
// buffer, `table_bytes` long, `*fresh` = it was just allocated and must be filled).
int pano_ctx_tap_set(pano_ctx *ctx, const float *taps, const int *ntaps, int n, size_t table_bytes,
                     PanoTapSet **out, bool *fresh);
// After the caller has queued the fill of a `fresh` table buffer on ctx->stream: uses from other
// streams wait for it.
int pano_ctx_tap_set_built(pano_ctx *ctx, PanoTapSet *set);

#define PANO_ENTER(ctx, who)                                       \
    PANO_REQUIRE((ctx) != nullptr, "%s: null context", who);       \
    if (int rc_ = pano_ctx_enter(ctx)) return rc_;                 \
    void *const stream = (void *)(ctx)->stream;                    \
    (void)stream

// An entry point that only READS what a stitch left behind (the crop reads the valid mask): the
// kept geometry (stitch.hip) survives it.
#define PANO_ENTER_READONLY(ctx, who)                              \
    const bool geom_keep_ = (ctx) != nullptr && (ctx)->memo.geom_valid; \
    PANO_ENTER(ctx, who);                                          \
    (ctx)->memo.geom_valid = geom_keep_

void pano_timing_edge(pano_ctx *ctx, int kid, hipStream_t stream, bool begin);

// Launch `...` on `stream`; when timing is enabled bracket it with events.
#define PANO_TIMED(kid, stream, ...)                                        \
    do {                                                                    \
        if (ctx->timing_on) pano_timing_edge(ctx, kid, stream, true);       \
        __VA_ARGS__;                                                        \
        if (ctx->timing_on) pano_timing_edge(ctx, kid, stream, false);      \
    } while (0)

static inline int pano_pitch_of(int w) { return (w + 3) & ~3; }

// blur_mfma.hip: all multiband levels of all records on the matrix cores
int pano_launch_blur_mfma(pano_ctx *ctx, const pano_patch *table, int n, int max_aw, int max_ah,
                          const int16_t *owner, int W, const float *taps, const int *ntaps,
                          int n_blur, const uint8_t *interior, uint8_t *tile_flags);
int pano_prepare_blur_mfma(pano_ctx *ctx, const pano_patch *table, int n, int max_aw, int max_ah,
                           int W, const uint8_t *interior, uint8_t *tile_flags);
int pano_tiles_blur_mfma(pano_ctx *ctx, const pano_patch *table, int n, int max_aw, int max_ah,
                         int W, int radius, const uint8_t *interior, uint8_t *tile_flags,
                         uint8_t *warp_need);
int pano_blur_mfma_opt_in(void);
int pano_blur_valu_opt_in(void);
int pano_deflate_opt_in(void);                     // png_enc.hip
static inline bool pano_blur_uses_mfma(const pano_ctx *ctx) {
    return ctx->opt[PANO_OPT_BLUR_KERNEL] == PANO_BLUR_MFMA;
}

// ---- integer helpers ---------------------------------------------------------
// (in the wider of the two types: int for ints, int64_t as soon as one operand is)
template <class A, class B>
static inline auto ceil_div(A a, B b) -> decltype(a + b) { return (a + b - 1) / b; }
// the next multiple of 256 bytes: where a part of a work buffer starts
template <class T>
static inline T align_up(T bytes) { return (bytes + 255) / 256 * 256; }
// whether the byte ranges [a, a + na) and [b, b + nb) meet
static inline bool pano_overlap(const void *a, size_t na, const void *b, size_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
// an exposure stack (fuse.hip, align.hip, deghost.hip): k frames of h x w within the limits of the header
static inline bool pano_stack_ok(int h, int w, int k) {
    return h >= 1 && w >= 1 && h <= PANO_FUSE_MAX_SIDE && w <= PANO_FUSE_MAX_SIDE && k >= 2 &&
           k <= PANO_FUSE_MAX_EXPOSURES;
}
// Stack i of entry point `who` (align.hip, deghost.hip): k exposures src within the limits above,
// `reference` one of them, none null, pitches of 3 w or more, and every dst that is given misses
// the source frames of its stack and the workspace.
static inline int pano_stack_frames_check(const char *who, int i, const uint8_t *const *src, const int64_t *src_pitch,
                                          uint8_t *const *dst, const int64_t *dst_pitch, int w, int h, int k,
                                          int reference, const void *work, size_t work_bytes) {
    PANO_REQUIRE(pano_stack_ok(h, w, k), "%s: stack %d: %d exposures of %d x %d (2 .. %d, sides 1 .. %d)", who, i, k, w,
                 h, PANO_FUSE_MAX_EXPOSURES, PANO_FUSE_MAX_SIDE);
    PANO_REQUIRE(reference >= 0 && reference < k, "%s: stack %d: reference %d of %d exposures", who, i, reference, k);
    for (int e = 0; e < k; ++e) {
        PANO_REQUIRE(src[e], "%s: stack %d: exposure %d: null pointer", who, i, e);
        PANO_REQUIRE(src_pitch[e] >= 3 * (int64_t)w, "%s: stack %d: exposure %d: pitch %lld for %d pixels", who, i, e,
                     (long long)src_pitch[e], w);
    }
    for (int e = 0; e < k; ++e) {
        if (!dst[e]) continue;
        PANO_REQUIRE(dst_pitch[e] >= 3 * (int64_t)w, "%s: stack %d: dst %d: pitch %lld for %d pixels", who, i, e,
                     (long long)dst_pitch[e], w);
        const size_t dst_bytes = (size_t)(h - 1) * dst_pitch[e] + 3 * (size_t)w;
        PANO_REQUIRE(!pano_overlap(dst[e], dst_bytes, work, work_bytes), "%s: stack %d: dst %d overlaps the workspace",
                     who, i, e);
        for (int f = 0; f < k; ++f)
            PANO_REQUIRE(!pano_overlap(dst[e], dst_bytes, src[f], (size_t)(h - 1) * src_pitch[f] + 3 * (size_t)w),
                         "%s: stack %d: dst %d overlaps exposure %d", who, i, e, f);
    }
    return PANO_OK;
}
// the grid of a kernel that loops beyond `cap` workgroups
static inline dim3 capped_grid(int64_t groups, int64_t cap) {
    return dim3((unsigned)(groups < cap ? groups : cap));
}

// ---- device helpers --------------------------------------------------------
// Scalar-cache view of read-only global memory: loads through this pointer are
// selected as s_load (SGPR operands for the FMA chains of the blur kernels).
typedef const __attribute__((address_space(4))) float *kptr_f32;

// cv2.BORDER_REFLECT      ... c b a | a b c ... z | z y x ...
__device__ __forceinline__ int reflect_edge(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    int per = 2 * len;
    int m = p % per;
    if (m < 0) m += per;
    return m < len ? m : per - 1 - m;
}

// cv2.BORDER_REFLECT_101  ... c b | a b c ... z | y x ...   (len 1 -> 0)
__device__ __forceinline__ int reflect_101(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    int per = 2 * len - 2;
    int m = p % per;
    if (m < 0) m += per;
    return m < len ? m : per - m;
}

// cvRound(float) the way x86 cvtss2si does it: ties to even, and the
// "integer indefinite" 0x80000000 for NaN or anything outside int32.
__device__ __forceinline__ int cv_round(float v) {
    const float r = rintf(v);
    // (one compare: |r| < 2^31 fails for NaN, for everything outside int32 and for -2^31 itself,
    // whose conversion is that same bit pattern)
    return fabsf(r) < 2147483648.0f ? (int)r : (int)0x80000000;
}

__device__ __forceinline__ int sat16(int v) {
    return v < -32768 ? -32768 : (v > 32767 ? 32767 : v);
}
