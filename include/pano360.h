/*
 * pano360.h - C ABI of libpano360_hip.so (MI355X / gfx950).
 *
 * The reference (Banus/pano360) is pure Python and has no FFI; its boundary
 * for the warp/blend hot path is the Python function surface of stitcher.py.
 * Each entry point below names the reference function (file:line, relative to
 * the reference repo) whose arithmetic it replaces.  pano360_amd/stitcher.py
 * keeps those Python signatures and calls these symbols through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every kernel-launching entry point takes a context (pano_ctx, below) first:
 *     it names the device and the stream the work is enqueued on, carries the
 *     option switches and owns everything the library remembers between calls
 *     (work-list buffers of the blur, device copies and operand tables of the
 *     tap sets it has seen, the timing registry).  There is no process-wide
 *     state: two contexts - two streams, two devices, two host threads - do not
 *     see each other.  A context is not thread-safe: one per host thread;
 *   - every pointer marked "dev" is a device (HBM) pointer owned by the
 *     caller; "host" pointers are ordinary host memory read before return;
 *   - all work is enqueued asynchronously on the context's stream, nothing
 *     synchronises;
 *   - return value: 0 on success, a negative PANO_E* code otherwise, with a
 *     thread-local message available from pano_last_error();
 *   - no exceptions cross the boundary.
 *
 * Layouts
 *   frame      uint8  [H][W][3]      as cv2.imread hands it to the reference
 *   planes     float  [c][vh][vpitch] planar R,G,B(,A) of a warped patch
 *                                    window, pitch = pano_pitch(width) floats
 *   mask       uint8  [h][w]         1 = outside the source frame
 *   owner      int16  [H][W]         patch index owning the pixel, -1 = none
 *   mosaic     uint8  [H][W][3]
 *
 * Windows.  Multiband blending only ever uses a patch near the pixels it owns:
 * beyond the Gaussian radius of the last owned pixel every blurred alpha is an
 * exact 0 and the patch contributes 0 to every sum (stitcher.py:231-232).  A
 * patch therefore carries two sub-rectangles, in patch-local coordinates:
 *   A = bounding box of its owned pixels grown by the largest radius R
 *       (clipped to the patch): where blurred copies exist and are gathered;
 *   V = A grown by R again (closed under the REFLECT_101 border rule, its
 *       columns rounded outwards to multiples of 4 and clipped to the patch):
 *       where the warped colour is needed as blur input.
 * Both default to the whole patch (the stage-level blender API).
 */
#ifndef PANO360_H
#define PANO360_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PANO_OK 0
#define PANO_EINVAL (-1)   /* bad argument (shape, null pointer, limits)   */
#define PANO_EHIP (-2)     /* a HIP runtime call failed                    */
#define PANO_ELIMIT (-3)   /* size beyond a compiled-in limit              */
#define PANO_ESOLVE (-4)   /* an iterative solve hit its cap or broke down */

#define PANO_MAX_TAPS 129      /* largest Gaussian aperture (sigma <= 16)  */
#define PANO_MAX_LEVELS 8      /* n_levels of multiband_blend              */
#define PANO_TAP_LEAD 7        /* zero taps in front of a padded tap table */
#define PANO_TAP_PAD 40        /* padded table length = ntaps + this       */
#ifndef PANO_INTERIOR_BLOCK
#define PANO_INTERIOR_BLOCK 4  /* side of the blocks of pano_interior_map  */
#endif
#ifndef PANO_MEDIAN_KEEP
#define PANO_MEDIAN_KEEP 32    /* samples of a pixel the median blend votes on in one pass */
#endif

/* One warped patch as the blenders see it (reference: the tuples appended at
 * stitcher.py:318-319).  All pointers dev. */
typedef struct pano_patch {
    float *planes;             /* [3 or 4][vh][vpitch] over window V        */
    uint8_t *mask;             /* [h][w], full patch; NULL in the fused path */
    float *blurred;            /* [n_levels-1][4][ah][apitch] over A; or NULL */
    float *scratch;            /* [n_levels-1][4][vh][apitch] row-pass output */
    int32_t y0, x0, h, w;      /* patch rectangle in mosaic coordinates     */
    int32_t vy0, vx0, vh, vw;  /* window V, patch-local                     */
    int32_t ay0, ax0, ah, aw;  /* rectangle A, patch-local                  */
    int32_t vpitch, apitch;    /* floats per row of planes / blurred        */
    int32_t index;             /* camera / owner-map index this record belongs
                                  to: a patch whose owned pixels fall into
                                  several far-apart column spans (a frame that
                                  straddles the +-pi seam of a 360 degree sweep)
                                  is split into one record per span           */
    int32_t tiles_off;         /* first entry of this record's 64 x 128 column
                                  tiles in the tile_flags array (row-major,
                                  ceil(aw/64) per row)                        */
} pano_patch;

/* What pano_layout_windows reports besides the records. */
typedef struct pano_layout {
    int64_t planes_floats;     /* arena sizes the records' pointers will index     */
    int64_t blurred_floats;
    int64_t scratch_floats;
    int32_t n_records, n_tiles;
    int32_t max_vw, max_vh, max_aw, max_ah;
    int32_t missing;           /* records of cameras flagged absent in `have`      */
} pano_layout;

/* One registered frame (reference: bundle_adj.Image, bundle_adj.py:18-33,
 * plus the patch rectangle stitch() derives for it). */
typedef struct pano_camera {
    double proj[9];            /* K R, row-major (bundle_adj.py:31-33)      */
    const uint8_t *frame;      /* dev uint8 [sh][sw][3]; may be NULL for the
                                  ownership kernel, which reads no pixels   */
    const double *hat_x;       /* dev double[sw] = _hat(sw) (stitcher.py:251) */
    const double *hat_y;       /* dev double[sh]                            */
    int32_t sh, sw;            /* frame size                                */
    int32_t y0, x0, h, w;      /* patch rectangle in mosaic coordinates     */
} pano_camera;

/* One (i, j) iteration of equalize_gains (stitcher.py:44-63). */
typedef struct pano_pair {
    double minv[9];            /* cv::invert of the pixel homography j -> i
                                  (stitcher.py:48), row-major                */
    int32_t i, j;              /* camera indices, frame i is the destination */
} pano_pair;

/* One SIFT keypoint (reference: the cv2.KeyPoint objects of features.py:197). */
typedef struct pano_sift_keypoint {
    float x, y;                /* position                                   */
    float size;                /* diameter of the meaningful neighbourhood    */
    float angle;               /* degrees, [0, 360)                           */
    float response;            /* |contrast| of the refined extremum          */
    int32_t octave;            /* octave | layer << 8 | round((xi+0.5)*255) << 16 */
    int32_t r, c;              /* refined sample in the octave's own grid     */
} pano_sift_keypoint;

/* Colour tables.  The reference turns a frame into float32(u8)/255
 * (stitcher.py:259) and, with equalize=True, into clip(gain * that, 0, 1)
 * (stitcher.py:66): either way a function of the uint8 value alone, so the
 * kernels sample uint8 frames through a 256-entry float table built on the
 * host with NumPy.  Entry points that sample several cameras take
 * (lut, lut_stride): camera k uses lut + k * lut_stride; stride 0 = one table
 * for all (no equalisation), stride 256 = one table per camera. */

const char *pano_version(void);
const char *pano_last_error(void);
int pano_device_count(void);
/* Row pitch (in floats) used for every float plane of width w. */
int pano_pitch(int w);
/* PANO_INTERIOR_BLOCK as this build of the library was compiled with it. */
int pano_interior_block(void);

/* The context (no reference counterpart: the reference is one Python process
 * with OpenCV's global state).  pano_ctx_create binds a device and a stream
 * (a hipStream_t passed as void*, NULL = the default stream); the caller keeps
 * the stream alive for as long as the context uses it.  pano_ctx_set_stream
 * re-targets later calls (work already queued stays where it is; state built
 * on the old stream - tile flags, work lists, tap tables - is ordered by the
 * caller with events, as for any two streams).  pano_ctx_destroy waits for the
 * context's stream and frees what the context owns.
 * Options (pano_ctx_set_option / pano_ctx_get_option):
 *   PANO_OPT_BLUR_KERNEL  which kernels run the multiband Gaussian levels:
 *                         PANO_BLUR_MFMA (default) = the fused matrix-core kernel
 *                         (split float16 operands, float32 accumulate),
 *                         PANO_BLUR_VALU = separate row / column passes in float32
 *                         on the vector ALU (one FMA per tap)
 *   PANO_OPT_OWN_PRUNE    bit 0: 1 (default) = pano_ownership_cameras skips cameras that
 *                         rigorous bounds exclude (per 64 x 16 sub-tile, the survivors again
 *                         per 16 x 16 quarter); 0 = evaluate every camera at every pixel.
 *                         bit 1: 2 = the one-level kernel of round 4 (bounds per 64 x 16
 *                         sub-tile only; A/B and cross-check).  Same maps, bit for bit.
 *   PANO_OPT_BLUR_SEGMENTS  matrix-core blur: 1 (default) = when a launch has too few column
 *                         strips to fill the CUs (one GPU's share of a panorama, small
 *                         scenes) each strip is cut into vertical segments; 0 = never
 *   PANO_OPT_BLUR_LEAN    matrix-core blur: 1 (default) = a kernel with a short, hand-ordered
 *                         instruction stream takes every work item (those whose bands hold
 *                         reflected columns, unaligned windows or low patches load them
 *                         element by element); 0 = the general kernel for everything.
 *                         Same results bit for bit.  With it on, the five
 *                         Gaussian levels of a six-level pyramid (n_levels = 6) run in ONE
 *                         launch (the two lightest levels on one wave pair); off, they split
 *                         into launches of 2 + 2 + 1 levels that each stage the bands.
 *   PANO_OPT_STITCH_STREAMS  pano_stitch_multiband: 1 (default) = the interior map runs beside
 *                         the region search, and the blur's tile flags and work list beside
 *                         the warp, on a second stream the context owns (ordered by events);
 *                         0 = everything on the context's stream.  Same results.
 *   PANO_OPT_STITCH_ASYNC  pano_stitch_multiband: 1 = when the previous stitch of the same
 *                         shape went through, the record table is laid out by a kernel and
 *                         the warp, blur and collapse are queued behind it at once, sized by
 *                         what the previous layout needed (plus slack); the host then waits
 *                         for the layout's summary while the GPU works, and only if this
 *                         layout needed more (or an arena is too small) the stitch is laid
 *                         out again on the host and its tail queued a second time.
 *                         0 (default) = always the host layout: measured, the round trip it
 *                         saves is already covered by the side stream's kernels (DESIGN.md
 *                         section 4.14), so the simpler path is the default.  Same results.
 *                         (2 = as 1 with launch bounds the layout is sure to exceed: the
 *                         tests' way into the fallback.)
 *   PANO_OPT_BLUR_SEG_LEN matrix-core blur, with PANO_OPT_BLUR_SEGMENTS on: 0 (default) = the
 *                         length of the vertical segments a launch with few work items is cut
 *                         into comes from the sort kernel's list-schedule estimate; n >= 4 =
 *                         segments of n bands (32 rows each); -1 = nothing is cut.  Same results
 *                         bit for bit (A/B of the estimate, and the tests' way to other cuts).
 *   PANO_OPT_SIFT_GRAPH   pano_sift_detect: 1 (default) = a frame's launch sequence is captured
 *                         into a HIP graph the second time a set of buffers is used and replayed
 *                         from then on (one hipGraphLaunch per frame instead of ~110 launches);
 *                         0 = always launch by launch.  Same results bit for bit.
 *   PANO_OPT_LEVEL_CLASSES  pano_multiband_compose / pano_stitch_multiband: 1 = the collapse
 *                         uses the level classes (pano_interior_classes; the stitch computes
 *                         them); 0 (default) = it gathers every copy on every pixel that is not
 *                         interior.  The mosaics agree to float32 rounding.  Measured (round 6,
 *                         profiles/r06/ab_level_classes.txt): the classes take 13 % off the
 *                         collapse's HBM traffic and ADD 15 - 19 % to its time - it is bound by its
 *                         memory instructions, which a wave issues while ANY lane needs them,
 *                         not by bytes - so the option is off. */
typedef struct pano_ctx pano_ctx;
#define PANO_OPT_BLUR_KERNEL 0
#define PANO_OPT_OWN_PRUNE 1
#define PANO_OPT_BLUR_SEGMENTS 2
#define PANO_OPT_BLUR_LEAN 3
#define PANO_OPT_STITCH_STREAMS 4
#define PANO_OPT_STITCH_ASYNC 5
#define PANO_OPT_BLUR_SEG_LEN 6
#define PANO_OPT_SIFT_GRAPH 7
#define PANO_OPT_LEVEL_CLASSES 8
#define PANO_OPT_COUNT 9
#define PANO_BLUR_MFMA 0
#define PANO_BLUR_VALU 1
int pano_ctx_create(int device, void *stream, pano_ctx **out);
int pano_ctx_destroy(pano_ctx *ctx);
int pano_ctx_set_stream(pano_ctx *ctx, void *stream);
int pano_ctx_set_option(pano_ctx *ctx, int option, int value);
int pano_ctx_get_option(const pano_ctx *ctx, int option, int *value);

/* Instrumentation for bench.py (no reference counterpart): when enabled every
 * kernel launch of this context is bracketed by HIP events recorded on its
 * stream.  pano_timing_read waits for kernel class `kid`'s events and returns
 * the summed duration in ms and the number of launches since the last enable. */
int pano_timing_enable(pano_ctx *ctx, int on);
int pano_kernel_count(void);
const char *pano_kernel_name(int kid);
int pano_timing_read(pano_ctx *ctx, int kid, double *total_ms, int *launches);

/* _add_weights                                        stitcher.py:251-263
 * frame uint8 [h][w][3] -> rgba float32 [h][w][4] interleaved (the array the
 * reference leaves in reg.img).  lut255: dev float[256] = float32(i)/255
 * (built on the host with NumPy); hat_x / hat_y: dev double[w] / [h]. */
int pano_add_weights(pano_ctx *ctx, const uint8_t *frame, int h, int w,
                     const float *lut255, const double *hat_x, const double *hat_y,
                     float *rgba);

/* Inverse map + mask + bilinear REFLECT remap of one whole patch
 *                                       stitcher.py:300-317 (+ cv2.remap)
 * proj: host double[9] = K R row-major (bundle_adj.py:31-33).
 * sin_t, cos_t: dev double tables over mosaic columns, tan_p over mosaic rows
 * (angles = index*resolution + min, stitcher.py:301-303, NumPy on the host).
 * (gx0, gy0) = patch origin in the mosaic, pw x ph = patch size.
 * Outputs: planes [4][ph][pitch] (alpha already multiplied by ~mask, :317),
 * mask [ph][pw]; map_x / map_y float [ph][pw] optional (NULL to skip). */
int pano_warp_spherical(pano_ctx *ctx, const uint8_t *frame, int sh, int sw,
                        const double *proj, const double *sin_t, const double *cos_t,
                        const double *tan_p, const float *lut255, const double *hat_x,
                        const double *hat_y, int gx0, int gy0, int pw, int ph,
                        float *planes, uint8_t *mask, float *map_x, float *map_y);

/* Same arithmetic, colour only, for window V of EVERY patch in one launch:
 * cams[i].frame is warped into patches[i].planes ([3][vh][vpitch]).  Alpha and
 * mask are not produced: the fused path gets them from
 * pano_ownership_cameras.  cams, patches: dev arrays of n records;
 * max_vw / max_vh: the largest window among them (sizes the grid).
 * need (optional): the per-tile flags pano_blur_tiles writes (one byte per 32 x 32
 * tile of every record, at patches[i].tiles_off, the grid being that of rectangle A with
 * the tiles of V's pixels outside it clamped to its border); every pixel of V whose tile is
 * needed is written, blocks of pixels none of whose tiles is needed may be left unwritten -
 * nothing reads them. */
int pano_warp_windows(pano_ctx *ctx, const pano_camera *cams, const pano_patch *patches,
                      int n, int max_vw, int max_vh, const double *sin_t,
                      const double *cos_t, const double *tan_p, const float *lut,
                      int lut_stride, const uint8_t *need);

/* Ownership + validity from warped patches   stitcher.py:196-204, 266-271
 * owner = first-index argmax of the patches' alpha plane (planes[3]), -1 where
 * all are 0; valid = OR over patches of ~mask.  patches: dev array of n
 * pano_patch with 4 planes and a mask, V = whole patch. */
int pano_ownership(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                   int16_t *owner, uint8_t *valid);

/* The same two maps straight from the cameras (no pixel data is read): for
 * every mosaic pixel in columns [xs0, xs1) and every camera whose patch
 * rectangle holds it, the inverse map, the mask and the bilinear alpha are
 * re-evaluated exactly as pano_warp_spherical does - but only for the cameras
 * that can still win: per 64 x 16 tile, cameras whose alpha is bounded (interval
 * arithmetic on the ray, rigorous) below another camera's lower bound are
 * skipped, which changes neither map (option PANO_OPT_OWN_PRUNE = 0 disables it).
 * cams: dev array. */
int pano_ownership_cameras(pano_ctx *ctx, const pano_camera *cams, int n, int H, int W,
                           int xs0, int xs1, const double *sin_t, const double *cos_t,
                           const double *tan_p, int16_t *owner, uint8_t *valid);

/* Where each patch owns pixels inside the column strip [xs0, xs1), one record
 * of 5 + 2*max_spans int32 per patch:
 *   {ymin, ymax, xmin, xmax, count, xa_0, xb_0, xa_1, xb_1, ...}
 * bounding box (inclusive, mosaic coordinates; ymax < ymin when the patch owns
 * nothing there) and `count` column spans [xa, xb]: runs of columns in which
 * the patch owns at least one pixel, runs closer than min_gap columns merged
 * (so that the spans' rectangles A stay disjoint), at most max_spans (later
 * runs are folded into the last span).  marks: dev uint8 [n][W] workspace. */
int pano_owned_regions(pano_ctx *ctx, const int16_t *owner, int H, int W, int xs0, int xs1,
                       int n, int min_gap, int max_spans, uint8_t *marks,
                       int32_t *regions);

/* pano_ownership_cameras and pano_owned_regions in one pass over the mosaic
 * (stitcher.py:196-204, 266-271 and the bookkeeping of the sharp masks of
 * :207-208): the ownership kernel leaves the cameras' boxes and column marks
 * behind while the owners are in its registers.  Same owner, valid and regions
 * as the two calls in sequence. */
int pano_ownership_regions(pano_ctx *ctx, const pano_camera *cams, int n, int H, int W,
                           int xs0, int xs1, const double *sin_t, const double *cos_t,
                           const double *tan_p, int16_t *owner, uint8_t *valid,
                           int min_gap, int max_spans, uint8_t *marks, int32_t *regions);

/* The n_levels-1 Gaussian blurs of every patch  stitcher.py:207-208, 218, 226
 * (cv2.GaussianBlur(warped, (0,0), 4*sqrt(2k+1)) with the alpha channel
 * replaced by the sharp mask owner == index), evaluated on rectangle A of each
 * patch from its colour planes over V, all levels, records and channels in one
 * launch (matrix-core kernel; the vector-ALU alternative runs one row pass for
 * all levels and one column pass per level through patches[i].scratch).
 * patches: dev array of n records with planes and blurred set (scratch only for
 * the vector-ALU kernels); max_aw / max_vh / max_ah: the largest extents.
 * taps: HOST float, n_blur tables laid out back to back; table k has
 * ntaps[k] + PANO_TAP_PAD floats: PANO_TAP_LEAD + ((R - r_k) & 3) zeros, the
 * ntaps[k] taps, zeros, where r_k = ntaps[k] / 2 and R = max r_k (the extra
 * zeros keep the row pass's 16-byte LDS reads aligned for every level).
 * ntaps: host int[n_blur].  Writes patches[i].blurred.  The context keeps a
 * device copy (and the matrix-core operand tables) of every tap set it has
 * seen, keyed on the apertures and the tap VALUES; the first call with a new
 * set uploads it in stream order, later calls only hash ~400 floats.
 * interior (optional, with tile_flags): the map of pano_interior_map; tiles
 * that hold only interior pixels (and the intermediate rows only they would
 * read) are skipped.  tile_flags: dev uint8, one entry per tile of every record,
 * record i's entries starting at patches[i].tiles_off, written here.  The tile
 * grid follows the context's PANO_OPT_BLUR_KERNEL, reported by pano_blur_tile_grid():
 *   32: 32 x 32 tiles anchored at multiples of 32 in patch coordinates, i.e.
 *       ((ax0+aw-1)>>5) - (ax0>>5) + 1 per row, ((ay0+ah-1)>>5) - (ay0>>5) + 1
 *       rows (the matrix-core kernel, default);
 *    0: 64-column x 128-row tiles relative to A, ceil(aw/64) per row,
 *       ceil(ah/128) rows (the vector-ALU kernels, PANO_BLUR_VALU).
 * The matrix-core kernel computes in split float16 (hi + lo, three products)
 * with float32 accumulation and does not use patches[i].scratch.
 * pano_multiband_blur_prepare (optional): the part of the call that depends on the
 * records' geometry and the interior map only (tile flags and the sorted work list of
 * the matrix-core kernel).  It may be queued on another stream while the warp fills the
 * planes; the caller orders it before the pano_multiband_blur call on the same table
 * (same patches pointer and n) with an event.  Without it pano_multiband_blur does
 * the same work itself.
 * pano_blur_tiles (optional, tile grid 32 only, before the two above, same stream order):
 * writes tile_flags from the interior map and warp_need = the tiles of window V whose
 * pixels the blur (its band fetches reach 16 ceil(radius / 16) columns and two tile rows
 * past an active tile) or the collapse will read, for pano_warp_windows; the following
 * prepare / blur call on the same table does not recompute the flags. */
int pano_blur_tile_grid(const pano_ctx *ctx);
int pano_blur_tiles(pano_ctx *ctx, const pano_patch *patches, int n, int max_aw,
                    int max_ah, int W, int radius, const uint8_t *interior,
                    uint8_t *tile_flags, uint8_t *warp_need);
int pano_multiband_blur_prepare(pano_ctx *ctx, const pano_patch *patches, int n,
                                int max_aw, int max_ah, int W, const uint8_t *interior,
                                uint8_t *tile_flags);
int pano_multiband_blur(pano_ctx *ctx, const pano_patch *patches, int n, int max_aw,
                        int max_vh, int max_ah, const int16_t *owner, int W,
                        const float *taps, const int *ntaps, int n_blur,
                        const uint8_t *interior, uint8_t *tile_flags);

/* Interior map (no reference counterpart: an exact-in-real-arithmetic property
 * of stitcher.py:210-241).  Where every pixel within `radius` (the largest
 * Gaussian radius) of p is owned by one patch, the band-pass stack telescopes:
 * all of that patch's blurred alphas equal the full tap sum, every other
 * patch's are exact zeros, and the multiband mosaic at p is the patch's warped
 * colour (to float32 rounding, <= 6e-8 absolute).  interior: dev uint8
 * [ceil(H/B)][ceil(W/B)], B = PANO_INTERIOR_BLOCK, 1 = every pixel of the B x B
 * block is such a pixel (conservative: tested on whole blocks); block_owner: dev
 * int16 workspace, twice that shape.  Only columns [xs0, xs1) of owner are read, and only the
 * blocks that meet those columns are written (one GPU's strip of the mosaic: the rest of
 * `interior` keeps whatever it held). */
int pano_interior_map(pano_ctx *ctx, const int16_t *owner, int H, int W, int xs0, int xs1,
                      int radius, int16_t *block_owner, uint8_t *interior);
/* The same test level by level (round 6).  radii: host int [n_radii], the Gaussian radii of the
 * levels, ascending (stitcher.py:218: the apertures grow with the level); classes: dev uint8, the
 * interior map's shape: the number of leading levels k whose (2 radii[k] + 1)^2 window around the
 * block holds one owner (0 .. n_radii; interior = the map at radii[n_radii - 1] = class n_radii).
 * For a pixel of class j >= 1 the levels below j telescope to  I - G_{j-1} I  of the owner alone:
 * pano_multiband_compose then gathers, of every record over the pixel, the colour of copy j - 1
 * and the copies j and up only - not the copies below, not alpha j - 1, and the warped planes of
 * the owner's record only (same result to float32 rounding, as for the interior pixels). */
int pano_interior_classes(pano_ctx *ctx, const int16_t *owner, int H, int W, int xs0, int xs1,
                          const int *radii, int n_radii, int16_t *block_owner, uint8_t *interior,
                          uint8_t *classes);

/* Host side of the fused path: the record table from the owned regions
 * (no reference counterpart; the arithmetic of "Windows" above).  regions: host copy
 * of pano_owned_regions' output, [n][5 + 2 max_spans]; rects: host int32 [n][4] =
 * patch rectangles (y0, y1, x0, x1) in mosaic coordinates; have (optional): [n], 0 =
 * that camera's frame is not resident; radius = the largest Gaussian radius;
 * [xs0, xs1) = the mosaic columns to produce; tile_grid = pano_blur_tile_grid() of the
 * context that will run the blur (32 or 0).  Writes one record per (camera, owned
 * column span) that reaches the strip, in camera order, with rectangles A and V,
 * pitches, tile offsets, and - until pano_layout_place - arena OFFSETS in the pointer
 * fields.  pano_layout_place turns them into addresses inside the three arenas
 * (blurred aligned up to 128 bytes; blurred / scratch may be NULL when unused). */
int pano_layout_windows(int tile_grid, const int32_t *regions, int n, int max_spans,
                        const int32_t *rects, const uint8_t *have, int radius,
                        int xs0, int xs1, int n_blur, pano_patch *records, int cap,
                        pano_layout *out);
int pano_layout_place(pano_patch *records, int n_records, void *planes, void *blurred,
                      void *scratch);

/* Band-pass build + collapse                     stitcher.py:210-241
 * Gathers, per mosaic pixel and in patch order, layer_k / wsum_k of every
 * level over the patches whose A holds the pixel, zeroes outside `valid`,
 * sums the levels, clips, truncates to uint8 - for the mosaic columns
 * [xs0, xs1) (the whole mosaic: 0, W; one GPU's share when the mosaic is split
 * into column strips).  mosaic / mosaic_f32 are full-size [H][W][3] buffers,
 * only the strip is written; mosaic_f32 is optional.
 * interior (optional): pixels of interior blocks are not gathered; the owner's
 * frame (cams[owner].frame) is sampled there exactly as the warp samples it,
 * which needs cams, the trig tables and the colour tables (all NULL
 * otherwise).
 * classes (optional, with interior): the level classes of pano_interior_classes - a pixel
 * of class j >= 1 gathers the copies j - 1 and up only (see there). */
int pano_multiband_compose(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                           int xs0, int xs1, int n_levels, const int16_t *owner,
                           const uint8_t *valid, const uint8_t *interior,
                           const uint8_t *classes, const pano_camera *cams,
                           const double *sin_t, const double *cos_t, const double *tan_p,
                           const float *lut, int lut_stride, uint8_t *mosaic,
                           float *mosaic_f32);

/* linear_blend (linear != 0) or no_blend (linear == 0) of the mosaic columns
 * [xs0, xs1) straight from the frames         stitcher.py:160-183 + :300-317
 * No patch is materialised: per mosaic pixel the covering cameras (UNPADDED
 * patch rectangles, stitcher.py:289-291) are mapped, sampled and combined in
 * index order.  cams: dev array with frame pointers set.  valid (optional,
 * dev uint8 [H][W]) receives _valid (stitcher.py:266-271) for the strip. */
int pano_blend_cameras(pano_ctx *ctx, const pano_camera *cams, int n, int H, int W,
                       int xs0, int xs1, int linear, const double *sin_t,
                       const double *cos_t, const double *tan_p, const float *lut,
                       int lut_stride, uint8_t *mosaic, uint8_t *valid);

/* Ghost-rejecting median blend of the mosaic columns [xs0, xs1) straight from the
 * frames (no reference counterpart; DESIGN.md section 5m is the contract).  The samples
 * of a pixel are what pano_blend_cameras' linear blend combines, in index order: colour
 * c_i, alpha a_i of every covering, unmasked camera.  With the integer weights
 * w_i = trunc(clamp(a_i, 0, 1) 2^30), T = sum w_i and the keys k_i = (c_i[0] + c_i[1]) + c_i[2],
 * the median sample j is the first, in ascending (k_i, i) order over the samples with
 * w_i > 0, whose running weight S satisfies 2 S >= T; a sample is an inlier when
 * |c_i[ch] - c_j[ch]| <= tol in all three channels (every sample when T = 0), and the pixel
 * is the linear blend over the inliers in index order.  Where all samples agree that is
 * pano_blend_cameras' linear mosaic bit for bit.  A pixel may have any number of samples:
 * beyond PANO_MEDIAN_KEEP the sorted order is consumed in passes, never truncated.
 * tol >= 0.  lut, lut_stride, valid: as for pano_blend_cameras. */
int pano_median_cameras(pano_ctx *ctx, const pano_camera *cams, int n, int H, int W,
                        int xs0, int xs1, float tol, const double *sin_t,
                        const double *cos_t, const double *tan_p, const float *lut,
                        int lut_stride, uint8_t *mosaic, uint8_t *valid);

/* The same blend on warped patches (whole-patch planes, as pano_linear_blend): a patch
 * contributes a sample where its mask is 0. */
int pano_median_blend(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                      float tol, uint8_t *mosaic);

/* Overlap statistics of equalize_gains           stitcher.py:36-63
 * For each pair, every pixel (x, y) of frame i is looked up in frame j as
 * cv2.warpPerspective(img_j, hom, (w, h), INTER_LINEAR, BORDER_TRANSPARENT)
 * does on the float32 RGBA image (OpenCV semantics restated, parity unpinned):
 * in double, with x = xb + x1, xb = (x / bw0) * bw0 the column-block start,
 *   W = 32 / (m6*xb + m7*y + m8 + m6*x1)          (0 if the denominator is 0)
 *   X = cvRound(clamp_int((m0*xb + m1*y + m2 + m0*x1) * W)),  Y likewise,
 * taps (X >> 5, Y >> 5) saturated to int16, fractions X & 31, Y & 31; the pixel
 * is written only if all four taps lie inside frame j; the bilinear sum runs
 * left to right in float32.  A pixel counts where the sampled alpha (analytic,
 * float32(hat_y*hat_x) per tap) is non-zero (stitcher.py:58).
 * All frames must be h x w (the reference sizes everything by regions[0],
 * stitcher.py:41).  bw0 = min(1024 / min(16, h), w) (WarpPerspectiveInvoker's
 * block width).  lut255: dev float[256], float32(u8)/255.
 * partials: dev double [n_pairs][pano_overlap_blocks(h, w)][3] workspace.
 * stats: dev double [n_pairs][3] = {pixel count (stitcher.py:59), sum of
 * frame i's colours over those pixels and the 3 channels, sum of the sampled
 * colours of frame j}; the means of stitcher.py:62-63 are sum / (3 count).
 * Sums are taken in double in a fixed order (the reference's np.mean sums in
 * float32 pairwise; the two agree to ~1e-7 relative). */
int pano_overlap_blocks(int h, int w);
int pano_overlap_stats(pano_ctx *ctx, const pano_camera *cams, const pano_pair *pairs,
                       int n_pairs, int h, int w, int bw0, const float *lut255,
                       double *partials, double *stats);

/* linear_blend on warped patches                        stitcher.py:171-183 */
int pano_linear_blend(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                      uint8_t *mosaic);

/* no_blend                                              stitcher.py:160-168 */
int pano_no_blend(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                  uint8_t *mosaic);

/* crop_mosaic rectangle                                 stitcher.py:340-369
 * valid: dev uint8 [H][W].  heights: dev int32 [H][W] workspace.
 * result: dev int64[6] = {found, y0, x0, h, w, area}. */
int pano_crop_rect(pano_ctx *ctx, const uint8_t *valid, int H, int W, int32_t *heights,
                   int64_t *result);

/* Separable symmetric filter on one float plane, BORDER_REFLECT_101
 *                     cv2.GaussianBlur at features.py:24 / stitcher.py:226
 * taps: HOST padded table of one aperture (layout and caching as for
 * pano_multiband_blur); tmp: dev [h][pitch]. */
int pano_blur_plane(pano_ctx *ctx, const float *src, float *dst, float *tmp, int h, int w,
                    int pitch, const float *taps, int ntaps);

/* cv2.pyrDown on one float plane                        features.py:155
 * src [h][w] (dense) -> dst [(h+1)/2][(w+1)/2] (dense). */
int pano_pyr_down(pano_ctx *ctx, const float *src, int h, int w, float *dst);

/* Scale-space building blocks of the SIFT detector the reference obtains from
 * OpenCV (features.py:192-201); with pano_blur_plane they make the Gaussian and
 * difference-of-Gaussian pyramid (pano360_amd/features.py: sift_pyramid).
 * OpenCV semantics restated, parity unpinned (see csrc/pyramid.hip).
 *   pano_gray_u8     cvtColor(BGR2GRAY) on uint8 [h][w][3] -> float [h][w]
 *   pano_resize_up2  resize(2w x 2h, INTER_LINEAR): float [h][w] -> [2h][2w]
 *   pano_decimate2   resize(w/2 x h/2, INTER_NEAREST): float [h][w] -> [h/2][w/2]
 *   pano_subtract    out = a - b over n floats (one DoG layer) */
int pano_gray_u8(pano_ctx *ctx, const uint8_t *bgr, int h, int w, float *out);
/* One step of buildGaussianPyramid + buildDoGPyramid, fused (csrc/scalespace.hip):
 *   dst = GaussianBlur(src, taps) (REFLECT_101; both passes in one launch, the row-pass
 *   image stays in LDS), dog (optional) = dst - src.
 * src, dst, dog: dev float [h][w] dense, distinct; taps: HOST float[ntaps] (the bare kernel
 * of cv::getGaussianKernel, no padding), ntaps odd and <= 33 (sigma <= 4). */
int pano_scale_step(pano_ctx *ctx, const float *src, int h, int w, const float *taps, int ntaps,
                    float *dst, float *dog);
/* The whole scale space of one frame in ONE call (createInitialImage + buildGaussianPyramid
 * + buildDoGPyramid): grey -> 2x bilinear -> blur to sigma, then per octave n_layers + 2
 * pano_scale_step launches and the nearest-neighbour halving of layer n_layers into the
 * next octave.  frame: dev uint8 [h][w][3]; octave o is rows_o x cols_o with rows_0 = 2h,
 * cols_0 = 2w, halved (floor) from octave to octave, all >= 1; gauss / dog: HOST arrays of
 * n_octaves dev pointers, gauss[o] = float [n_layers+3][rows_o][cols_o], dog[o] likewise
 * with n_layers+2; taps: HOST float, n_layers + 3 bare kernels back to back (kernel 0: the
 * base blur, kernel i: the step into layer i), ntaps: HOST their apertures;
 * work: dev float [5 h w] scratch (grey image, doubled base). */
int pano_scale_space(pano_ctx *ctx, const uint8_t *frame, int h, int w, int n_octaves,
                     int n_layers, const float *taps, const int *ntaps, float *const *gauss,
                     float *const *dog, float *work);
int pano_resize_up2(pano_ctx *ctx, const float *src, int h, int w, float *dst);
int pano_decimate2(pano_ctx *ctx, const float *src, int h, int w, float *dst);
int pano_subtract(pano_ctx *ctx, const float *a, const float *b, size_t n, float *out);

/* Decimated Laplacian-pyramid blending of two images     blend.py:105-140
 * (blend.laplacian_blending: cv2.pyrDown / cv2.pyrUp pyramids of two float32
 * images and a float64 mask, la*gm + lb*(1-gm) per level in float64, collapse,
 * clip, uint8).  Images are interleaved [h][w][c], c <= 4, dense; is_f64 selects
 * double (the mask and everything after the mix) or float (the image pyramids).
 * OpenCV's pyrDown / pyrUp restated, parity unpinned (csrc/laplacian.hip).
 *   pano_pyr_down_image  cv2.pyrDown: [h][w][c] -> [(h+1)/2][(w+1)/2][c]
 *   pano_pyr_up_image    cv2.pyrUp(src)[:oh, :ow] (blend.py:126,138), combined with
 *                        `other` [oh][ow][c]: mode 0 = the up-sampled image,
 *                        1 = other - up (a Laplacian level), 2 = other + up (collapse)
 *   pano_u8_to_f32       img.astype("float32")                        blend.py:132-133
 *   pano_laplacian_mix   out = la*gm + lb*(1.0 - gm) in the mask's type   blend.py:136
 *                        (float64 against the default / a float64 mask, float32 against a
 *                        float32 mask, as NumPy promotes them)
 *   pano_clip_u8         np.clip(x, 0, 255).astype("uint8")             blend.py:140 */
int pano_pyr_down_image(pano_ctx *ctx, const void *src, int h, int w, int c, int is_f64,
                        void *dst);
int pano_pyr_up_image(pano_ctx *ctx, const void *src, int sh, int sw, int c, int is_f64,
                      const void *other, int mode, void *dst, int oh, int ow);
int pano_u8_to_f32(pano_ctx *ctx, const uint8_t *src, size_t n, float *dst);
int pano_laplacian_mix(pano_ctx *ctx, const float *la, const float *lb, const void *gm, size_t n,
                       int is_f64, void *out);
int pano_clip_u8(pano_ctx *ctx, const void *src, size_t n, int is_f64, uint8_t *dst);

/* Poisson (seamless cloning) blend of two uint8 images          blend.py:143-203
 * (blend.poisson_blend: per channel the sparse system A sol = b, one unknown per pixel, and
 * target = np.array(np.clip(sol, 0, 255), uint8).)  The reference factorises A; this call
 * iterates BiCGStab in float64 on the pixel grid and builds no matrix (csrc/poisson.hip).
 *   src, tgt   dev uint8 [h][w][c] interleaved, c <= 4; tgt is overwritten at the mask pixels
 *   mask       dev uint8 [h][w], nonzero = a pixel to solve (the reference's img_mask != 0)
 * The system, with i = y w + x, N = h w, "flat neighbours" n in {i-1, i+1, i-w, i+w} kept when
 * 0 <= n < N (so a row's last pixel and the next row's first are neighbours), as the
 * reference's spdiags calls with their zeroed slots make it (poisson_matrix, :143-172):
 *   b    outside the mask tgt[i]; inside 4 src[i] - src[n] over the flat neighbours whose
 *        COLUMN is not w-1: nobody reads the last column, and a last-column pixel reads only
 *        i-1 and i+1.
 *   A    identity rows outside the mask; a mask row is 4 on the diagonal and -1 at the flat
 *        neighbours, without i+1 when x == w-2 and without i-1 when x == 0.  A pixel at
 *        x == w-1 keeps i+1 (a wrap link) and both vertical neighbours.  Not symmetric.
 * Solver: x0 = tgt, unpreconditioned BiCGStab (the diagonal is constant on the mask, Jacobi
 * scaling changes nothing), every vector, dot product and scalar float64, scalars and flags in
 * device memory, all channels in the same launches, a converged channel frozen.  A channel
 * stops when ||r||_2 <= rtol ||b||_2 with r the recurrence's residual and b the whole right-hand
 * side, identity rows included.  The host queues PANO_POISSON_CHUNK iterations at a time and
 * reads the channels' flags back once per chunk.  Sums have a fixed order (per lane, xor
 * butterfly per wave, waves in order, blocks' partials in order; no atomics): the same input
 * gives the same bits.
 *   rtol, max_iters   the stopping threshold and the iteration cap (per channel)
 *   solution   dev double [c][h][w] or NULL: the float64 solution, every pixel
 *   iters, resid   HOST int32 [c] / double [c] or NULL: iterations used and the final
 *              ||r|| / ||b|| per channel, also written when the call fails
 * Returns PANO_ESOLVE when a channel reaches max_iters unconverged or BiCGStab breaks down
 * (rho, omega or (rhat, v) at zero, a scalar that is not finite); tgt is then untouched.  The
 * call waits for the stream (the readbacks); scratch is the context's and grows on demand. */
#define PANO_POISSON_CHUNK 32
int pano_poisson_blend(pano_ctx *ctx, const uint8_t *src, uint8_t *tgt, const uint8_t *mask,
                       int h, int w, int c, double rtol, int max_iters, double *solution,
                       int32_t *iters, double *resid);

/* The overlap seam: blend.graph_cut of the reference             blend.py:56-100
 * (not a min-cut but a two-marker priority flood: cells leave a heap of (-difference, colour,
 * x, y) smallest first and hand their colour to their unlabelled 4-neighbours), in three calls
 * (csrc/graphcut.hip), and blend.alpha_blend (blend.py:48-53).
 *
 * pano_seam_levels   the priorities ("levels") of the flood, higher first: per pixel
 *     max over channels |img1 - img2|, -1 where a fourth channel is 0 in either image, cropped
 *     to a multiple of shrink and reduced by the MINIMUM over shrink x shrink cells ->
 *     level dev int16 [h / shrink][w / shrink], -1 .. 255.  img1, img2: dev [h][w][c]
 *     interleaved, c <= 4, of one dtype (PANO_SEAM_*), holding integers 0 .. 255; *bad (dev
 *     int32, zeroed by the call) becomes 1 when a value is not one.  PANO_SEAM_U8 restates what
 *     the reference's uint8 arithmetic does: the difference wraps (3 - 5 = 254), and so does
 *     the heap key -difference (-0 = 0, -d = 256 - d), which orders the differences 0, 255,
 *     254, .. 1; the level is therefore 255 for a pooled difference of 0 and d - 1 otherwise
 *     (c == 4 is refused for uint8: the reference cannot store its -1 there).
 * pano_seam_flood    labels dev int8 [rows][cols] from the levels.  Presets (blend.py:74-80):
 *     columns [0, border) and the seed column `border` are -1, the seed column cols - border
 *     and columns (cols - border, cols) are +1; border >= 2, cols >= 2 border + 1.  The heap's
 *     order is a pure function of the data and the labels depend only on the order of the
 *     CLASSES (level descending, colour -1 before +1): while (d, c) is the smallest class
 *     waiting, every entry the flood creates has colour c and those of a level >= d sort before
 *     everything of the other colour.  So for d = 255 .. -1 and c = -1, +1 the call labels with c
 *     every connected component of unlabelled cells of level >= d that touches a c-labelled
 *     cell - at most 514 closures, each a data-parallel fill, bit-identical to the heap loop.
 *     A closure alternates row and column passes; a pass spreads c over every maximal run of
 *     open cells that holds a cell with a c neighbour (a 64-cell ballot per wave, carries
 *     between a line's chunks), until a pass labels nothing.  Levels that do not occur are
 *     skipped; a class without a frontier costs the one pass that finds none.
 *     path 0: by size, 1: resident - the grid and a one-cell wall live in the LDS of ONE
 *     1024-thread workgroup (two bytes a cell, (rows + 2)(cols + 2) <= PANO_SEAM_RESIDENT_CELLS),
 *     which runs every class without leaving the kernel; 2: tiled - 64 x 64 tiles with a
 *     one-cell halo flood to their own fixed point in LDS and write back, one launch per round,
 *     a class ends with the round in which no tile changed; the class and the "changed" word
 *     live in device memory and the host reads one word per PANO_SEAM_BATCH queued rounds.
 *     A cell only ever goes from 0 to the colour of the running class, so the races between
 *     waves (and tiles) are benign: no atomics, the same bits on every run.
 *     stats (optional, dev int32 [4]): classes that labelled a cell, passes (resident) or
 *     rounds (tiled) that labelled one, the most of them in one class, the path taken.
 * pano_seam_mask     cv2.resize of the float32 plane (labels == -1) to [h][w], INTER_LINEAR,
 *     times 255, truncated to uint8 (blend.py:99-100).  OpenCV's float path restated (parity
 *     unpinned: a build that fuses the multiply-add can differ by one grey level where a value
 *     sits within an ulp of an integer): xtab / ytab dev int32 [w][4] / [h][4] = (first tap,
 *     second tap, bits of the float32 weight of the first, of the second), built by the host;
 *     s0 a0 + s1 a1 along x, then r0 b0 + r1 b1 along y, one rounding per operation.
 * pano_alpha_blend   (img1 mask + img2 (1 - mask)) truncated to uint8: two products and one sum,
 *     unfused, in NumPy's promoted type (float64, or float32 when the mask is float32 and the
 *     images are uint8, int16 or float32); 1 - mask in the mask's own type.  img1, img2 as
 *     for pano_seam_levels (any values), mask dev float32 / float64 read at
 *     y mask_sy + x mask_sx + k mask_sc (0 = broadcast), out dev uint8 [h][w][c]. */
#define PANO_SEAM_U8 0
#define PANO_SEAM_I16 1
#define PANO_SEAM_I32 2
#define PANO_SEAM_F32 3
#define PANO_SEAM_F64 4
#define PANO_SEAM_RESIDENT_CELLS 81408
#define PANO_SEAM_BATCH 64
int pano_seam_levels(pano_ctx *ctx, const void *img1, const void *img2, int dtype, int h, int w,
                     int c, int shrink, int16_t *level, int32_t *bad);
int pano_seam_flood(pano_ctx *ctx, const int16_t *level, int rows, int cols, int border,
                    int path, int8_t *labels, int32_t *stats);
int pano_seam_mask(pano_ctx *ctx, const int8_t *labels, int rows, int cols,
                   const int32_t *xtab, const int32_t *ytab, uint8_t *mask, int h, int w);
int pano_alpha_blend(pano_ctx *ctx, const void *img1, const void *img2, int dtype,
                     const void *mask, int mask_f64, int64_t mask_sy, int64_t mask_sx,
                     int64_t mask_sc, int h, int w, int c, uint8_t *out);

/* Seam routing in front of the multiband blend (csrc/seam_route.hip; no reference counterpart;
 * DESIGN.md section 5t; tests/seam_route_model.py restates all of it in NumPy, heap loop included).
 * The stage-level multiband path takes any owner map; these calls rewrite pano_ownership's inside
 * the zones two cameras contest, so that the seam runs where the two agree.
 *
 * Per mosaic pixel, from the patch table pano_ownership takes (n <= PANO_SEAM_ROUTE_MAX_CAMERAS):
 *   a      owner0 at the pixel (first-index argmax of alpha, -1 where every alpha is 0)
 *   b      the camera other than a with the largest alpha > 0 there, lowest index on ties, else -1
 *   D      where b >= 0: max over the 3 colour channels of |qa - qb|, q = uint8(255.0f * c), the
 *          truncation of pano_no_blend; 0 elsewhere
 *   open   the pixel is valid (some patch's mask is 0 there), a >= 0, b >= 0 and
 *          alpha_b >= ratio * alpha_a (one float32 product).  Every other valid pixel with
 *          a >= 0 is a SEED, labelled a for good; the rest are WALLS.
 * Two cameras COMPETE when some open pixel has them as {a, b}; group[c] is the smallest
 * non-negative integer no lower-indexed competitor of c uses (greedy colouring in index order, on
 * the host), so the two cameras an open pixel admits - a and b, no others - are of different
 * groups, and cameras of one group admit no common pixel.
 * Flood: pop the smallest (-D, group[c], c, y, x) from a heap; label the pixel c if it is still
 * unlabelled; push its unlabelled open 4-neighbours that admit c.  As for pano_seam_flood the
 * labels depend only on the order of the CLASSES (D descending, group ascending): for d = 255 .. 0
 * and g = 0 .. n_groups - 1, and every camera c of group g, each 4-connected component of
 * unlabelled open pixels with D >= d that admit c and that touches a pixel labelled c becomes c.
 * Result: the label, a where an open pixel was never reached, -1 on walls: every owner is a camera
 * with alpha > 0 at its pixel.
 *
 * pano_seam_route_prepare   one thread per mosaic pixel over the patch table.  owner0: dev int16
 *     [H][W], pano_ownership's.  Writes second (b) dev int16 [H][W], diff (D) dev uint8 [H][W],
 *     label dev int16 [H][W] (a on seeds, -1 on open pixels, -2 on walls), pairs dev uint8 [n][n]
 *     (pairs[a][b] = 1 for the open pixels' (a, b); zeroed by the call) and present dev uint8 [256]
 *     (present[D] = 1 for the open pixels' D; zeroed by the call).  0 < ratio <= 1.  present is
 *     for the caller's information (how many classes the flood will walk): the flood takes plain
 *     planes, which may be forged, and reads the levels that occur off them itself.
 * pano_seam_route_flood     the class sweep on plain planes (a, second, diff as above; label is
 *     the flood's state and is updated in place: what is still -1 afterwards was never reached).
 *     group: HOST int32 [n], 0 <= group[c] < n_groups; the two cameras of an open pixel must be of
 *     different groups (an index outside [0, n) admits nothing).  64 x 64 tiles with a one-cell halo
 *     flood to their own fixed point of the running class in LDS and write back, one launch per
 *     round, a one-thread kernel between the rounds keeps the class while the round's "changed"
 *     word was set and else takes the next class whose level occurs; the host reads one word per
 *     PANO_SEAM_BATCH queued rounds.  A cell only ever goes from -1 to the one label its class
 *     admits, so stale reads between waves and tiles only delay a label: no atomics, the same
 *     bytes on every run.  owner_out dev int16 [H][W] (may be a).  stats (optional, dev int32 [4]):
 *     classes that labelled a cell, rounds that labelled one, the most of them in one class,
 *     pixels whose owner is not a.  Waits for the stream (the reads of "done").
 * pano_seam_route           pano_ownership, the prepare, the download of pairs, the colouring,
 *     the flood: owner dev int16 [H][W], valid dev uint8 [H][W] (pano_ownership's); stats
 *     (optional, dev int32 [6]): the flood's four, the open pixels, the groups.  The planes in
 *     between are the context's. */
#define PANO_SEAM_ROUTE_MAX_CAMERAS 4096
int pano_seam_route_prepare(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                            const int16_t *owner0, float ratio, int16_t *second, uint8_t *diff,
                            int16_t *label, uint8_t *pairs, uint8_t *present);
int pano_seam_route_flood(pano_ctx *ctx, const int16_t *a, const int16_t *second,
                          const uint8_t *diff, int16_t *label, const int32_t *group, int n,
                          int n_groups, int H, int W, int16_t *owner_out, int32_t *stats);
int pano_seam_route(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W, float ratio,
                    int16_t *owner, uint8_t *valid, int32_t *stats);

/* cv2.resize(im, None, fx=1/shrink, fy=1/shrink) on a uint8 image   stitcher.py:419-420
 * (INTER_LINEAR, OpenCV's 8-bit fixed-point path restated; parity unpinned).
 * xtab / ytab: dev int32 [ow][4] / [oh][4] = (first tap, second tap, coefficient of
 * the first, of the second; 11-bit fixed point), built by the host exactly as the
 * oracle builds them.  Both NULL: the exact 2:1 reduction, which cv2.resize takes by
 * rounded 2 x 2 box means (sh == 2 oh, sw == 2 ow). */
int pano_resize_u8(pano_ctx *ctx, const uint8_t *src, int sh, int sw, int c,
                   const int32_t *xtab, const int32_t *ytab, uint8_t *dst, int oh, int ow);

/* Keypoints and descriptors of SIFT_create().detectAndCompute  features.py:192-198
 * (the arithmetic lives in OpenCV's xfeatures2d/sift.cpp, restated with the
 * SIFT_create() defaults; parity unpinned).  The scale space comes from the
 * building blocks above, one contiguous stack per octave:
 * gauss[o] = dev float [n_layers+3][rows_o][cols_o], dog likewise with n_layers+2;
 * dims = dev int32 {rows_0, cols_0, rows_1, cols_1, ...}.
 *   pano_sift_extrema   findScaleSpaceExtrema + adjustLocalExtrema of one octave:
 *                       refined extrema (angle 0, coordinates of the doubled base
 *                       image, octave index not yet shifted) appended at
 *                       cands[atomicAdd(count)] while below max_cands.
 *   pano_sift_orient    calcOrientationHist: every candidate becomes one keypoint
 *                       per dominant orientation, appended to kpts.  n_cands: dev.
 *   pano_sift_describe  calcSIFTDescriptor of n keypoints as detectAndCompute
 *                       returns them (full-resolution coordinates, octave field
 *                       shifted by first_octave): desc dev float [n][128], values
 *                       0..255.  RootSIFT (features.py:198) is left to the caller.
 * List order is arbitrary (atomics); pano_sift_sort_unique puts it into OpenCV's:
 *   pano_sift_sort_unique  KeyPointsFilter::removeDuplicatedSorted + the first-octave
 *                       adjustment of detectAndCompute: the n keypoints of pano_sift_orient
 *                       sorted by x, y, size (descending), angle, response (descending),
 *                       octave (descending), the first of every (x, y, size, angle) group
 *                       kept, positions and sizes scaled by 2^first_octave and the octave
 *                       byte shifted by first_octave -> out (dev, room for n), *n_out (dev).
 *                       work: dev scratch of pano_sift_sort_work_bytes(n) bytes.
 * n_dev (optional, pano_sift_sort_unique and pano_sift_describe): a device int holding the
 * real count, at most n - the host then passes the capacity as n and never waits for the
 * counters pano_sift_orient / pano_sift_sort_unique leave on the device. */
int pano_sift_extrema(pano_ctx *ctx, const float *dog, int rows, int cols, int octave,
                      int n_layers, float contrast_thr, float edge_thr, float sigma,
                      pano_sift_keypoint *cands, int *count, int max_cands);
int pano_sift_orient(pano_ctx *ctx, const float *const *gauss, const int *dims,
                     int n_layers, const pano_sift_keypoint *cands, const int *n_cands,
                     int max_cands, pano_sift_keypoint *kpts, int *count, int max_kpts);
int pano_sift_describe(pano_ctx *ctx, const float *const *gauss, const int *dims,
                       int first_octave, const pano_sift_keypoint *kpts, int n,
                       const int *n_dev, float *desc);
size_t pano_sift_sort_work_bytes(int n);
int pano_sift_sort_unique(pano_ctx *ctx, const pano_sift_keypoint *kpts, int n, const int *n_dev,
                          int first_octave, void *work, pano_sift_keypoint *out, int *n_out);

/* One frame of the detector's front end per call           features.py:192-201 (_detect)
 * = pano_scale_space, then - with `detect` - pano_sift_extrema for every octave,
 * pano_sift_orient, pano_sift_sort_unique and pano_sift_describe, in that order on the
 * context's stream, nothing waited for: the candidate / keypoint / kept counts stay on the
 * device in counts[0..2] (zeroed here).  Every launch's grid and arguments follow from the
 * frame size and the buffers alone, so with PANO_OPT_SIFT_GRAPH (default) the sequence is
 * captured into a HIP graph the second time a set of buffers comes by and replayed afterwards:
 * `frame_copy` (dev, h * w * 3 bytes, optional) is the frame buffer the graph reads - the
 * caller's frame is copied into it in front of every replay; without it, or while kernels are
 * being timed, the sequence is queued launch by launch.  Results are the same either way.
 * Buffers: as the entry points named above take them; gauss / dog: host arrays of n_octaves
 * device pointers; gauss_dev / dims_dev: the device arrays pano_sift_orient reads; the result:
 * cands (the kept keypoints, OpenCV's order), desc, counts[2]. */
typedef struct pano_sift_args {
    const uint8_t *frame;      /* dev uint8 [h][w][3]                                   */
    uint8_t *frame_copy;       /* dev, same size: the graph's own frame buffer, or NULL  */
    int32_t h, w, n_octaves, n_layers;
    const float *taps;         /* host: the n_layers + 3 kernels of pano_scale_space     */
    const int32_t *ntaps;      /* host [n_layers + 3]                                    */
    float *const *gauss;       /* host [n_octaves] of dev float [n_layers + 3][rows][cols] */
    float *const *dog;         /* host [n_octaves] of dev float [n_layers + 2][rows][cols] */
    float *work;               /* dev, 5 h w floats                                      */
    int32_t detect;            /* 0 = the scale space only                               */
    float contrast_thr, edge_thr, sigma;
    int32_t first_octave, max_keypoints;
    const float *const *gauss_dev;   /* dev [n_octaves]: the pointers of `gauss`         */
    const int32_t *dims_dev;         /* dev [n_octaves][2]: rows, cols                   */
    pano_sift_keypoint *cands, *kpts;   /* dev [max_keypoints] each                      */
    int32_t *counts;           /* dev int32 [3]: candidates, keypoints, kept             */
    void *sort_work;           /* dev, pano_sift_sort_work_bytes(max_keypoints)          */
    float *desc;               /* dev float [max_keypoints][128]                         */
} pano_sift_args;
int pano_sift_detect(pano_ctx *ctx, const pano_sift_args *args);
/* 1 when the most recently used set of buffers of pano_sift_detect is replayed as a graph */
int pano_sift_detect_replaying(const pano_ctx *ctx);

/* The two nearest rows of `train` for every row of `query` (Euclidean), the search behind
 * flann_matching                                                  features.py:222-232
 * (cv2.FlannBasedMatcher().knnMatch(des1, des2, k=2): FLANN's randomised kd-trees give an
 * approximate answer; this search is exhaustive and its answer exact).  The cross terms of
 * |q - t|^2 run on the matrix cores in split float16 and only rank the candidates; the
 * four best per query are re-evaluated in float32 (sum of squared differences) and a bound
 * on the ranking error proves that no other row can be among the best two - a query whose
 * proof fails is rescanned exactly (counted in *rescans, optional dev int).
 * A distance is the float32 sum of squared differences in one fixed order, then sqrtf.
 * query: dev float [nq][d], train: dev float [nt][d], nt >= 2, d <= 128; scale: a finite
 * power of two with max |value| * scale <= 2048 over both sets (the float16 high halves stay
 * finite, the products far below float32's range) and max |train value| * scale >= 2^-3
 * (below that the low halves are float16 denormals whose rounding the error bound no longer
 * covers; the values are not inspected, so a scale outside this interval is not refused and
 * the answer may then be inexact); work: dev scratch of pano_knn2_work_bytes(nq, nt, d)
 * bytes, contents ignored.  idx: dev int32 [nq][2], dist: dev float [nq][2], nearest first
 * (equal distances: lower index first). */
size_t pano_knn2_work_bytes(int nq, int nt, int d);
int pano_knn2(pano_ctx *ctx, const float *query, int nq, const float *train, int nt, int d,
              float scale, void *work, int32_t *idx, float *dist, int *rescans);

/* Lowe's ratio test over one pair's pano_knn2 result, packed for pano_hom_ransac
 *                                                  features.py:232-243
 * Query q survives iff (double) dist[q][0] < ratio * (double) dist[q][1] (strict; the reference
 * compares cv2.DMatch distances in Python floats).  The survivors are written in ascending query
 * order (a stable compaction) to pts (dev float [nq][4]: the query keypoint x, y, then its
 * nearest train keypoint's x, y) and match (dev int32 [nq][2]: q, idx[q][0]); their number goes
 * to *count (dev int32).  The capacity of pts / match is nq rows, so the caller sizes a pair's
 * region on the host with no wait; only the survivors' rows are written: rows *count .. nq - 1
 * and everything behind them keep what they held, so pairs can be packed back to back in one
 * buffer.  A NaN distance never survives (the comparison is false).  idx, dist: dev [nq][2] of
 * pano_knn2 (idx[q][1] is not read); kp_query, kp_train: dev float [nq][2] / [nt][2] (centred
 * keypoints); a train index outside [0, nt) never survives.  nq = 0: only *count = 0 is written
 * and the other pointers may be null.  pts 16-byte aligned, dist and the keypoints 8-byte
 * aligned.  One launch, nothing waited for; a refused call (PANO_EINVAL) writes nothing. */
int pano_match_pack(pano_ctx *ctx, const int32_t *idx, const float *dist, int nq, double ratio,
                    const float *kp_query, const float *kp_train, int nt, float *pts,
                    int32_t *match, int32_t *count);

/* RANSAC homographies of a batch of pairs                       features.py:244
 * (cv2.findHomography(src, dst, cv2.RANSAC), restated; not pinned against OpenCV).
 *   pts        dev float [m][4]: src x, y, dst x, y, all pairs packed, 16-byte aligned
 *   offsets    dev int32 [n_pairs]: first row of each pair in pts
 *   counts     dev int32 [n_pairs]: rows of each pair (< 4: the pair fails)
 *   work       dev, pano_hom_ransac_work_bytes(n_pairs, max_iters) (may be NULL with hyp_inliers)
 *   hom        dev double [n_pairs][9], row-major, hom[8] = 1; zeros on failure
 *   mask       dev uint8 [m]: 1 = inlier of the best hypothesis; zeros on failure
 *   n_inliers  dev int32 [n_pairs]: inliers of the best hypothesis; 0 on failure
 *   hyp_inliers  optional dev int32 [n_pairs][max_iters]: every hypothesis's score (-1: invalid)
 * Kernels on the context's stream and nothing else (no allocation, no wait, no host copy): the
 * call may be captured into a graph.  Semantics, so that a model can reproduce every score:
 * - Sampler.  Draw k (0..3) of attempt a (0..63) of hypothesis h (0..max_iters-1) of a pair of
 *   `count` rows is ((r >> 32) * count) >> 32 with r = splitmix64(seed + G * (h * 256 + a * 4 + k
 *   + 1)) in uint64 arithmetic, G = 0x9E3779B97F4A7C15 and splitmix64(x): z = x + G;
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.
 *   The key does not involve the pair's index or the batch: a pair's result is the same alone
 *   and in any batch.
 * - Degeneracy.  An attempt is rejected unless its four indices are distinct and, for each
 *   triple (0,1,2), (0,1,3), (0,2,3), (1,2,3), the signed areas of the src and of the dst
 *   triangle, (xb - xa) * (yc - ya) - (yb - ya) * (xc - xa) in f64, have a product > 0 (collinear
 *   triples, flipped orientation and NaN all reject).  The first accepted attempt is the sample;
 *   after 64 rejected attempts the hypothesis is invalid.
 * - Hypothesis.  The exact 4-point homography in f64, h33 = 1: rows [x, y, 1, 0, 0, 0, -(u x),
 *   -(u y) | u] and [0, 0, 0, x, y, 1, -(v x), -(v y) | v] per point, Gaussian elimination with
 *   partial pivoting (column c: the first row r >= c of maximal |a_rc|, a NaN counting as
 *   maximal; swap; a_rk = a_rk - (a_rc / a_cc) * a_ck for r > c, k > c), back substitution
 *   (s = b_r; s = s - a_rk * h_k for k = r+1 .. 7; h_r = s / a_rr).  A zero or non-finite pivot
 *   makes the hypothesis invalid.
 * - Score.  Hf = the hypothesis rounded to float32; t2 = float32(float64(thresh)^2); in float32,
 *   one rounding per operation, left to right: ww = 1 / ((Hf6 x + Hf7 y) + 1),
 *   dx = ((Hf0 x + Hf1 y) + Hf2) * ww - u, dy likewise with Hf3..5 and v, err = dx dx + dy dy;
 *   an inlier iff err <= t2.  Every hypothesis is scored (no adaptive stop).
 * - Selection.  The most inliers, the lowest h of a tie.  mask is its inlier set (not re-tested
 *   after the refit).
 * - Refit.  Over the best hypothesis's inliers: Hartley normalisation (centroid to the origin,
 *   mean distance sqrt 2, per image), the DLT's 9 x 9 normal matrix in f64 summed in a fixed
 *   order, its smallest eigenvector (cyclic Jacobi), denormalised, scaled to h33 = 1.  The same
 *   input gives the same bits on every run.  No Levenberg-Marquardt polish.
 * - Failure.  count < 4, no valid hypothesis, fewer than 4 inliers, or a non-finite refit:
 *   hom, n_inliers and the pair's mask are zero. */
size_t pano_hom_ransac_work_bytes(int n_pairs, int max_iters);
int pano_hom_ransac(pano_ctx *ctx, const float *pts, const int32_t *offsets, const int32_t *counts,
                    int n_pairs, int max_iters, float thresh, uint64_t seed, void *work,
                    double *hom, uint8_t *mask, int32_t *n_inliers, int32_t *hyp_inliers);

/* Bundle adjustment: the per-match work of the Levenberg-Marquardt loop  bundle_adj.py:311-345
 * All arithmetic is f64; the host derives every 3 x 3 table (in NumPy, in the reference's
 * operation order) and uploads it once per iteration, the device forms only sums of products.
 *   rows    dev double [m][4]: (x_b, y_b, x_a, y_a) per match, the homogeneous 1s implicit; the
 *           columns 0..1 and 3..4 of the reference's match rows (stitcher.py:372-386)
 *   pairs   dev int32 [n_pairs][4]: (a, b, first, count), the reference's match tuple
 *           (a, b, rows) of IncrementalBundleAdjuster.matches (:306) in its order; the pair's
 *           rows are rows[first .. first + count).  Camera b is the reference's `i` / "from",
 *           camera a its `j` / "to" in _jacobian_symbolic (:199-205).
 *   hom     dev double [n_pairs][9], row-major: H = K_b R_b R_a^T K_a^-1 (_hom_to_from, :36-38)
 * A matrix times p = (x_a, y_a, 1) is (m0 x_a + m1 y_a) + m2 per row, a matrix times a vector
 * v is (m0 v0 + m1 v1) + m2 v2, with one rounding per operation (no contraction).
 *
 * pano_ba_residuals: ssq[p] (dev double [n_pairs]) = the pair's sum over its matches of
 *   rx^2 + ry^2, rx = x_b - X / Z, ry = y_b - Y / Z, (X, Y, Z) = H p - get_diff (:145-149)
 *   summed per pair.  loss (:158-160) and the gate of `add` (:304) follow on the host.
 *   Summation: lane t of a block of 256 takes the pair's matches t, t + 256, ... in order; the
 *   64 lanes of a wave by an xor butterfly (offsets 32, 16, .. 1), the four waves in order.
 *
 * pano_ba_normal: the damped system (J^T J + lambda I) delta = J^T r of one iteration
 *   (:322-327) over the active cameras.  slot: dev int32 [n_cameras], the parameter block of
 *   each camera (-1: inactive; every camera of a pair is active); the parameters are the active
 *   cameras in ascending index, 6 each in camera_to_params's order (:138-142): f, ppx, ppy,
 *   then the three exponential-map angles.  J is _jacobian_symbolic as written (:186-258), NOT
 *   the derivative of the residual.  jtab: dev double [n_pairs][90], ten row-major 3 x 3
 *   matrices per pair, all at the state J is taken at:
 *     [0]     H                                   (:203)
 *     [1]     S_b = (R_b R_a^T) K_a^-1            (:219)
 *     [2]     S_r = R_a^T K_a^-1                  (:227)
 *     [3]     K_a^-1                              (:233)
 *     [4..6]  N_k = K_b dR_b[k]                   (:228-230, dR = dr_dvi, :163-177)
 *     [7..9]  Q_k = (K_b R_b) dR_a[k]^T           (:240-243)
 *   Per match: (X, Y, Z) = H p, iz = 1 / Z, d = (X iz iz, Y iz iz, -iz) (:208-210) and a column
 *   of J from w = (w0, w1, w2) is (w0 d2 + w2 d0, w1 d2 + w2 d1) (:212-215).  Columns 0..5 are
 *   camera b's: s = S_b p gives w = (s0, s1, 0), (s2, 0, 0), (0, s2, 0) for f, ppx, ppy (the dK
 *   products of :222-224 written out), N_k (S_r p) for the angles; columns 6..11 camera a's:
 *   n = -(K_a^-1 p) gives w_r = (H_r0 n0 + H_r1 n1) + 0 n2, (0 n0 + 0 n1) + H_r0 n2 and
 *   (0 n0 + 0 n1) + H_r1 n2 (H dK, :236-238), Q_k (K_a^-1 p) for the angles.
 *   TWO STATES.  r is the residual at hom_r (dev double [n_pairs][9], H at the state r is
 *   taken at), J at the state of jtab.  The reference takes J at its accepted cameras but r is
 *   `errs`, the residual of the last CANDIDATE (:314, :335): after a rejected step J^T r pairs J
 *   at the accepted state with r at the rejected one, and the caller reproduces that by passing
 *   the rejected candidate's H here.
 *   Summation.  ba_pair_kernel, one block per pair: per chunk of 256 matches the 90 products
 *   of each lane are summed over the wave (the butterfly above) and lane 0 adds each sum to its
 *   wave's running total, chunk by chunk; the four waves' totals are added in order into
 *   work[p][90]: [0..20] J_b^T J_b and [21..41] J_a^T J_a (upper triangles, row-major),
 *   [42..77] J_b^T J_a (6 x 6, row-major), [78..89] J^T r (camera b's 6, then camera a's 6).
 *   ba_assemble_kernel, one block per 6 x 6 block of the system: starting from 0, the pairs are
 *   added in pair order (the cross block of a pair at (b, a), its transpose at (a, b), :249-256),
 *   then lambda on the diagonal (:324).  jtj: dev double [6 n_active][6 n_active] row-major,
 *   every entry written; jtr: dev double [6 n_active].  work: dev, pano_ba_work_bytes(n_pairs).
 * Both calls queue kernels on the context's stream and nothing else (no allocation, no wait, no
 * host copy).  No atomics: the same input gives the same bits on every run.  The caller keeps
 * first + count within rows and every camera index within slot. */
size_t pano_ba_work_bytes(int n_pairs);
int pano_ba_residuals(pano_ctx *ctx, const double *rows, const int32_t *pairs, int n_pairs,
                      const double *hom, double *ssq);
int pano_ba_normal(pano_ctx *ctx, const double *rows, const int32_t *pairs, int n_pairs,
                   const int32_t *slot, int n_active, const double *jtab, const double *hom_r,
                   double lambda, void *work, double *jtj, double *jtr);

/* Robust refinement of registered cameras with a shared radial distortion  (bundle_adj.refine)
 * Not the reference's: the stage after traverse.  Per pair the Huber-weighted normal equations of
 * the reprojection error, J the TRUE derivative of the residual.  f64, one rounding per operation,
 * sqrt the only function called.  ONE launch, no atomics, no allocation, no wait.
 *   rows    dev double [n_rows][4], pairs dev int32 [n_pairs][4]: as pano_ba_residuals takes them
 *           (coordinates centred on the image; count may be 0)
 *   cams    dev double [n_cameras][12]: f, px, py, then R row-major (world -> camera)
 *   k1, k2  the radial coefficients, shared by all cameras; delta: the Huber threshold, pixels
 * undist(c, x, y): d = ((x - px_c) / f_c, (y - py_c) / f_c), rd = sqrt(d0 d0 + d1 d1); r solves
 *   h(r) = r ((1 + k1 r^2) + k2 r^4) = rd by exactly 10 Newton steps r <- r - (h(r) - rd) / h'(r)
 *   from r = rd, h'(r) = (1 + 3 k1 r^2) + 5 k2 r^4; s = rd > 0 ? r / rd : 1; the result is
 *   u = s d: the inverse of the forward Brown radial model of pano_lens_undistort_u8.
 * Residual of a match: q = (u_a, 1), v = R_b (R_a^T q), pi = (v0 / v2, v1 / v2),
 *   e = f_b (u_b - pi): pixels of camera b's corrected image.
 * A match is INVALID when an h' met (the ten steps' and the one at the solution, of either
 *   camera) is <= 0, when v2 <= 0, or when e or an entry of J is not finite; so is every match of
 *   a pair that names a camera outside [0, n_cameras) or rows outside [0, n_rows), which reads
 *   nothing.  An invalid match adds to out[p][67] and to nothing else.
 * J, 2 x 10, by the local parameters (f_b, omega_b[3], f_a, omega_a[3], k1, k2), the
 *   perturbations f + df and R <- exp([omega]x) R at omega = 0, through the Newton solution by the
 *   implicit function theorem (dr/drd = 1 / h', dr/dk1 = -r^3 / h', dr/dk2 = -r^5 / h'):
 *     du/df  = -d / (h' f)        du/dk1 = -(s r^2) d / h'        du/dk2 = r^2 du/dk1
 *     P w    = ((w0 - pi0 w2) / v2, (w1 - pi1 w2) / v2)           (the derivative of pi, on w)
 *     M w    = R_b (R_a^T w)
 *     f_b:       (u_b - pi) - d_b / h'_b
 *     omega_b,k: -f_b P (e_k x v)
 *     f_a:       -f_b P M (du_a/df_a, 0)
 *     omega_a,k: +f_b P M (e_k x q)
 *     k1, k2:    f_b (du_b/dk - P M (du_a/dk, 0))
 * With n = |e|: w = n <= delta ? 1 : delta / n, rho = n <= delta ? n^2 / 2 : delta (n - delta / 2).
 * out: dev double [n_pairs][70], every entry written, per pair over its valid matches:
 *     [0..54]  sum of (w J_c)^T J_e, c <= e: the upper triangle of sum w J^T J, row-major
 *     [55..64] sum of (w J)^T e      [65] sum rho      [66] sum w      [67] invalid matches
 *     [68] sum n^2 over the matches with n <= delta    [69] the number of those
 * Summation: one block of 256 per pair; thread t adds the pair's matches t, t + 256, ... in
 *   order to its own 70 sums, from 0; then per sum the 64 lanes of a wave by the xor butterfly
 *   (offsets 32, 16, .. 1) and the four waves as (w0 + w1) + (w2 + w3).  The same input gives the
 *   same bytes on every call.
 * PANO_EINVAL, with nothing launched and out untouched: a null pointer, n_pairs < 1,
 *   n_cameras < 1, n_rows < 0, a delta that is not finite or not positive. */
int pano_ba_refine(pano_ctx *ctx, const double *rows, int64_t n_rows, const int32_t *pairs,
                   int n_pairs, const double *cams, int n_cameras, double k1, double k2,
                   double delta, double *out);

/* Baseline JPEG decode of a batch                               stitcher.py:415-421 (cv2.imread)
 * Frames equal to libjpeg-turbo's default decompression as Pillow runs it, bit for bit, after
 * ImageOps.exif_transpose and convert("RGB"), written as uint8 BGR [h][w][3].  Scope: SOF0 /
 * SOF1, 8-bit, Huffman, one interleaved scan, 1 component or 3 in YCbCr with the luma sampled
 * 1x1, 2x1 or 2x2 and both chroma 1x1 (4:4:4, 4:2:2, 4:2:0), restart markers or none, any size,
 * EXIF orientation 1..8, quantisers <= 255.  The IDCT runs in int32: bit-exact while the
 * dequantised coefficients stay within 16 bits, which every encoder's output from 8-bit samples
 * does (libjpeg-turbo's own C and SIMD IDCTs disagree beyond that).  Limits: entropy data of an
 * image < 2^28 bytes, packed_bytes < 2^31 (pano360_amd/jpeg.py splits larger sets).  The host (pano360_amd/jpeg.py) parses the markers and lays the batch
 * out; this call does everything after that.
 *   desc     host int64 [n + 1][PANO_JPEG_FIELDS]: n image rows (PANO_JD_*), then the batch row
 *            (PANO_JB_*).  The same table is the head of `packed` (the device reads it there).
 *   packed   dev uint8 [packed_bytes]: desc, then per image its tables at PANO_JD_TAB_OFF (4 DC
 *            and 4 AC Huffman lookups of PANO_JPEG_HUFF_BYTES: fast[512] uint16 = length << 8 |
 *            symbol of every 9-bit prefix holding a code of <= 9 bits, else 0; maxcode[18] int32
 *            (-1: no code of that length); valoff[18] int32 = index of the length's first symbol
 *            minus its first code; vals[256] uint8; then 4 quantisation tables uint16 [64] in
 *            natural order) and its entropy-coded bytes (between SOS and EOI) at PANO_JD_DATA_OFF
 *   work     dev scratch of desc's PANO_JB_WORK_BYTES, laid out by desc (destuffed bytes,
 *            planes, and the PANO_JB_W_* arrays); out: dev uint8, frame i at PANO_JD_OUT_OFF.
 * Stages, each a kernel on the context's stream:
 *   1. destuff: per chunk of PANO_JPEG_CHUNK raw bytes the bytes kept and RSTn markers met
 *      (FF 00 -> FF; FF Dn and fill FFs dropped), an exclusive scan over all chunks, then the
 *      kept bytes written and every restart interval's first byte recorded.
 *   2. Huffman, self-synchronising (Weissenberger & Schmidt, ICPP 2018): each interval is cut in
 *      subsequences of PANO_JPEG_SUBSEQ bits.  The first of an interval starts in the known state
 *      (bit 0, block 0 of the MCU, coefficient 0); the others start at their first bit in that
 *      state as a guess.  Each decodes to the first codeword boundary at or past its end and
 *      records the state there (bit, block in MCU, coefficient, blocks completed).  Then, one
 *      launch per round, every subsequence whose predecessor's exit changed decodes again from
 *      that exit; the host reads one flag per round and stops when no exit changed (round r
 *      makes the first r + 1 subsequences of every interval exact, so it ends).  A scan of the
 *      completed-block counts places each subsequence's blocks; a last pass writes the
 *      coefficients (int16 [64], natural order, the DC as a difference).  Reads beyond an
 *      interval's end see zero bits; blocks past an interval's MCU count are dropped.
 *   3. DC prediction: per interval and component, a prefix sum of the differences in MCU order.
 *   4. Dequantise and ISLOW IDCT (CONST_BITS 13, PASS1_BITS 2), 8 lanes per block; the output
 *      through libjpeg's range-limit table: clamp(wrap10(v) + 128, 0, 255) with wrap10 the
 *      10-bit two's-complement wrap of the descaled value.
 *   5. Pixels: per output pixel, the EXIF orientation folded into the indexing; fancy
 *      upsampling of the chroma (the triangle filter, replicated edges; a plane of <= 2 samples
 *      across is replicated instead) and YCbCr -> RGB in libjpeg's 16-bit fixed point.
 * Every result has one writer and the scans run in a fixed order: the same input gives the same
 * bits on every run.  The call waits on the stream once per synchronisation round (it is not
 * capturable).  The host row fields are checked against the buffer sizes before anything is
 * queued; a malformed entropy stream gives wrong pixels, never a read or write outside them. */
#define PANO_JPEG_FIELDS 32
#define PANO_JPEG_CHUNK 1024
#define PANO_JPEG_SUBSEQ 1024
#define PANO_JPEG_HUFF_BYTES 1424
enum {  /* image row */
    PANO_JD_W, PANO_JD_H, PANO_JD_NC, PANO_JD_HMAX, PANO_JD_VMAX, PANO_JD_MCUX, PANO_JD_MCUY,
    PANO_JD_RI,        /* MCUs per restart interval, 0: none */
    PANO_JD_NINT,      /* restart intervals */
    PANO_JD_BPM,       /* blocks per MCU */
    PANO_JD_ORIENT, PANO_JD_DATA_OFF, PANO_JD_DATA_LEN, PANO_JD_TAB_OFF,
    PANO_JD_CHUNK0,    /* first chunk, interval, block, pixel of the image */
    PANO_JD_INT0,
    PANO_JD_SUB0,      /* running sum of the images' subsequence-slot capacities (entropy bits /
                          PANO_JPEG_SUBSEQ + intervals + 1): checked, it sizes PANO_JB_SUBS; the
                          slots themselves are assigned by the scan of the intervals' counts */
    PANO_JD_BLK0, PANO_JD_PIX0,
    PANO_JD_DST_OFF,   /* work: destuffed bytes */
    PANO_JD_PLANE0, PANO_JD_PLANE1, PANO_JD_PLANE2,   /* work: sample planes, whole blocks */
    PANO_JD_PITCH0, PANO_JD_PITCH1, PANO_JD_PITCH2,
    PANO_JD_OUT_OFF,
    PANO_JD_COMP_U,    /* 2 bits per block of the MCU: its component */
    PANO_JD_SAMP,      /* byte per component: h | v << 4 */
    PANO_JD_TABSEL     /* byte per component: DC table | AC table << 2 | quant table << 4 */
};
enum {  /* batch row */
    PANO_JB_N, PANO_JB_CHUNKS, PANO_JB_INTS, PANO_JB_SUBS, PANO_JB_BLOCKS, PANO_JB_PIXELS,
    PANO_JB_OUT_BYTES, PANO_JB_W_KEPT, PANO_JB_W_RST, PANO_JB_W_KEPTX, PANO_JB_W_RSTX,
    PANO_JB_W_DSTLEN, PANO_JB_W_ISTART, PANO_JB_W_IEND, PANO_JB_W_INSUB, PANO_JB_W_ISUBX,
    PANO_JB_W_STATE0, PANO_JB_W_STATE1, PANO_JB_W_CNTX, PANO_JB_W_FLAG, PANO_JB_W_COEF,
    PANO_JB_WORK_BYTES, PANO_JB_PACKED_BYTES
};
int pano_jpeg_decode(pano_ctx *ctx, const int64_t *desc, int n, const uint8_t *packed,
                     int64_t packed_bytes, void *work, int64_t work_bytes, uint8_t *out,
                     int64_t out_bytes);

/* Baseline JPEG encode of one image                              stitcher.py:446-447 (cv2.imwrite)
 * The entropy-coded segment libjpeg-turbo 3.x writes with its defaults as Pillow runs them
 * (Image.save(f, "JPEG", quality=, subsampling=)), bit for bit: 8-bit, 3 components YCbCr from
 * RGB, one interleaved scan, no restart markers, the Annex K Huffman tables.  The host
 * (pano360_amd/jpeg.py) makes the quantisation tables and the markers around the segment.
 *   img          dev uint8, pixel (x, y) at img[y * pitch + 3 x], channels R, G, B (flags 0) or
 *                B, G, R (PANO_JPEG_BGR); pitch >= 3 w, any other value (a cropped view needs no
 *                copy).  The caller guarantees (h - 1) * pitch + 3 w readable bytes.
 *   h, w         1 .. PANO_JPEG_MAX_SIDE (libjpeg's JPEG_MAX_DIMENSION)
 *   subsampling  luma sampling, the chroma 1x1: 0 = 1x1 (4:4:4), 1 = 2x1 (4:2:2), 2 = 2x2 (4:2:0)
 *   qt           host uint8 [2][64]: luma then chroma quantisers, natural order, 1 .. 255
 *   work         dev scratch of pano_jpeg_encode_work_bytes(h, w, subsampling) bytes (0: bad
 *                size).  It starts with the quantised blocks: int16 [blocks][64], zigzag order,
 *                the DC not differenced, in scan order (MCU by MCU; in an MCU the luma blocks
 *                row by row, then Cb, then Cr).
 *   *stream, *stream_bytes   out: the entropy-coded segment (stuffed, padded), in pinned host
 *                memory the context owns, valid until its next pano_jpeg_encode or its
 *                destruction.
 * Stages, each a kernel on the context's stream:
 *   1. blocks, 8 lanes per block: jccolor.c's 16-bit fixed-point RGB -> YCbCr; the last column
 *      and row replicated; chroma downsampled h2v1 ((a + b + bias) >> 1, bias 0, 1, ...) or h2v2
 *      ((a + b + c + d + bias) >> 2, bias 1, 2, ...) over those samples, and below the last
 *      downsampled h2v2 row that row again; the ISLOW FDCT (CONST_BITS 13, PASS1_BITS 2);
 *      rounded division by 8 q, the sign applied after.  A block of an MCU beyond its
 *      component's blocks across or down is jccoefct.c's dummy: AC zero, the DC of the block
 *      before it.
 *   2. bit counts, one wave per block: a ballot of the nonzero coefficients gives every lane
 *      its run; DC difference per component in scan order, run/size codes, ZRL, EOB.
 *   3. an exclusive scan of the counts into int64 bit offsets (a stream may pass 2^31 bits).
 *      The call waits for the total.
 *   4. emission, one wave per block: the block's bits assembled in LDS, MSB first; the words
 *      wholly inside the block stored, its two boundary words atomicOr'ed into the zeroed
 *      stream (integer, disjoint bits: order-free); the last byte padded with 1-bits.
 *   5. stuffing: 0xFF bytes counted per 64-byte chunk, the counts scanned (the call waits for
 *      the total), every byte written at its shifted place with a 0x00 after each 0xFF.
 * Then the stuffed bytes are copied to the host and the call waits for that.  Not capturable.
 * The raw stream and the stuffed stream grow inside the context.  The same input gives the same
 * bytes on every run.  Sizes, pitch, flags and quantisers are checked before anything is
 * queued. */
#define PANO_JPEG_MAX_SIDE 65500
#define PANO_JPEG_BGR 1
size_t pano_jpeg_encode_work_bytes(int h, int w, int subsampling);
int pano_jpeg_encode(pano_ctx *ctx, const uint8_t *img, int h, int w, int64_t pitch, int flags,
                     int subsampling, const uint8_t *qt, void *work, int64_t work_bytes,
                     const uint8_t **stream, int64_t *stream_bytes);

/* Baseline JPEG encode of a batch                          the tiles of pano360_amd/tiles.py
 * n images of any sizes in one call; for every image on its own the contract of pano_jpeg_encode
 * holds (its stream is the bytes that call returns for it).  The sampling, the channel order and
 * the quantisers are the batch's.
 *   images       host pano_jpeg_image [n]: img (dev), pitch, h, w as in pano_jpeg_encode; an
 *                image may be a crop view of a larger one (a tile is not copied).  The call
 *                uploads the table.
 *   n            1 .. PANO_JPEG_BATCH_MAX; all images together at most
 *                PANO_JPEG_BATCH_MAX_BLOCKS blocks (dummy blocks included)
 *   work         dev scratch of pano_jpeg_encode_batch_work_bytes(blocks, n) bytes (0: bad
 *                size), blocks the sum over the images of MCUs x blocks per MCU.  It starts with
 *                the quantised blocks of all images, image after image, as in pano_jpeg_encode.
 *   *streams     out: the n entropy-coded segments (stuffed, padded) one after the other
 *   *offsets     out: int64 [n + 1], image i's segment is (*streams)[(*offsets)[i] ..
 *                (*offsets)[i + 1]).  Both in pinned host memory the context owns, valid until
 *                its next pano_jpeg_encode or pano_jpeg_encode_batch or its destruction.
 * The five stages of pano_jpeg_encode run over the batch as a whole, the blocks of all images
 * numbered one after the other:
 *   - a block finds its image by bisecting the table of the images' first blocks (int32 [n + 1],
 *     uploaded with the descriptors), once per block and stage; workgroups straddle images.  Edge
 *     replication, dummy blocks and the DC prediction (zero at an image's first MCU) are the
 *     image's own.
 *   - one scan of all blocks' bit counts; an image's bits are the difference of the offsets at
 *     its ends.  A kernel over the images turns them into bytes (padded with 1-bits to a whole
 *     byte, by the image's last block) and 64-byte stuffing chunks, and a second, small scan
 *     gives every image its first chunk: an image's raw bits start on a chunk of its own, never
 *     byte-packed behind its neighbour, so no word, pad bit or 0xFF of one image is seen with
 *     another's.  The call waits for the chunk total (wait 1).
 *   - stuffing: a chunk's count is its stream bytes plus its 0xFF bytes, so the scan of the
 *     counts is the position in the output, where the streams are packed byte after byte; an
 *     image's first chunk also writes offsets[i].  The call waits for the stuffed size (wait 2).
 * Then the offsets and the streams are copied to the host in one copy and the call waits for
 * that: two waits and one download whatever n is.  Not capturable.  The same input gives the same
 * bytes on every run.  n, sizes, pitches, flags, quantisers, the block total and the scratch
 * size are checked before anything is queued. */
#define PANO_JPEG_BATCH_MAX 16384
#define PANO_JPEG_BATCH_MAX_BLOCKS (1 << 28)
typedef struct pano_jpeg_image {
    const uint8_t *img;
    int64_t pitch;
    int32_t h, w;
} pano_jpeg_image;
size_t pano_jpeg_encode_batch_work_bytes(int64_t blocks, int n);
int pano_jpeg_encode_batch(pano_ctx *ctx, const pano_jpeg_image *images, int n, int flags,
                           int subsampling, const uint8_t *qt, void *work, int64_t work_bytes,
                           const uint8_t **streams, const int64_t **offsets);

/* PNG output: the scanline filters and a deflate coder            stitcher.py:446-447 (cv2.imwrite)
 * A PNG cannot be zlib's bytes (its match search is serial); the contract is: the file decodes
 * to exactly the image's pixels, the same input gives the same bytes on every run, and the file
 * is about as small as Pillow's.  The host (pano360_amd/png.py) wraps the stream as zlib data
 * and cuts it into the container's chunks.
 *
 * pano_png_filter: the scanlines of an 8-bit RGB PNG, filtered.  Asynchronous on the stream.
 *   img          dev uint8, pixel (x, y) at img[y * pitch + 3 x], channels R, G, B (flags 0) or
 *                B, G, R (PANO_PNG_BGR); pitch >= 3 w (a cropped view needs no copy).  The caller
 *                guarantees (h - 1) * pitch + 3 w readable bytes.
 *   filtered     dev uint8 [h][1 + 3 w]: per row the filter's number, then the filtered bytes in
 *                R, G, B order
 * All five filters at 3 bytes per pixel: bytes left of the row and the row above row 0 count as
 * 0, Average is (left + up) >> 1, Paeth breaks ties in the order left, up, upper left.  Per row
 * the filter with the smallest sum of the filtered bytes' absolute values as signed 8-bit
 * wins, the first minimum in the order 0 .. 4.  One workgroup per row, every candidate from the
 * unfiltered neighbours: rows are independent.
 *
 * pano_deflate: a raw deflate stream (RFC 1951) of a device byte buffer, and its Adler-32.
 *   data, n      dev bytes, 0 <= n < PANO_DEFLATE_MAX_BYTES (2^34)
 *   work         dev scratch of pano_deflate_work_bytes(n) bytes (0: bad size)
 *   *stream, *stream_bytes   out: the stream, in pinned host memory the context owns, valid
 *                until its next pano_deflate or its destruction
 *   *adler       out: Adler-32 of data
 * The stream is one dynamic-Huffman block per PANO_DEFLATE_CHUNK input bytes (n = 0: one empty
 * block), concatenated bit by bit without alignment, BFINAL on the last.  Stages:
 *   1. runs: maximal runs of equal bytes over the whole buffer.  A run's first byte is a
 *      literal; the rest is matches of length 3 .. 258 at distance 1, a leftover of 1 - 2 bytes
 *      literals.  Tokens are cut at chunk borders; a match may reach the byte before its chunk,
 *      never before byte 0.  One workgroup per chunk holds it in LDS; a thread finds the run
 *      starts of its 64 bytes as a mask, two scans give it the starts around them.
 *   2. per chunk: literal/length and distance histograms by integer LDS atomics (order-free);
 *      code lengths limited to 15 bits, the code-length alphabet to 7, both optimal under the
 *      limit (package-merge, see pano_deflate_lengths); the lengths run-length coded with the
 *      16 / 17 / 18 repeat codes, HCLEN order; the dynamic-block header; the chunk's bit count;
 *      Adler-32 partial sums (a, b) of the chunk.
 *   3. an exclusive scan of the bit counts into int64 bit offsets (a stream may pass 2^31
 *      bits).  The call waits for the total, and combines the Adler partials in order.
 *   4. emission, LSB first, canonical codes: a thread writes its tokens' bits at their offset,
 *      words wholly inside its range stored, its first and last word atomicOr'ed into the
 *      zeroed stream (integer, disjoint bits: order-free); the header likewise.
 * Then the stream is copied to the host and the call waits for that.  Not capturable.
 *
 * pano_deflate_lengths: the length-limited code builder as a stage of its own.
 *   freq         dev uint32 [n_sym], their sum below 2^32;  lengths  dev uint8 [n_sym]
 *   n_sym        1 .. 288, at most 2^max_bits;  max_bits  1 .. 15
 * Zero frequency <=> length 0; one used symbol gets length 1; otherwise the lengths minimise
 * sum freq * length under the limit and their Kraft sum is exactly 1.  Asynchronous. */
#define PANO_PNG_BGR 1
#define PANO_DEFLATE_CHUNK 65536
#define PANO_DEFLATE_MAX_BYTES ((int64_t)1 << 34)
int pano_png_filter(pano_ctx *ctx, const uint8_t *img, int h, int w, int64_t pitch, int flags,
                    uint8_t *filtered);
size_t pano_deflate_work_bytes(int64_t n);
int pano_deflate(pano_ctx *ctx, const uint8_t *data, int64_t n, void *work, int64_t work_bytes,
                 const uint8_t **stream, int64_t *stream_bytes, uint32_t *adler);
int pano_deflate_lengths(pano_ctx *ctx, const uint32_t *freq, int n_sym, int max_bits,
                         uint8_t *lengths);

/* The MSOP detector                                  features.py:27-156, 204-212 (csrc/msop.hip)
 * OpenCV's cornerHarris / Sobel / warpPerspective restated, parity unpinned; the arithmetic is
 * stated in NumPy in tests/msop_model.py and in DESIGN 5i.  All planes dense float [h][w].
 * pano_harris      features.py:140: cornerHarris(gray, blockSize 2, ksize 3, k) -> out, fused
 *     (Sobel / 8, REFLECT_101; the products; the 2 x 2 box sum, anchor (1, 1);
 *     a c - b b - k (a + c)(a + c) left to right).
 * pano_sobel       features.py:112-113: the unscaled Sobel 3 x 3 planes dx, dy (REFLECT_101).
 * pano_msop_smooth features.py:20-24, 112-114: cv2.GaussianBlur of one plane (REFLECT_101) in the
 *     operation order of OpenCV's sepFilter2D, multiply and add rounded separately - row pass
 *     s = k[0] x[0]; s += k[j] x[j] ascending, column pass s = k[r] y[0];
 *     s += k[r + j] (y[+j] + y[-j]) - so that g_x, g_y and the blurred plane equal the model
 *     bit for bit (pano_blur_plane's FMA sums differ in the last bit).  taps: HOST float [ntaps]
 *     (cv::getGaussianKernel), ntaps odd, at most PANO_MSOP_SMOOTH_TAPS; tmp, dst dev [h][w];
 *     dst may be src.
 * pano_msop_candidates  features.py:142: the pixels >= their 8 neighbours, compacted in row-major
 *     order: keys (order-preserving uint32 of the response, -0 = +0), pos (y w + x), both dev
 *     [h w]; *count dev.  work: pano_msop_candidates_work_bytes bytes.
 * pano_msop_cut    features.py:143-146: one stable ascending sort of the n candidates (equal
 *     responses stay in row-major order) and the last `keep` of them as points dev int32
 *     [keep][2] = (row, col), weakest first.  work: pano_msop_cut_work_bytes(n) bytes.
 * pano_ssc_probe   features.py:71-89: ONE greedy walk of ssc over points dev int32 [n][2] in
 *     order, for the grid of one width: cgr = width / 2, a point's cell is
 *     (floor(p[1] / cgr), floor(p[0] / cgr)) in double - the reference's swap - in a grid of
 *     (n_cell_rows + 1) x (n_cell_cols + 1) cells; a point whose cell is uncovered is taken and
 *     covers the cells within `reach` of its own, clipped.  sel dev int32 [n]: the indices taken,
 *     in order; *count dev.  One wave walks 64 points a step.  path PANO_SSC_AUTO: by size,
 *     PANO_SSC_ONCHIP: the coverage bitmap in LDS (at most PANO_SSC_ONCHIP_CELLS cells),
 *     PANO_SSC_GLOBAL: in work, pano_ssc_probe_work_bytes bytes (may be NULL on the on-chip
 *     path).  A point outside the grid is never taken.  The scalar search around the probes
 *     (features.py:36-69, 91-97) is the host's.
 * pano_msop_describe  features.py:116-128 for the n points points[sel[i]] (sel NULL: points[i]),
 *     one wave each: theta = atan2f(gx, gy) at the point; the 8 x 8 tile of `blurred` turned by
 *     theta (x = cs (u - 4) + sn (v - 4) + col, y = -sn (u - 4) + cs (v - 4) + row in double,
 *     cs = (float)cos((double)theta); 5-bit fixed-point bilinear taps, constant border 0);
 *     (t - mean) / (std + 1e-8) with NumPy's pairwise float32 sums.  Out, all dev: points_out
 *     double [n][4] = (scale row, scale col, theta, scale), theta float [n], tiles float [n][64]
 *     (each optional), desc float [n][64]. */
#define PANO_SSC_AUTO 0
#define PANO_SSC_ONCHIP 1
#define PANO_SSC_GLOBAL 2
#define PANO_SSC_ONCHIP_CELLS 524288
#define PANO_MSOP_SMOOTH_TAPS 15
int pano_harris(pano_ctx *ctx, const float *gray, int h, int w, float k, float *out);
int pano_sobel(pano_ctx *ctx, const float *gray, int h, int w, float *dx, float *dy);
int pano_msop_smooth(pano_ctx *ctx, const float *src, int h, int w, const float *taps, int ntaps,
                     float *tmp, float *dst);
size_t pano_msop_candidates_work_bytes(int h, int w);
int pano_msop_candidates(pano_ctx *ctx, const float *hrs, int h, int w, void *work,
                         uint32_t *keys, uint32_t *pos, int *count);
size_t pano_msop_cut_work_bytes(int n);
int pano_msop_cut(pano_ctx *ctx, const uint32_t *keys, const uint32_t *pos, int n, int keep,
                  int w, void *work, int32_t *points);
size_t pano_ssc_probe_work_bytes(int n_cell_rows, int n_cell_cols);
int pano_ssc_probe(pano_ctx *ctx, const int32_t *points, int n, double cgr, int n_cell_rows,
                   int n_cell_cols, int reach, int path, void *work, int32_t *sel,
                   int32_t *count);
int pano_msop_describe(pano_ctx *ctx, const float *gx, const float *gy, const float *blurred,
                       int h, int w, const int32_t *points, const int32_t *sel, int n, int scale,
                       double *points_out, float *theta, float *tiles, float *desc);

/* Views of a finished mosaic        (the reference ends with cv2.imshow, stitcher.py:449-451:
 * a person looks at the mosaic; here a renderer does, csrc/view.hip)
 * A mosaic of H x W pixels samples the sphere at theta = low[0] + x res[0], phi = low[1] + y res[1]
 * (Plan.__init__, SphProj.hom2proj: theta = atan2(x, z), phi = atan2(y, hypot(x, z)); the frame is
 * x right, y down, z forward).  It is CLOSED when |W res[0] - 2 pi| < res[0] / 2: column W is
 * column 0 again.
 *
 * pano_mip_u8: the mip chain of a uint8 [h][w][3] image whose rows are `pitch` bytes apart.
 *     Level 0 is the image, level l + 1 is ((h_l + 1) / 2, (w_l + 1) / 2), a pixel
 *     (a + b + c + d + 2) >> 2 over its 2 x 2 block with the odd index clamped to the last row or
 *     column; the levels stop at 1 x 1 or at PANO_VIEW_MAX_LEVELS.  mips: dev, level l dense at
 *     mips + offsets[l]; offsets: HOST int64 [n_levels + 1], ascending, offsets[l + 1] >=
 *     offsets[l] + 3 h_l w_l (the last entry is the buffer's size); n_levels must be the chain's
 *     length.  One copy and n_levels - 1 launches, asynchronous on the stream.
 * pano_view_render: ONE launch renders n views (at most PANO_VIEW_MAX_VIEWS, of any sizes and
 *     kinds) of the chain.  View i writes image uint8 [h][w][3] and mask uint8 [h][w] (1 = the
 *     mosaic covers the pixel's direction; an uncovered pixel is 0 in both).  mosaic, views: HOST
 *     records in float64, converted to float32 by the call; everything on the device is float32,
 *     one rounding per operation.  Output pixel (u, v) gets a direction d by the view's kind:
 *       PANO_VIEW_RECTILINEAR    d = m (u, v, 1), m = R K^-1 formed by the caller
 *       PANO_VIEW_EQUIRECT       theta' = p[0] + u p[1], phi' = p[2] + v p[3],
 *                                d = m (cos phi' sin theta', sin phi', cos phi' cos theta'), m = R
 *       PANO_VIEW_STEREOGRAPHIC  X = (u - p[0]) / p[2], Y = (v - p[1]) / p[2],
 *                                d = m (4 X, 4 Y, 4 - (X X + Y Y)), m = R
 *     then, for every kind:
 *       theta = atan2(dx, dz), phi = atan2(dy, hypot(dx, dz));
 *       fx = (theta - low[0]) / res[0] brought into [0, 2 pi / res[0]) and, on a closed mosaic,
 *       multiplied by W / (2 pi / res[0]) so that its period is W; fy = (phi - low[1]) / res[1];
 *       covered: 0 <= fy <= H - 1 and, on an open mosaic, fx <= W - 1;
 *       rho = the larger length of the forward differences of (fx, fy) towards (u + 1, v) and
 *       (u, v + 1), which the thread evaluates itself (the theta difference wrapped into
 *       (-pi, pi]); lod = clamp(log2 rho, 0, n_levels - 1);
 *       the sample is trilinear: bilinear in the levels floor(lod) and floor(lod) + 1 at the level
 *       coordinate (f - (2^l - 1) / 2) / 2^l, rows clamped, columns clamped (open) or taken modulo
 *       the level's width (closed), mixed by lod - floor(lod); floor(x + 0.5) clamped to 0 .. 255.
 *     On a closed mosaic whose W is not a multiple of 2^l the seam is slightly stretched at level
 *     l (its width times 2^l is not W). */
#define PANO_VIEW_MAX_LEVELS 16
#define PANO_VIEW_MAX_VIEWS 32
#define PANO_VIEW_MAX_SIDE 32768   /* of a mosaic and of a view                    */
#define PANO_VIEW_RECTILINEAR 0
#define PANO_VIEW_EQUIRECT 1
#define PANO_VIEW_STEREOGRAPHIC 2
typedef struct pano_view {
    double m[9];               /* row-major: R K^-1 (rectilinear), else R        */
    double p[4];               /* equirect: a0, sa, b0, sb; stereographic: cx, cy, f */
    uint8_t *image;            /* dev uint8 [h][w][3]                            */
    uint8_t *mask;             /* dev uint8 [h][w]                               */
    int32_t kind, w, h, reserved;
} pano_view;
typedef struct pano_view_mosaic {
    double low[2], res[2];     /* (theta, phi) of pixel (0, 0); rad/px along x, y */
    int32_t h, w;
    int32_t closed;            /* 1 = the columns wrap (checked against w res[0]) */
    int32_t reserved;
} pano_view_mosaic;
int pano_mip_u8(pano_ctx *ctx, const uint8_t *img, int h, int w, int64_t pitch, uint8_t *mips,
                const int64_t *offsets, int n_levels);
int pano_view_render(pano_ctx *ctx, const uint8_t *mips, const int64_t *offsets, int n_levels,
                     const pano_view_mosaic *mosaic, const pano_view *views, int n);

/* Filling what no frame covers          (the reference leaves it black or cuts it away with --crop,
 * stitcher.py:340-369; csrc/fill.hip, float64 statement: tests/fill_model.py)
 * pano_fill_u8: pull-push fill of the invalid pixels of a uint8 [h][w][3] image.  img, mask
 *     (uint8 [h][w], nonzero = valid), out: dev, rows img_pitch / mask_pitch / out_pitch bytes apart;
 *     out may be img (same pitch): then only the invalid pixels are written.  closed: column w is
 *     column 0.  Sides 1 .. PANO_VIEW_MAX_SIDE.
 *     Levels: S_0 = (h, w), S_{l+1} = ((h_l + 1) / 2, (w_l + 1) / 2) down to 1 x 1 (the chain of
 *     pano_mip_u8); levels >= 1 are float32, one rounding per operation.
 *     Pull: v_0 = mask != 0, c_0 = img.  Pixel (Y, X) of level l + 1 has the children
 *     (2Y + dy, 2X + dx), dy, dx in {0, 1}, that lie inside S_l (no clamp, no wrap); it is valid if
 *     any child is, and its colour is the sum of the valid children's colours, taken in the order
 *     (0,0), (0,1), (1,0), (1,1), divided by their count (0 when there is none).
 *     Push: f_top = c_top; from the top down a valid pixel keeps f_l = c_l and an invalid pixel
 *     (y, x) takes 0.5625 f(Y, X) + 0.1875 f(Y, X') + 0.1875 f(Y', X) + 0.0625 f(Y', X') of level
 *     l + 1, added left to right, with Y = y >> 1, X = x >> 1, Y' = Y + (y & 1 ? 1 : -1) clamped to
 *     the level, X' = X + (x & 1 ? 1 : -1) clamped (open) or modulo w_{l+1} (closed).
 *     Output: valid pixels are the input's bytes, invalid ones clamp(floor(f_0 + 0.5), 0, 255); an
 *     image without a valid pixel comes back as it is.
 *     One launch per pulled level of more than PANO_FILL_TAIL_PIXELS pixels, one workgroup that
 *     takes the first level of at most that many down to 1 x 1 and back up in LDS, one launch per
 *     pushed level above it.  The levels live in a buffer of the context, which grows on demand (the
 *     call then waits for the stream first); otherwise asynchronous on the stream.  No atomics: the
 *     same input gives the same bytes.
 *     On a closed image whose width is odd at some level the modulo joins a slightly stretched
 *     seam (as pano_view_render's).  The fill works in the image plane: on an equirectangular image
 *     it is smooth near a pole, not isotropic.
 * pano_select_u8: out = mask ? a : b per pixel of two dense uint8 [n_pixels][3] images; mask uint8
 *     [n_pixels], nonzero = a.  out may be a or b.  One launch, asynchronous. */
#define PANO_FILL_TAIL_PIXELS 4096
int pano_fill_u8(pano_ctx *ctx, const uint8_t *img, int64_t img_pitch, const uint8_t *mask,
                 int64_t mask_pitch, int h, int w, int closed, uint8_t *out, int64_t out_pitch);
int pano_select_u8(pano_ctx *ctx, const uint8_t *a, const uint8_t *mask, const uint8_t *b,
                   uint8_t *out, int64_t n_pixels);

/* Lens correction at the ingest          (the reference has none: it assumes an ideal pinhole
 * camera whose principal point is the image centre; csrc/lens.hip, NumPy statement:
 * tests/lens_model.py)
 * pano_lens_undistort_u8: ONE call resamples n uint8 [h][w][3] frames (any n; of any sizes,
 *     pitches and calibrations) into the centred pinhole image of focal length f_new, each into
 *     a new frame of its size.  frames: HOST records; src, dst: dev, rows src_pitch / dst_pitch
 *     bytes apart; dst must not overlap its src.  Sides 1 .. PANO_LENS_MAX_SIDE.  For output pixel
 *     (u, v), in float64, one rounding per operation in the order written:
 *       x = (u - w / 2) / f_new, y = (v - h / 2) / f_new
 *       PANO_LENS_BROWN (k = OpenCV's k1 k2 p1 p2 k3):
 *         r2 = x x + y y, rad = 1 + r2 (k1 + r2 (k2 + r2 k3))
 *         xd = x rad + 2 p1 x y + p2 (r2 + 2 x x), yd = y rad + p1 (r2 + 2 y y) + 2 p2 x y
 *       PANO_LENS_FISHEYE (k = OpenCV's fisheye k1 .. k4; k[4] is not read):
 *         r = sqrt(x x + y y), th = atan(r), t2 = th th
 *         thd = th (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4)))), s = r > 0 ? thd / r : 1
 *         xd = x s, yd = y s
 *       px = fx xd + cx, py = fy yd + cy: the calibration's FORWARD model, nothing is iterated.
 *     px is clamped to [-2, w + 1], py to [-2, h + 1] (a position that is not a number becomes -2)
 *     and quantised to 1 / 32 pixel: sx = rint(32 px) (ties to even), ix = sx >> 5, t = (sx & 31)
 *     / 32, the same in y.  PANO_LENS_CUBIC: Catmull-Rom over the columns ix - 1 .. ix + 2 and the
 *     rows iy - 1 .. iy + 2, every index clamped to the frame, with the weights
 *       w0 = ((-0.5 t + 1) t - 0.5) t, w1 = (1.5 t - 2.5) t t + 1,
 *       w2 = ((-1.5 t + 2) t + 0.5) t, w3 = (0.5 t - 0.5) t t        (exact in float32);
 *     a row is ((p0 w0 + p1 w1) + p2 w2) + p3 w3 in float32, the four rows are combined the same
 *     way with the y weights, and the result is rint (ties to even) clamped to 0 .. 255.
 *     PANO_LENS_LINEAR: the taps ix, ix + 1 and iy, iy + 1 with the weights 1 - t, t, likewise.
 *     A refused batch (PANO_EINVAL: a null pointer, a side, a pitch below 3 w, an overlap, a
 *     parameter that is not finite, fx, fy or f_new <= 0, an unknown model or interpolation,
 *     n < 1) queues nothing.  The records travel in a buffer of the context (it grows on demand,
 *     the call then waits for the stream first); one launch per 64 frames, asynchronous on the
 *     stream.  No atomics: the same input gives the same bytes. */
#define PANO_LENS_MAX_SIDE 32767
#define PANO_LENS_BROWN 0
#define PANO_LENS_FISHEYE 1
#define PANO_LENS_CUBIC 0
#define PANO_LENS_LINEAR 1
typedef struct pano_lens_frame {
    const uint8_t *src;        /* dev uint8 [h][w][3], rows src_pitch bytes apart   */
    uint8_t *dst;              /* dev, the same size, rows dst_pitch bytes apart    */
    int64_t src_pitch, dst_pitch;
    double fx, fy, cx, cy;     /* the calibration, in pixels of this frame          */
    double f_new;              /* focal length of the corrected frame               */
    double k[5];               /* Brown: k1 k2 p1 p2 k3; fisheye: k1 k2 k3 k4, -    */
    int32_t w, h, model, interp;
} pano_lens_frame;
int pano_lens_undistort_u8(pano_ctx *ctx, const pano_lens_frame *frames, int n);

/* Photometric alignment of the frames before the stitch          (the reference has one scalar
 * gain per camera, equalize_gains; csrc/photo.hip, NumPy statement: tests/photo_model.py)
 * The model: camera i records I = g[i][c] V(rho) E in channel c, log V(rho) = a1 rho + a2 rho^2 +
 * a3 rho^3, rho = ((2x + 1 - w)^2 + (2y + 1 - h)^2) / (w^2 + h^2) at pixel position (x, y) of a
 * w x h frame: the squared distance from the image centre over the squared half diagonal.
 *
 * pano_photo_stats: the 25 weighted sums of the normal equations for each of n_pairs camera pairs,
 *     in ONE call.  frames, pairs, log_gains, alpha: HOST; sums: dev float64 [n_pairs][25].
 *     Frames are uint8 [h][w][3], rows `pitch` bytes apart, sides 2 .. PANO_PHOTO_MAX_SIDE, of any
 *     sizes.  A pair (i, j, H) maps frame i's centred pixel positions into frame j's.  For every
 *     step-th pixel (x, y) of frame i in x and y, from 0, in float64, one rounding per operation
 *     in the order written:
 *       xc = x - w_i / 2, yc = y - h_i / 2
 *       X = (H0 xc + H1 yc) + H2, Y = (H3 xc + H4 yc) + H5, Z = (H6 xc + H7 yc) + H8; Z > 0 or drop
 *       px = X / Z + w_j / 2, py = Y / Z + h_j / 2; 0 <= px <= w_j - 1 and 0 <= py <= h_j - 1 or drop
 *       sx = rint(32 px) (ties to even), ix = min(sx >> 5, w_j - 2), tx = (sx - 32 ix) / 32; y alike
 *     Frame j is sampled bilinearly in float32 at the taps ix, ix + 1 and iy, iy + 1:
 *     top = p00 (1 - tx) + p01 tx, bot alike, v_j = top (1 - ty) + bot ty (exact: dyadic weights,
 *     8-bit values); v_i is the byte of frame i.  The sample counts only when all six values lie
 *     in [lo, hi] (1 <= lo <= hi <= 255).  Then, in float64,
 *       d_c = log(v_i,c) - log(v_j,c)
 *       rho_i from (x, y), rho_j from (sx / 32, sy / 32): the squares and their sum are exact,
 *                                                         the division rounds once
 *       e1 = rho_i - rho_j, e2 = rho_i rho_i - rho_j rho_j, e3 = (rho_i rho_i) rho_i - (rho_j rho_j) rho_j
 *       r_c = (d_c - (lg[i][c] - lg[j][c])) - ((a1 e1 + a2 e2) + a3 e3), m = max_c |r_c|
 *       wt = m > tau ? tau / m : 1          (tau > 0; +infinity: every weight is 1)
 *     and the pair's sums are, at [0] wt; [1 .. 3] wt e_k; [4 .. 9] wt e_k e_l for (k, l) = 11, 12,
 *     13, 22, 23, 33; and at [10 + 5 c ..] per channel wt d_c, wt d_c e_1, wt d_c e_2, wt d_c e_3,
 *     wt d_c d_c.  No floating-point atomics: per-thread sums, a wave butterfly, per-workgroup
 *     partials (in a buffer of the context; it grows on demand, the call then waits for the stream
 *     first) and a second kernel that adds a pair's partials, all in a fixed order - two calls give
 *     the same bytes, and a pair's sums do not depend on what else is in the batch.  A pair
 *     without a sample gets 25 zeros.  PANO_EINVAL, with nothing launched: a null pointer,
 *     n_frames < 1, n_pairs < 0, a side, a pitch below 3 w, step < 1 or > PANO_PHOTO_MAX_SIDE, lo < 1, hi > 255, lo > hi, a
 *     pair index out of range, i == j, an H, log-gain or alpha that is not finite, tau that is not
 *     a number or <= 0.  n_pairs == 0 launches nothing.  Asynchronous on the stream.
 * pano_photo_apply_u8: ONE call corrects n uint8 [h][w][3] frames (any n, any sizes 1 ..
 *     PANO_PHOTO_MAX_SIDE) by their tables.  frames: HOST records; src, dst, table: dev; table is
 *     float32 [3][PANO_PHOTO_TABLE], T[c][k] the factor of channel c at rho = k / 1024.  Per pixel
 *       d2 = (2x + 1 - w)^2 + (2y + 1 - h)^2 (64-bit integers), s = (double)d2 / (double)(w^2 + h^2)
 *       * 1024.0, k = (int)s, t = (float)(s - k), f = T[c][k] + t (T[c][k + 1] - T[c][k]) in float32
 *       without a fused multiply-add, out = rint(min(v f, 255)) (ties to even).
 *     dst == src with equal pitches is allowed (the correction is pointwise); any other overlap of
 *     a frame's dst with its src is refused, as are a null pointer, a side, a pitch below 3 w and
 *     n < 1 (PANO_EINVAL, nothing launched).  The records travel in a buffer of the context; one
 *     launch per 64 frames, asynchronous on the stream. */
#define PANO_PHOTO_MAX_SIDE 32767
#define PANO_PHOTO_SUMS 25
#define PANO_PHOTO_TABLE 1026
typedef struct pano_photo_frame {
    const uint8_t *img;        /* dev uint8 [h][w][3], rows pitch bytes apart       */
    int64_t pitch;
    int32_t w, h;
} pano_photo_frame;
typedef struct pano_photo_pair {
    double H[9];               /* centred pixels of frame i -> centred pixels of j  */
    int32_t i, j;
} pano_photo_pair;
typedef struct pano_photo_apply {
    const uint8_t *src;        /* dev uint8 [h][w][3], rows src_pitch bytes apart   */
    uint8_t *dst;              /* dev, the same size; may be src itself             */
    const float *table;        /* dev float32 [3][PANO_PHOTO_TABLE]                 */
    int64_t src_pitch, dst_pitch;
    int32_t w, h;
} pano_photo_apply;
int pano_photo_stats(pano_ctx *ctx, const pano_photo_frame *frames, int n_frames,
                     const pano_photo_pair *pairs, int n_pairs, int step, int lo, int hi,
                     const double *log_gains, const double *alpha, double tau, double *sums);
int pano_photo_apply_u8(pano_ctx *ctx, const pano_photo_apply *frames, int n);

/* Exposure fusion of bracketed frames at the ingest          (the reference takes one image per
 * position; Mertens, Kautz, Van Reeth 2007, OpenCV's MergeMertens; csrc/fuse.hip, NumPy statement:
 * tests/fuse_model.py)
 * A stack is k exposures (2 .. PANO_FUSE_MAX_EXPOSURES) of one view: uint8 [h][w][3] BGR frames of
 * one size, sides 1 .. PANO_FUSE_MAX_SIDE, rows `pitch` bytes apart; one fused uint8 [h][w][3]
 * frame comes out.  Everything is float32, one rounding per operation in the order written (no
 * fused multiply-add), pyrDown / pyrUp are cv2's as oracle/cv2_shim.py restates them.
 *   A, raw weights, per exposure and pixel:
 *       B, G, R = (float)byte / 255.0f
 *       g = (0.114f B + 0.587f G) + 0.299f R
 *       lap = ((g[y][x-1] + g[y][x+1]) + (g[y-1][x] + g[y+1][x])) - 4 g, indices reflected as
 *             BORDER_REFLECT_101 (on a side of length 1 the neighbour is the pixel itself)
 *       C = |lap|
 *       m = ((B + G) + R) / 3, S = sqrtf((((B-m)^2 + (G-m)^2) + (R-m)^2) / 3)
 *       E = expf(-((((B-.5f)^2 + (G-.5f)^2) + (R-.5f)^2) / 0.08f))       (sigma = 0.2, one exponential)
 *       W = ((C^contrast S^saturation) E^exposure) + 1e-12f: an exponent of exactly 1 multiplies
 *           the factor as it is, of exactly 0 leaves it out, anything else is powf.  (1, 1, 1) is
 *           the paper's choice; OpenCV's default is (1, 1, 0).
 *   B, normalise and pack: T = ((W_0 + W_1) + ...) + W_k-1, N_i = W_i / T, the packed pixel of
 *       exposure i is the float4 (B, G, R, N_i).
 *   C, pyramids: L = max(0, bit_length(min(h, w)) - 2) levels below the frame, so that the coarsest
 *       level is at least 2 x 2 (where pyrUp is defined; one level fewer than OpenCV's
 *       int(log2(min side))); params->n_levels in 0 .. L overrides it, -1 is the default.
 *       P_i,0 = the packed image, P_i,l+1 = pyrDown(P_i,l) on all four channels.
 *   D, fused levels: for l < L, R_l = sum_i N_i,l (P_i,l[BGR] - pyrUp(P_i,l+1[BGR])[:h_l, :w_l]);
 *       R_L = sum_i N_i,L P_i,L[BGR]; N_i,l is channel 3 of P_i,l; a sum starts from the i = 0
 *       product and adds the others in order of i.  The Laplacian pyramids are never stored.
 *   E, collapse and quantise: from l = L - 1 down to 0, R_l = R_l + pyrUp(R_l+1)[:h_l, :w_l];
 *       out = rint(min(max(R_0 255, 0), 255)), ties to even.
 * pano_fuse_work_bytes(h, w, k): the workspace of one stack, callable without a GPU: with h_0 = h,
 *     w_0 = w, h_l+1 = (h_l + 1) / 2 (w alike) and a256 rounding up to a multiple of 256,
 *       sum over l = 0 .. L of a256(16 k h_l w_l) + a256(16 h_l w_l)
 *     (the k packed images and the fused level, float4 per pixel).  0 for a side or k out of range.
 * pano_fuse_u8: ONE call fuses n stacks of mixed sizes and k, one after another on the context's
 *     stream through the one workspace `work` (dev, work_bytes long, at least pano_fuse_work_bytes
 *     of the call's largest stack).  stacks: HOST records; src, dst, raw, fused: dev.  raw
 *     (float32 [k][h][w], stage A's W) and fused (float32 [h][w][3], stage E's R_0 before it is
 *     quantised) are optional outputs of the kernels that feed the next stage; NULL: not written.
 *     3 L + 2 launches per stack (3 when L = 0), asynchronous, no host wait, no atomics: two calls
 *     give the same bytes, and a stack's result does not depend on what else is in the call.
 *     PANO_EINVAL, with nothing launched: a null pointer, n < 1, k outside 2 .. 8, a side outside
 *     1 .. 32767, a pitch below 3 w, n_levels outside -1 .. L of any stack, an exponent that is
 *     negative or not finite, work_bytes too small, a dst that overlaps a source frame of its
 *     stack or the workspace. */
#define PANO_FUSE_MAX_EXPOSURES 8
#define PANO_FUSE_MAX_SIDE 32767
typedef struct pano_fuse_stack {
    const uint8_t *src[PANO_FUSE_MAX_EXPOSURES];   /* dev uint8 [h][w][3]; the first k are read   */
    int64_t src_pitch[PANO_FUSE_MAX_EXPOSURES];    /* bytes between their rows                    */
    uint8_t *dst;              /* dev uint8 [h][w][3], rows dst_pitch bytes apart   */
    int64_t dst_pitch;
    float *raw;                /* dev float32 [k][h][w] or NULL                     */
    float *fused;              /* dev float32 [h][w][3] or NULL                     */
    int32_t w, h, k, reserved;
} pano_fuse_stack;
typedef struct pano_fuse_params {
    float contrast, saturation, exposure;          /* the exponents, finite and >= 0              */
    int32_t n_levels;          /* -1: the default L of each stack                   */
} pano_fuse_params;
size_t pano_fuse_work_bytes(int h, int w, int k);
int pano_fuse_u8(pano_ctx *ctx, const pano_fuse_stack *stacks, int n, const pano_fuse_params *params,
                 void *work, int64_t work_bytes);

/* Alignment of hand-held exposure brackets before they are fused   (the reference takes one image
 * per position; G. Ward 2003, median threshold bitmaps, OpenCV's AlignMTB; csrc/align.hip, NumPy
 * statement: tests/align_model.py)
 * A stack is k exposures (2 .. PANO_FUSE_MAX_EXPOSURES) of one view: uint8 [h][w][3] BGR frames of
 * one size, sides 1 .. PANO_FUSE_MAX_SIDE, rows `pitch` bytes apart; `reference` (0 .. k - 1) is the
 * exposure the others are moved onto.  Integers throughout; params: max_bits 0 .. 7 (the usual 6),
 * exclude 0 .. 127 (the usual 4).
 *   A, grey: g = (29 B + 150 G + 77 R + 128) >> 8, uint8.
 *   B, pyramid: L = min(max_bits, max(0, bit_length(min(h, w)) - 5)) levels above the frame: the
 *       coarsest keeps a short side of at least 16.  Level l + 1 is h_l / 2 by w_l / 2 (rounded
 *       down: h_l = h >> l), each pixel (a + b + c + d + 2) >> 2 of its 2 x 2 block of level l; an
 *       odd last row or column is dropped.  The levels nest: a 128 x 128-aligned tile of level 0
 *       determines its part of every level up to 7.
 *   C, median, per frame and level: m = the smallest v with #{g <= v} >= (N + 1) / 2, N = h_l w_l.
 *   D, bitmaps, per frame and level: tb = g > m, eb = |g - m| > exclude, both packed 32 pixels a
 *       uint32 along the row, wpr_l = ceil(w_l / 32) words per row: bit x & 31 of word x >> 5 is
 *       pixel x; the bits from w_l on are 0.
 *   E, search, for every frame i other than the reference r: s = (0, 0) at level L; going down a
 *       level s <- 2 s.  At each level the nine candidates c = s + d are counted, numbered
 *       d = (0, 0) first, then dy = -1, 0, 1 outer and dx = -1, 0, 1 inner without (0, 0):
 *       err(c) = the number of pixels (x, y) of the reference with (x - c.x, y - c.y) inside frame
 *       i and (tb_r[y][x] ^ tb_i[y - c.y][x - c.x]) & eb_r[y][x] & eb_i[y - c.y][x - c.x] set.
 *       s <- the first candidate with the smallest err (strict <: identical or featureless frames
 *       give (0, 0)).  The result (dx, dy) = s of level 0, |dx|, |dy| <= 2^(L+1) - 1, means
 *       aligned[y][x] = src[y - dy][x - dx]; the reference's is (0, 0).
 *   F, apply: aligned[y][x] = src[clamp(y - dy, 0, h - 1)][clamp(x - dx, 0, w - 1)], all three
 *       bytes, for the frames that have a dst and a shift other than (0, 0).  The reference and
 *       frames with a zero shift are NOT copied: their dst is left as it was, the caller takes
 *       their src.  (The shifts stay on the device: the call waits for nothing, and the tiles of
 *       an unmoved frame leave at once.)
 * pano_align_work_bytes(h, w, k): the workspace of one stack, callable without a GPU: with
 *     Lm = min(7, max(0, bit_length(min(h, w)) - 5)), h_l = h >> l, w_l = w >> l, p_l = w_l rounded
 *     up to a multiple of 4, wpr_l as above and a256 rounding up to a multiple of 256,
 *       a256(1024 k (Lm + 1)) + a256(36 k (Lm + 1)) + a256(4 k (Lm + 1))
 *       + k * sum over l = 0 .. Lm of (a256(h_l p_l) + a256(8 h_l wpr_l))
 *     (histograms, error counts, medians; per frame the grey levels and the two bitmaps of every
 *     level).  0 for a side or k out of range.
 * pano_align_mtb: ONE call aligns n stacks of mixed sizes and k: one table of tiles over all their
 *     frames, 6 + L_max launches for up to 256 frames, queued on the context's stream, no host wait.
 *     `work` (dev, work_bytes long) holds ALL stacks of the call at once: at least the sum of their
 *     pano_align_work_bytes; it need not be cleared.  stacks: HOST records; src, dst, shifts and
 *     the stage outputs: dev.  shifts: int32 [k][2] = (dx, dy) per exposure, always written.
 *     dst[e] NULL: exposure e is not applied (shifts only).  Stage outputs, NULL in production,
 *     dense, frame after frame and within a frame level 0 .. L: grey uint8 [h_l][w_l]; medians
 *     int32 [k][L + 1]; bitmaps uint32, per level tb [h_l][wpr_l] then eb [h_l][wpr_l]; errs uint32
 *     [k][L + 1][9] (the reference's are 0).  The counts are integer sums: two calls give the same
 *     bytes, and a stack's result does not depend on what else is in the call.
 *     PANO_EINVAL, with nothing launched or written: a null pointer (stacks, params, work, a src,
 *     shifts), n < 1, k outside 2 .. 8, a side outside 1 .. 32767, reference outside 0 .. k - 1,
 *     max_bits outside 0 .. 7, exclude outside 0 .. 127, a pitch below 3 w, work_bytes too small,
 *     a dst that overlaps a source frame of its stack or the workspace. */
typedef struct pano_align_stack {
    const uint8_t *src[PANO_FUSE_MAX_EXPOSURES];   /* dev uint8 [h][w][3]; the first k are read   */
    int64_t src_pitch[PANO_FUSE_MAX_EXPOSURES];    /* bytes between their rows                    */
    uint8_t *dst[PANO_FUSE_MAX_EXPOSURES];         /* dev uint8 [h][w][3] per exposure, or NULL   */
    int64_t dst_pitch[PANO_FUSE_MAX_EXPOSURES];
    int32_t *shifts;           /* dev int32 [k][2]: (dx, dy)                        */
    uint8_t *grey;             /* stage outputs, dev or NULL                        */
    int32_t *medians;
    uint32_t *bitmaps;
    uint32_t *errs;
    int32_t w, h, k, reference;
} pano_align_stack;
typedef struct pano_align_params {
    int32_t max_bits;          /* 0 .. 7: at most this many levels above the frame  */
    int32_t exclude;           /* 0 .. 127: pixels this close to the median are ignored */
} pano_align_params;
size_t pano_align_work_bytes(int h, int w, int k);
int pano_align_mtb(pano_ctx *ctx, const pano_align_stack *stacks, int n, const pano_align_params *params,
                   void *work, int64_t work_bytes);

/* Deghosting of exposure brackets before they are fused      (the reference takes one image per
 * position; reference-guided and rank based; csrc/deghost.hip, NumPy statement:
 * tests/deghost_model.py)
 * Two exposures of a static scene differ by a monotone map of brightness, so a pixel's RANK within
 * its own frame's histogram is nearly the same in both.  A pixel of exposure i whose rank disagrees
 * with the reference exposure's shows other scene content; it is replaced by the reference's pixel,
 * carried to exposure i's brightness through the histogram-matching map of the two frames.  A
 * clipped pixel sits in a huge bin: its rank is an interval that agrees with anything in it.
 * A stack is as for pano_align_mtb: k exposures (2 .. PANO_FUSE_MAX_EXPOSURES), uint8 [h][w][3] BGR
 * of one size, sides 1 .. PANO_FUSE_MAX_SIDE, rows `pitch` bytes apart; `reference` 0 .. k - 1;
 * N = h w.  Integers throughout; params: slack 0 .. 15 (the usual 3) grey levels of noise tolerated,
 * tol 0 .. 255 (8) rank units of 1/255 tolerated, erode 0 .. 3 (1), dilate 0 .. 15 (3).
 *   A, histograms: g = (29 B + 150 G + 77 R + 128) >> 8 (pano_align_mtb's grey); per frame uint32
 *       hist[4][256] of g, B, G, R.
 *   B, tables, per frame: below[v] = #{. < v}, v = 0 .. 256.  The rank interval of grey v:
 *       lo[v] = below_g[max(v - slack, 0)] 255 / N, hi[v] = below_g[min(v + slack + 1, 256)] 255 / N,
 *       64-bit products, floor division, both uint8.  The colour map onto frame i from the
 *       reference r, per channel c: target = below_r,c[v] + (hist_r,c[v] + 1) / 2; map_i,c[v] = the
 *       smallest u with below_i,c[u + 1] >= target (it exists: target <= N).  map_r is the identity.
 *   C, raw mask, per frame i != r and pixel: set where lo_i[g_i] > hi_r[g_r] + tol or
 *       lo_r[g_r] > hi_i[g_i] + tol.  Packed as pano_align_mtb's bitmaps: bit x & 31 of word x >> 5,
 *       wpr = ceil(w / 32) words per row, the bits from w on 0.
 *   D, clean-up: eroded by a (2 erode + 1)^2 square, pixels outside the image counting as set, then
 *       dilated by a (2 dilate + 1)^2 square, pixels outside counting as clear; the bits from w on
 *       are 0.  count[i] = the set bits; count[r] = 0.
 *   E, apply, for every frame i != r with a dst and count[i] > 0:
 *       dst[y][x][c] = mask ? map_i,c[ref[y][x][c]] : src[y][x][c].  The reference and frames with
 *       a count of 0 are NOT copied: their dst is left as it was, the caller takes their src.  (The
 *       counts stay on the device: the call waits for nothing, the tiles of such a frame leave.)
 * pano_deghost_work_bytes(h, w, k): the workspace of one stack, callable without a GPU: with
 *     p = w rounded up to a multiple of 4, wpr as above and a256 rounding up to a multiple of 256,
 *       a256(4096 k) + a256(512 k) + a256(768 k) + k (a256(h p) + 2 a256(4 h wpr))
 *     (histograms, rank tables, colour maps; per frame the grey image, the raw and the final
 *     mask).  0 for a side or k out of range.
 * pano_deghost_u8: ONE call takes n stacks of mixed sizes and k: one table of tiles over all their
 *     frames, 5 launches for up to 256 frames (more: further passes of whole stacks), queued on the
 *     context's stream, no host wait, no allocation.  `work` (dev, work_bytes long) holds ALL stacks
 *     of the call: at least the sum of their pano_deghost_work_bytes; it need not be cleared.
 *     stacks: HOST records; src, dst, counts and the stage outputs: dev.  counts: int32 [k], always
 *     written.  dst[e] NULL: exposure e is not applied.  Stage outputs, NULL in production: hists
 *     uint32 [k][4][256]; ranks uint8 [k][2][256] (lo, hi); maps uint8 [k][3][256]; raw and mask
 *     uint32 [k][h][wpr] (the reference's are 0).  The counts are integer sums: two calls give the
 *     same bytes, and a stack's result does not depend on what else is in the call.
 *     PANO_EINVAL, with nothing launched or written: a null pointer (stacks, params, work, a src,
 *     counts), n < 1, k outside 2 .. 8, a side outside 1 .. 32767, reference outside 0 .. k - 1,
 *     slack outside 0 .. 15, tol outside 0 .. 255, erode outside 0 .. 3, dilate outside 0 .. 15, a
 *     pitch below 3 w, work_bytes too small, a dst that overlaps a source frame of its stack or the
 *     workspace. */
typedef struct pano_deghost_stack {
    const uint8_t *src[PANO_FUSE_MAX_EXPOSURES];   /* dev uint8 [h][w][3]; the first k are read   */
    int64_t src_pitch[PANO_FUSE_MAX_EXPOSURES];    /* bytes between their rows                    */
    uint8_t *dst[PANO_FUSE_MAX_EXPOSURES];         /* dev uint8 [h][w][3] per exposure, or NULL   */
    int64_t dst_pitch[PANO_FUSE_MAX_EXPOSURES];
    int32_t *counts;           /* dev int32 [k]: replaced pixels per exposure       */
    uint32_t *hists;           /* stage outputs, dev or NULL                        */
    uint8_t *ranks;
    uint8_t *maps;
    uint32_t *raw;
    uint32_t *mask;
    int32_t w, h, k, reference;
} pano_deghost_stack;
typedef struct pano_deghost_params {
    int32_t slack;             /* 0 .. 15: grey levels of noise tolerated           */
    int32_t tol;               /* 0 .. 255: rank units of 1/255 tolerated           */
    int32_t erode;             /* 0 .. 3: the radius of the erosion                 */
    int32_t dilate;            /* 0 .. 15: the radius of the dilation               */
} pano_deghost_params;
size_t pano_deghost_work_bytes(int h, int w, int k);
int pano_deghost_u8(pano_ctx *ctx, const pano_deghost_stack *stacks, int n, const pano_deghost_params *params,
                    void *work, int64_t work_bytes);

/* Local alignment of the warped patches between the warp and the blend (--local-align; DESIGN.md
 * section 5u; tests/flow_model.py restates all of this in NumPy).  Two overlapping frames that
 * disagree by a small, smooth, locally varying displacement (parallax of a hand-held sweep) are
 * each moved part of the way towards the other, in proportion to the other's blend weight.
 * Everything up to the block vectors is integer arithmetic; the two float32 stages do one
 * rounding per operation in the order stated (-ffp-contract=off): the same input, the same bytes.
 *
 * Input: n stage-level patches (planes [4][h][vpitch] float32 over the whole patch, mask uint8
 *     [h][w] with 1 = invalid, the rect in the H x W mosaic), levels 0 .. PANO_FLOW_MAX_LEVELS
 *     (reach 2^(levels + 1) - 1 pixels), gain 1 .. PANO_FLOW_MAX_GAIN in 1/16 grey levels per
 *     sample, min_overlap >= 16.
 * Grey and validity, per camera: q_k = uint8(float32(255) * c_k) per colour plane,
 *     g = (q_0 + 2 q_1 + q_2 + 2) >> 2; valid where the mask is 0, invalid outside the rect; an
 *     invalid pixel has g = 0.
 * Levels 1 .. L are anchored at the MOSAIC's origin: sample (Y, X) of level l covers the mosaic
 *     pixels [Y 2^l, (Y + 1) 2^l) of each axis, is (a + b + c + d + 2) >> 2 of its four children
 *     and valid only if all four are.
 * Pairs (host): every i < j whose rects meet in at least min_overlap x min_overlap pixels, oh x
 *     ow; L_ij = min(levels, max(0, bit_length(min(oh, ow)) - 6)).
 * Blocks: block (by, bx) of level l is the 16 x 16 samples of level l from (16 by, 16 bx); a
 *     pair's blocks at a level are those that meet its intersection.
 * Search, l = L_ij .. 0: a block inherits v = 2 * the vector of block (by >> 1, bx >> 1) of level
 *     l + 1, (0, 0) at the top.  Candidates u = v + (dx, dy): (0, 0) first, then dy, dx = -1 .. 1
 *     in raster order.  n(u) counts the block's samples s with i valid at s and j valid at s + u,
 *     S(u) sums |g_i(s) - g_j(s + u)| over them; u is eligible when n(u) >= PANO_FLOW_MIN_COUNT.
 *     The winner w is the first eligible candidate that minimises S / n, compared exactly:
 *     S(u) n(w) < S(w) n(u) in int64.  If the centre c is eligible it stays unless
 *     16 S(w) n(c) + gain n(w) n(c) <= 16 S(c) n(w).  With no eligible candidate the block keeps v
 *     and is unknown.  Result: int16 (dx, dy, known, 0) per block, g_i(s) ~ g_j(s + F_ij).
 * Smoothing, per pair on its level-0 blocks: each component becomes the lower median (element
 *     (m - 1) >> 1 of the m sorted values) of the known vectors of the block's 3 x 3 neighbourhood
 *     inside the pair's block range; an unknown block takes it when m >= 3 and is (0, 0) otherwise.
 * Field per pixel: the smoothed vectors as float32, bilinear between the block centres 16 b + 7.5:
 *     t = float32(2 x - 15) / 32, b0 = floor(t), f = t - b0, the indices b0 and b0 + 1 clamped into
 *     the pair's block range; x first, then y; every lerp is a + f * (b - a).  F_ji = -F_ij.
 * Apply, per camera c and pixel p of its patch: a masked pixel is copied.  W = the float32 sum, in
 *     camera order, of alpha_k(p) over every camera k that covers p (inside its rect, mask 0; c is
 *     one).  d = sum over c's pair partners j that cover p with alpha_j(p) > 0, in camera order,
 *     of (alpha_j(p) / W) * F_cj(p), one division and one product per component, from d = 0.  If
 *     d == (0, 0) the pixel is copied; else the four planes are sampled bilinearly (same lerps) at
 *     patch position (x - d_x, y - d_y): x0 = floor, fx = sx - x0, taps x0, x0 + 1, likewise in y;
 *     if a tap is outside the patch or masked the pixel is copied.  The mask never changes.
 *
 * patches_host: a HOST array of the n records; their pointers are device pointers.
 * pano_flow_work_bytes: the workspace (dev) of a call, 0 for arguments a call would refuse.  It
 *     holds, each from a multiple of 256 bytes: the pyramids (uint16 g | valid << 8; per camera
 *     that has a pair, in order, the levels 0 .. max L_ij of its box - the rect grown to multiples
 *     of 16 mosaic pixels - dense, back to back), the block vectors (int16 [4]; per pair the
 *     levels 0 .. L_ij, [nby][nbx] each), the smoothed vectors (int16 [2]; per pair [nby][nbx] of
 *     level 0) and int32 statistics (pixels moved, unmasked pixels of the cameras with a pair).
 * pano_flow_pyramid / _search / _smooth / _apply: one stage each, reading what the stage before
 *     left in (or a test wrote into) the workspace.  out: HOST array of n device pointers, planes
 *     [4][h][vpitch] of their own for every camera that has a pair (the others are not read; the
 *     columns from w on are not written); stats (dev int32 [4] or NULL).
 * pano_flow_align: the whole stage, 3 + (max L_ij + 1) launches from one record table, no host
 *     wait; pyramid, vectors, fields, stats: dev or NULL, the workspace's regions copied out
 *     behind the kernels.  With no pair nothing is launched.
 * PANO_EINVAL with nothing written: a null table or workspace, n < 2, levels, gain or min_overlap
 *     out of range, a rect that leaves the mosaic, a patch whose window is not the whole patch or
 *     without a mask, work_bytes too small, a camera with a pair and no output planes of its own. */
#define PANO_FLOW_MAX_LEVELS 4
#define PANO_FLOW_MIN_COUNT 128
#define PANO_FLOW_MAX_GAIN 4080
typedef struct pano_flow_params {
    int32_t levels;            /* 0 .. 4; default 3: a reach of 15 pixels            */
    int32_t gain;              /* 1/16 grey levels per sample a move must gain; 16   */
    int32_t min_overlap;       /* side of the smallest intersection that is a pair; 64 */
    int32_t reserved;
} pano_flow_params;
size_t pano_flow_work_bytes(const pano_patch *patches_host, int n, int H, int W,
                            const pano_flow_params *params);
int pano_flow_pyramid(pano_ctx *ctx, const pano_patch *patches_host, int n, int H, int W,
                      const pano_flow_params *params, void *work, int64_t work_bytes);
int pano_flow_search(pano_ctx *ctx, const pano_patch *patches_host, int n, int H, int W,
                     const pano_flow_params *params, void *work, int64_t work_bytes);
int pano_flow_smooth(pano_ctx *ctx, const pano_patch *patches_host, int n, int H, int W,
                     const pano_flow_params *params, void *work, int64_t work_bytes);
int pano_flow_apply(pano_ctx *ctx, const pano_patch *patches_host, int n, int H, int W,
                    const pano_flow_params *params, void *work, int64_t work_bytes,
                    float *const *out, int32_t *stats);
int pano_flow_align(pano_ctx *ctx, const pano_patch *patches_host, int n, int H, int W,
                    const pano_flow_params *params, void *work, int64_t work_bytes,
                    float *const *out, uint16_t *pyramid, int16_t *vectors, int16_t *fields,
                    int32_t *stats);

/* One multiband stitch of the mosaic columns [xs0, xs1), queued by ONE call
 *                                                  stitcher.py:283-327 (equalize and crop aside)
 * = pano_ownership_cameras, pano_owned_regions (+ its copy to the host), pano_interior_map,
 * the one wait of a stitch, pano_layout_windows / pano_layout_place, the upload of the record
 * table, [pano_blur_tiles,] pano_warp_windows, pano_multiband_blur, pano_multiband_compose in
 * that order on the context's stream: the launch sequence of a stitch without a round trip
 * through the caller's language per launch (a dozen ctypes calls cost 0.3 ms per stitch,
 * as much as one GPU's share of the kernels when eight GPUs split a 4K panorama).
 * The caller owns every buffer; `args` says where they are and how large:
 *   cams               dev [n] records (frames NULL where not resident, see have)
 *   rects, have        host int32 [n][4] = (y0, y1, x0, x1) / host uint8 [n] (or NULL)
 *   [own0, own1)       columns to evaluate ownership on: the strip grown by what the interior
 *                      test and the windows look at (the whole mosaic: 0, W)
 *   taps, ntaps        host tap tables of the n_levels - 1 Gaussians (layout: pano_multiband_blur)
 *   shortcut           1 = interior map on (pano_interior_map, the compose's interior pixels)
 *   warp_need          1 = warp only the blocks anything reads (pano_blur_tiles), 0 = all of V,
 *                      -1 = decide by the mean width of the rectangles A (>= 768 columns)
 *   owner, valid       dev int16 / uint8 [H][W]: results
 *   marks, regions     dev workspaces of pano_owned_regions; regions_host: PINNED host copy
 *   block_owner, interior   dev workspaces of pano_interior_map
 *   records_host       PINNED host pano_patch [cap_records], cap_records >= n * max_spans
 *   table              dev pano_patch [cap_records]
 *   planes, blurred, scratch (+ their sizes in floats), tile_flags, need (cap_tiles bytes each)
 *   mosaic (+ optional mosaic_f32)   dev [H][W][3]: only columns [xs0, xs1) are written
 * Returns PANO_OK; PANO_EGROW (positive, not an error) when an arena or the tile arrays are too
 * small for this stitch: args->layout then says what is needed, everything up to the wait has
 * been queued, and the call is repeated with resume = 1 after the caller has grown them; or a
 * negative error (args->layout.missing > 0: a needed frame is not resident). */
#define PANO_EGROW 1
/* pano_stitch_args.trust_layout (described at the field) - in: */
#define PANO_TRUST_NONE 0
#define PANO_TRUST_LAYOUT 1
#define PANO_TRUST_GEOMETRY 3
/* ... and out (or PANO_TRUST_NONE: the stitch took a waiting path): */
#define PANO_TRUST_TRUSTED 2
#define PANO_TRUST_KEPT 4
typedef struct pano_stitch_args {
    const pano_camera *cams;
    const int32_t *rects;
    const uint8_t *have;
    const double *sin_t, *cos_t, *tan_p;
    const float *lut;
    const float *taps;
    const int32_t *ntaps;
    int16_t *owner;
    uint8_t *valid;
    uint8_t *marks;
    int32_t *regions;
    int32_t *regions_host;
    int16_t *block_owner;
    uint8_t *interior;
    pano_patch *records_host;
    pano_patch *table;
    float *planes, *blurred, *scratch;
    uint8_t *tile_flags, *need;
    uint8_t *mosaic;
    float *mosaic_f32;
    int64_t planes_floats, blurred_floats, scratch_floats;
    int32_t n, H, W, xs0, xs1, own0, own1;
    int32_t lut_stride, n_levels, radius, shortcut, warp_need, max_spans, min_gap;
    int32_t cap_records, cap_tiles;
    int32_t used_need;         /* out: 1 = the warp ran on the need flags */
    int32_t trust_layout;      /* PANO_TRUST_* above.
                                * in: 1 = the caller vouches that cameras (matrices, rectangles),
                                * strip and resident frames are those of this context's previous
                                * stitch (with PANO_OPT_STITCH_ASYNC on): the stitch is queued with
                                * that stitch's verified layout and NOBODY WAITS - the call returns
                                * when everything is queued.  out: 2 = it did, 0 = it took the
                                * waiting path (first stitch of a shape, option off, ...).  Every
                                * kernel still runs; what is trusted is only that the same cameras
                                * give the same layout, which pano_stitch_verify checks.
                                * in: 3 = the same promise, and the geometry may be KEPT: the owner
                                * map, valid mask, interior map, record table, tile flags and the
                                * context's work list are functions of exactly what the caller
                                * vouches for; when the buffers are the previous stitch's (owner,
                                * valid, table, interior, tile_flags, need, the arenas, sin_t - same
                                * pointers) and no other call has entered the context since, only
                                * the warp, the blur and the collapse are queued: out 4.  Otherwise
                                * as 1.  The reference recomputes all of it per stitch
                                * (stitcher.py:276-306, 196-204) - to the same values. */
    uint8_t *classes;          /* dev workspace of pano_interior_classes (the interior map's shape),
                                * or NULL: no level classes */
    pano_layout layout;        /* out */
} pano_stitch_args;
int pano_stitch_multiband(pano_ctx *ctx, pano_stitch_args *args, int resume);
/* Compares the layout summary of the last trusted stitch with the verified layout it was queued
 * with (waits for that stitch's layout kernel); PANO_EINVAL when they differ - the promise of
 * args->trust_layout did not hold and the trusted mosaics since the last check are void.  A no-op
 * without trusted stitches pending; the next untrusted pano_stitch_multiband calls it itself. */
int pano_stitch_verify(pano_ctx *ctx);
/* How many stitches of this context went through on the device-side layout
 * (PANO_OPT_STITCH_ASYNC) and how many of those attempts fell back to the host layout. */
int pano_stitch_counts(const pano_ctx *ctx, int *device_layouts, int *fallbacks);

#ifdef __cplusplus
}
#endif
#endif /* PANO360_H */
