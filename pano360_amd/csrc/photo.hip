// Photometric alignment of the frames before the stitch (pano_photo_stats, pano_photo_apply_u8):
// per-camera, per-channel gains and one radial falloff log V(rho) = a1 rho + a2 rho^2 + a3 rho^3,
// fitted by least squares in the log domain over every overlap of the rig.  The statistics kernel
// gathers, for a table of camera pairs, the 25 weighted sums the normal equations need; the host
// (pano360_amd/photo.py) solves them in float64 and the streaming kernel applies the correction.
// The contract is in include/pano360.h, a NumPy statement of the arithmetic is
// tests/photo_model.py.  No atomics: sums are taken per thread, per wave and per workgroup in a
// fixed order and a second kernel adds a pair's partials in a fixed order.
#include <math.h>

#include "batch.h"
#include "geom.h"
#include "wave.h"

#define PH_TW 64                    // lattice points across a statistics tile
#define PH_TH 16                    // lattice rows of a tile: four per thread
#define PH_CHUNK 256                // pairs of one statistics launch
#define PH_NS PANO_PHOTO_SUMS

struct PhotoPairDev {               // a pair of a launch, in device memory
    double H[9];
    double dlg[3];                  // lg[i][c] - lg[j][c]
    const uint8_t *fi, *fj;
    int64_t pitch_i, pitch_j;
    int64_t part0;                  // the pair's first partial in the buffer
    int wi, hi, wj, hj;
    TileSlot slot;
    int nblk, reserved;
};

// rho of a position whose doubled, centred coordinates are (a, b): the squares and their sum are
// exact in float64 (|a|, |b| < 2^16 with at most four fraction bits), the division rounds once
__device__ __forceinline__ double photo_rho(double a, double b, double den) {
    return (a * a + b * b) / den;
}

// One workgroup per 64 x 16 tile of one pair's lattice (every step-th pixel of frame i), a thread
// takes four lattice rows of a column.  The pair comes from the table's prefix of workgroup
// counts (batch.h).
__global__ __launch_bounds__(256) void photo_stats_kernel(
    const PhotoPairDev *__restrict__ table, int n, int step, int lo_v, int hi_v, double a1,
    double a2, double a3, double tau, double *__restrict__ partials) {
    __shared__ double s_log[256];
    __shared__ double s_red[4][PH_NS];
    __shared__ int s_skip;
    const int tid = threadIdx.x;
    int tile;
    const PhotoPairDev &P = batch_record(table, n, tile);
    const int wi = P.wi, hgt_i = P.hi, wj = P.wj, hj = P.hj;
    const int lw = (wi + step - 1) / step, lh = (hgt_i + step - 1) / step;
    const int tx0 = (tile % P.slot.tiles_x) * PH_TW, ty0 = (tile / P.slot.tiles_x) * PH_TH;
    double *out = partials + (P.part0 + tile) * PH_NS;
    double H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = P.H[k];
    const double cxi = (double)wi / 2.0, cyi = (double)hgt_i / 2.0;
    const double cxj = (double)wj / 2.0, cyj = (double)hj / 2.0;

    s_log[tid] = log((double)tid);                      // (entry 0 is never read: lo_v >= 1)
    if (tid == 0) {
        // Where the denominator is positive on the tile's corners it is on the tile, which then
        // maps into the convex hull of its mapped corners: when that hull (a pixel of slack)
        // misses frame j, or the denominator is nowhere positive, no sample of the tile counts.
        const int xe = (min(tx0 + PH_TW, lw) - 1) * step, ye = (min(ty0 + PH_TH, lh) - 1) * step;
        const int cx[4] = {tx0 * step, xe, tx0 * step, xe}, cy[4] = {ty0 * step, ty0 * step, ye, ye};
        double lo_x = 1e300, hi_x = -1e300, lo_y = 1e300, hi_y = -1e300;
        int pos = 0;
        for (int k = 0; k < 4; ++k) {
            const double xc = (double)cx[k] - cxi, yc = (double)cy[k] - cyi;
            const double Z = (H[6] * xc + H[7] * yc) + H[8];
            pos += Z > 0.0;
            const double u = ((H[0] * xc + H[1] * yc) + H[2]) / Z + cxj;
            const double v = ((H[3] * xc + H[4] * yc) + H[5]) / Z + cyj;
            lo_x = fmin(lo_x, u); hi_x = fmax(hi_x, u);
            lo_y = fmin(lo_y, v); hi_y = fmax(hi_y, v);
        }
        s_skip = pos == 0 || (pos == 4 && (hi_x < -1.0 || lo_x > (double)wj || hi_y < -1.0 ||
                                           lo_y > (double)hj));
    }
    __syncthreads();
    if (s_skip) {
        if (tid < PH_NS) out[tid] = 0.0;
        return;
    }

    const frame_ptr fi = (frame_ptr)P.fi, fj = (frame_ptr)P.fj;
    const int64_t pitch_i = P.pitch_i, pitch_j = P.pitch_j;
    const double den_i = (double)((int64_t)wi * wi + (int64_t)hgt_i * hgt_i);
    const double den_j = (double)((int64_t)wj * wj + (int64_t)hj * hj);
    const double g[3] = {P.dlg[0], P.dlg[1], P.dlg[2]};
    const float flo = (float)lo_v, fhi = (float)hi_v;
    const int lx = tx0 + (tid & 63), wave = tid >> 6;
    double acc[PH_NS];
#pragma unroll
    for (int k = 0; k < PH_NS; ++k) acc[k] = 0.0;
    if (lx < lw) {
        const int x = lx * step;
        const double xc = (double)x - cxi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ly = ty0 + wave * 4 + r;
            if (ly >= lh) break;
            const int y = ly * step;
            const double yc = (double)y - cyi;
            const double X = (H[0] * xc + H[1] * yc) + H[2];
            const double Y = (H[3] * xc + H[4] * yc) + H[5];
            const double Z = (H[6] * xc + H[7] * yc) + H[8];
            if (!(Z > 0.0)) continue;
            const double px = X / Z + cxj, py = Y / Z + cyj;
            if (!(px >= 0.0 && px <= (double)(wj - 1) && py >= 0.0 && py <= (double)(hj - 1)))
                continue;
            const int sx = (int)rint(32.0 * px), sy = (int)rint(32.0 * py);
            const int ix = min(sx >> 5, wj - 2), iy = min(sy >> 5, hj - 2);
            const float tx = (float)(sx - 32 * ix) * (1.0f / 32.0f);
            const float ty = (float)(sy - 32 * iy) * (1.0f / 32.0f);
            // a row's two taps are six neighbouring bytes; they end at 3 (ix + 2) - 1 <= 3 wj - 1
            const frame_ptr r0 = fj + (int64_t)iy * pitch_j + 3 * ix, r1 = r0 + pitch_j;
            uint32_t t[2][3], b[2][3];
            rgb2_load(r0, t);
            rgb2_load(r1, b);
            const frame_ptr q = fi + (int64_t)y * pitch_i + 3 * x;
            const uint32_t vi[3] = {q[0], q[1], q[2]};
            float vj[3];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = (float)t[0][c] * (1.0f - tx) + (float)t[1][c] * tx;
                const float bot = (float)b[0][c] * (1.0f - tx) + (float)b[1][c] * tx;
                vj[c] = top * (1.0f - ty) + bot * ty;
                ok = ok && vj[c] >= flo && vj[c] <= fhi && vi[c] >= (uint32_t)lo_v &&
                     vi[c] <= (uint32_t)hi_v;
            }
            if (!ok) continue;

            const double rho_i = photo_rho((double)(2 * x + 1 - wi), (double)(2 * y + 1 - hgt_i), den_i);
            const double qx = (double)sx / 32.0, qy = (double)sy / 32.0;
            const double rho_j = photo_rho((2.0 * qx + 1.0) - (double)wj, (2.0 * qy + 1.0) - (double)hj, den_j);
            double e[3];
            e[0] = rho_i - rho_j;
            e[1] = rho_i * rho_i - rho_j * rho_j;
            e[2] = (rho_i * rho_i) * rho_i - (rho_j * rho_j) * rho_j;
            const double fall = (a1 * e[0] + a2 * e[1]) + a3 * e[2];
            double d[3], m = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                d[c] = s_log[vi[c]] - log((double)vj[c]);
                m = fmax(m, fabs((d[c] - g[c]) - fall));
            }
            const double wt = m > tau ? tau / m : 1.0;
            acc[0] += wt;
            const double we[3] = {wt * e[0], wt * e[1], wt * e[2]};
            acc[1] += we[0];
            acc[2] += we[1];
            acc[3] += we[2];
            acc[4] += we[0] * e[0];
            acc[5] += we[0] * e[1];
            acc[6] += we[0] * e[2];
            acc[7] += we[1] * e[1];
            acc[8] += we[1] * e[2];
            acc[9] += we[2] * e[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double wd = wt * d[c];
                acc[10 + 5 * c] += wd;
                acc[11 + 5 * c] += wd * e[0];
                acc[12 + 5 * c] += wd * e[1];
                acc[13 + 5 * c] += wd * e[2];
                acc[14 + 5 * c] += wd * d[c];
            }
        }
    }
    const double sum = block_sum_fixed<PH_NS>(acc, s_red, tid & 63, wave);
    if (tid < PH_NS) out[tid] = sum;
}

// sums[pair] = the sum of the pair's partials, in a fixed order: the record says where they start
// and how many they are.
__global__ __launch_bounds__(256) void photo_reduce_kernel(const PhotoPairDev *__restrict__ table,
                                                           const double *__restrict__ partials,
                                                           double *__restrict__ sums) {
    __shared__ double s_red[4][PH_NS];
    const PhotoPairDev &P = table[blockIdx.x];
    const double sum = block_sum_partials<PH_NS>(partials + P.part0 * PH_NS, P.nblk, s_red);
    if (threadIdx.x < PH_NS) sums[(size_t)blockIdx.x * PH_NS + threadIdx.x] = sum;
}

extern "C" int pano_photo_stats(pano_ctx *ctx, const pano_photo_frame *frames, int n_frames,
                                const pano_photo_pair *pairs, int n_pairs, int step, int lo, int hi,
                                const double *log_gains, const double *alpha, double tau,
                                double *sums) {
    PANO_ENTER(ctx, "pano_photo_stats");
    PANO_REQUIRE(frames && pairs && log_gains && alpha && sums, "pano_photo_stats: null pointer");
    PANO_REQUIRE(n_frames >= 1 && n_pairs >= 0, "pano_photo_stats: %d frames, %d pairs", n_frames,
                 n_pairs);
    PANO_REQUIRE(step >= 1 && step <= PANO_PHOTO_MAX_SIDE, "pano_photo_stats: step %d (1 .. %d)", step,
                 PANO_PHOTO_MAX_SIDE);
    PANO_REQUIRE(lo >= 1 && hi <= 255 && lo <= hi, "pano_photo_stats: range [%d, %d] (1 <= lo <= hi <= 255)",
                 lo, hi);
    PANO_REQUIRE(tau > 0.0, "pano_photo_stats: tau %g (> 0, +infinity allowed)", tau);
    for (int i = 0; i < n_frames; ++i) {
        const pano_photo_frame &F = frames[i];
        PANO_REQUIRE(F.img, "pano_photo_stats: frame %d: null pointer", i);
        PANO_REQUIRE(F.w >= 2 && F.h >= 2 && F.w <= PANO_PHOTO_MAX_SIDE && F.h <= PANO_PHOTO_MAX_SIDE,
                     "pano_photo_stats: frame %d: %d x %d (sides 2 .. %d)", i, F.w, F.h,
                     PANO_PHOTO_MAX_SIDE);
        PANO_REQUIRE(F.pitch >= 3 * (int64_t)F.w, "pano_photo_stats: frame %d: pitch %lld for %d pixels",
                     i, (long long)F.pitch, F.w);
        for (int c = 0; c < 3; ++c)
            PANO_REQUIRE(isfinite(log_gains[3 * i + c]), "pano_photo_stats: frame %d: a log-gain is not finite", i);
    }
    PANO_REQUIRE(isfinite(alpha[0]) && isfinite(alpha[1]) && isfinite(alpha[2]),
                 "pano_photo_stats: a falloff coefficient is not finite");
    for (int p = 0; p < n_pairs; ++p) {
        const pano_photo_pair &Q = pairs[p];
        PANO_REQUIRE(Q.i >= 0 && Q.i < n_frames && Q.j >= 0 && Q.j < n_frames && Q.i != Q.j,
                     "pano_photo_stats: pair %d: cameras %d, %d of %d", p, Q.i, Q.j, n_frames);
        for (int k = 0; k < 9; ++k)
            PANO_REQUIRE(isfinite(Q.H[k]), "pano_photo_stats: pair %d: H is not finite", p);
    }
    if (n_pairs == 0) return PANO_OK;

    std::vector<PhotoPairDev> table((size_t)n_pairs);
    std::vector<int> blocks((size_t)ceil_div(n_pairs, PH_CHUNK), 0);
    int64_t parts = 0;
    for (int p = 0; p < n_pairs; ++p) {
        PhotoPairDev &D = table[p];
        const pano_photo_frame &A = frames[pairs[p].i], &B = frames[pairs[p].j];
        for (int k = 0; k < 9; ++k) D.H[k] = pairs[p].H[k];
        for (int c = 0; c < 3; ++c)
            D.dlg[c] = log_gains[3 * pairs[p].i + c] - log_gains[3 * pairs[p].j + c];
        D.fi = A.img, D.fj = B.img;
        D.pitch_i = A.pitch, D.pitch_j = B.pitch;
        D.wi = A.w, D.hi = A.h, D.wj = B.w, D.hj = B.h;
        // (the lattice: every step-th pixel of frame i)
        D.nblk = batch_assign<PANO_PHOTO_MAX_SIDE, PH_TW, PH_TH, PH_CHUNK>(
            D.slot, blocks.data(), p, ceil_div(A.w, step), ceil_div(A.h, step));
        D.part0 = parts;
        D.reserved = 0;
        parts += D.nblk;
    }
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = pano_buf_reserve_sync(ctx, BUF_PHOTO_PARTIALS, (size_t)parts * PH_NS * sizeof(double), s))
        return rc;
    double *const par = (double *)ctx->buf[BUF_PHOTO_PARTIALS].p;
    if (int rc = batch_run(ctx, BUF_PHOTO_DEV, table, PH_CHUNK, blocks.data(), s, "photo_stats_kernel",
                           [&](const PhotoPairDev *records, int count, int grid) {
            PANO_TIMED(PK_PHOTO_STATS, s,
                       hipLaunchKernelGGL(photo_stats_kernel, dim3((unsigned)grid), dim3(256), 0, s, records,
                                          count, step, lo, hi, alpha[0], alpha[1], alpha[2], tau, par));
        }))
        return rc;
    hipLaunchKernelGGL(photo_reduce_kernel, dim3((unsigned)n_pairs), dim3(256), 0, s,
                       (const PhotoPairDev *)ctx->buf[BUF_PHOTO_DEV].p, (const double *)par, sums);
    PANO_LAUNCH_CHECK("photo_reduce_kernel");
    return PANO_OK;
}

// ---- the correction ----------------------------------------------------------------
#define PA_PX 4                     // neighbouring pixels of a row a thread owns: 12 bytes, 3 dwords
#define PA_GX 16                    // threads across a tile: 64 pixels
#define PA_GY 16                    // rows of a tile
#define PA_TX (PA_GX * PA_PX)
#define PA_CHUNK 64                 // frames of one launch

struct PhotoApplyDev {              // a frame of a launch, in device memory
    pano_photo_apply f;
    TileSlot slot;
};

// One workgroup per 64 x 16 tile of one frame, one thread per four neighbouring pixels of a row;
// the frame comes from the table's prefix of workgroup counts (batch.h).  A thread reads its
// twelve bytes before it writes them, so dst may be src.
__global__ __launch_bounds__(PA_GX *PA_GY) void photo_apply_kernel(
    const PhotoApplyDev *__restrict__ table, int n) {
    int tile;
    const PhotoApplyDev &D = batch_record(table, n, tile);
    const pano_photo_apply &F = D.f;
    const int u0 = (tile % D.slot.tiles_x) * PA_TX + ((int)threadIdx.x % PA_GX) * PA_PX;
    const int v = (tile / D.slot.tiles_x) * PA_GY + (int)threadIdx.x / PA_GX;
    const int w = F.w, h = F.h;
    if (u0 >= w || v >= h) return;
    typedef const __attribute__((address_space(1))) float *table_ptr;
    const table_ptr T = (table_ptr)F.table;

    uint32_t b[PA_PX][3];
    rgb4_load((frame_ptr)F.src + (int64_t)v * F.src_pitch + 3 * u0, u0, w, b);
    const double den = (double)((int64_t)w * w + (int64_t)h * h);
    const int64_t dy = 2 * (int64_t)v + 1 - h;
#pragma unroll
    for (int j = 0; j < PA_PX; ++j) {
        const int64_t dx = 2 * (int64_t)(u0 + j) + 1 - w;
        const double s = (double)(dx * dx + dy * dy) / den * 1024.0;
        // (s < 1024 inside a frame; the clamp keeps a thread past the row's end inside the table)
        const int k = min((int)s, PANO_PHOTO_TABLE - 2);
        const float t = (float)(s - (double)k);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f0 = T[c * PANO_PHOTO_TABLE + k], f1 = T[c * PANO_PHOTO_TABLE + k + 1];
            const float f = f0 + t * (f1 - f0);
            b[j][c] = (uint32_t)rintf(fmaxf(fminf((float)b[j][c] * f, 255.0f), 0.0f));
        }
    }
    rgb4_store((rgb_out_ptr)F.dst + (int64_t)v * F.dst_pitch + 3 * u0, u0, w, b);
}

static int photo_apply_check(const pano_photo_apply &F, int i) {
    PANO_REQUIRE(F.src && F.dst && F.table, "pano_photo_apply_u8: frame %d: null pointer", i);
    return rgb_frames_check("pano_photo_apply_u8", i, F.src, F.src_pitch, F.dst, F.dst_pitch, F.w, F.h,
                            PANO_PHOTO_MAX_SIDE, true);
}

extern "C" int pano_photo_apply_u8(pano_ctx *ctx, const pano_photo_apply *frames, int n) {
    PANO_ENTER(ctx, "pano_photo_apply_u8");
    PANO_REQUIRE(frames, "pano_photo_apply_u8: null pointer");
    PANO_REQUIRE(n >= 1, "pano_photo_apply_u8: %d frames", n);
    for (int i = 0; i < n; ++i)                         // (nothing is queued for a refused batch)
        if (int rc = photo_apply_check(frames[i], i)) return rc;

    std::vector<PhotoApplyDev> table((size_t)n);
    std::vector<int> blocks((size_t)ceil_div(n, PA_CHUNK), 0);
    for (int i = 0; i < n; ++i) {
        PhotoApplyDev &D = table[i];
        D.f = frames[i];
        batch_assign<PANO_PHOTO_MAX_SIDE, PA_TX, PA_GY, PA_CHUNK>(D.slot, blocks.data(), i, D.f.w, D.f.h);
    }
    const hipStream_t s = (hipStream_t)stream;
    return batch_run(ctx, BUF_PHOTO_DEV, table, PA_CHUNK, blocks.data(), s, "photo_apply_kernel",
                     [&](const PhotoApplyDev *records, int count, int grid) {
        hipLaunchKernelGGL(photo_apply_kernel, dim3((unsigned)grid), dim3(PA_GX * PA_GY), 0, s, records, count);
    });
}
