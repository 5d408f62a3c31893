// Poisson (seamless cloning) blend: blend.poisson_blend of the reference (blend.py:143-203), its
// sparse direct solve replaced by a float64 BiCGStab iteration on the pixel grid.  The contract -
// the two stencils with the reference's quirks, the stopping rule, the summation structure - is
// in include/pano360.h; tests/poisson_model.py restates the stencils in NumPy.
//
// Layout.  Every vector is [c][stride] float64, stride = h w rounded up to PB_TILE, a plane per
// channel; flat index i = y w + x.  A block owns PB_TILE consecutive elements of one channel
// (blockIdx.x = tile, blockIdx.y = channel); a lane takes two neighbouring elements (16 bytes of
// every vector) per pass, PB_PASSES passes.  The stencil's flat neighbours i-1, i+1 come from the
// lane's own pair or one extra 8-byte load, i-w and i+w from two; every link is a predicate on
// the column (x == 0, w-2, w-1) folded into a select, so a wave never branches on a column.
// A wave whose 128 elements hold no mask pixel skips the pass: outside the mask x keeps the
// target and every Krylov vector stays 0, which is what the identity rows of A compute.
//
// One iteration is three vector kernels and two one-block scalar kernels:
//   pb_apply_p   v = A p                          partial (rhat, v)
//   pb_alpha     (closes the previous iteration, see pb_check;) alpha = rho / (rhat, v)
//   pb_apply_s   t = A s, s = r - alpha v formed on the fly at the five points (s is never
//                stored)                          partials (t, s), (t, t), (rhat, s), (rhat, t)
//   pb_omega     omega = (t, s) / (t, t); rho' = (rhat, s) - omega (rhat, t) = (rhat, r');
//                beta = (rho' / rho) (alpha / omega)
//   pb_update    x += alpha p + omega s; r = s - omega t; p = r + beta (p - omega v)
//                                                 partial (r, r)
//   pb_check     converged when (r, r) <= rtol^2 (b, b); breakdown flags.  A launch of its own
//                only at the end of a chunk; between iterations pb_alpha does it first
// Scalars and flags live in device memory (PbChan per channel); a channel whose state is not
// "running" makes every block of its kernels return at once, so a converged channel freezes
// while the others go on.  Sums: each lane adds its elements in pass order, a wave by a fixed
// xor butterfly, the block's four waves in order, the blocks' partials by pb_block_totals (lane t
// takes partials t, t + 256, .. in order, then the same butterfly and wave order).  No atomics:
// the same input gives the same bits.
#include <math.h>

#include "common.h"
#include "wave.h"

#define PB_BLOCK 256
#define PB_WAVES (PB_BLOCK / 64)
#define PB_PASSES 4
#define PB_TILE (2 * PB_BLOCK * PB_PASSES)       // elements of one channel per block
#define PB_PARTS 4                               // partial sums a vector kernel leaves per block
// Iterations queued between two readbacks of the channels' flags.  A readback drains the stream
// (tens of microseconds); an iteration of an overlap-sized blend (1080 x 976 x 3) is 64 us, so
// 32 keeps the drain under a few percent of a chunk, and what a chunk queues past convergence is
// at most 31 iterations of kernels that return on their first load.
#define PB_CHUNK PANO_POISSON_CHUNK

#define PB_RUNNING 0
#define PB_CONVERGED 1
#define PB_BREAKDOWN 2

struct PbChan {                 // 64 bytes per channel, device memory (and its pinned host copy)
    double rho, alpha, omega, beta, bnorm2, rr, thr;
    int32_t state, iters;
};
static_assert(sizeof(PbChan) == 64, "PbChan is read back as 64-byte records");

struct PbLinks {
    bool l, r, u, d;
};

// links of row j of A (blend.py:157-172): flat neighbours inside 0..n-1, i-1 dropped at x == 0,
// i+1 dropped at x == w-2; a pixel at x == w-1 keeps i+1, the next row's first pixel
__device__ __forceinline__ PbLinks pb_links_A(int j, int xj, int w, int n) {
    return PbLinks{xj != 0, j + 1 < n && xj != w - 2, j >= w, j + w < n};
}

// links of row j of P (blend.py:149-154): as A, and nobody reads column w-1, which takes the
// vertical neighbours of a last-column pixel too
__device__ __forceinline__ PbLinks pb_links_P(int j, int xj, int w, int n) {
    return PbLinks{xj != 0, j + 1 < n && xj != w - 2, j >= w && xj != w - 1,
                   j + w < n && xj != w - 1};
}

// the block's sum of v in thread 0 (waves in order); lds: PB_WAVES doubles of its own
__device__ __forceinline__ double pb_block_sum(double v, double *lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int k = 1; k < PB_WAVES; ++k) s += lds[k];
    return s;
}

// sums of K of one channel's arrays of per-block partials (slots first .. first + K - 1), the
// same in every thread; lds: K x PB_WAVES doubles.  The K arrays are loaded side by side so that
// their memory latencies overlap: these one-block kernels are latency, not work.
template <int K>
__device__ __forceinline__ void pb_block_totals(const double *__restrict__ part, int nblk,
                                                double (*lds)[PB_WAVES], double (&out)[K]) {
    double acc[K];
#pragma unroll
    for (int q = 0; q < K; ++q) acc[q] = 0.0;
    for (int k = threadIdx.x; k < nblk; k += PB_BLOCK) {
#pragma unroll
        for (int q = 0; q < K; ++q) acc[q] += part[(size_t)q * nblk + k];
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
        acc[q] = wave_sum(acc[q]);
        if ((threadIdx.x & 63) == 0) lds[q][threadIdx.x >> 6] = acc[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        double t = lds[q][0];
#pragma unroll
        for (int w = 1; w < PB_WAVES; ++w) t += lds[q][w];
        out[q] = t;
    }
}

// 4 c - (the linked neighbours), left to right: left, right, up, down
__device__ __forceinline__ double pb_row(PbLinks k, double c, double l, double r, double u,
                                         double d) {
    double v = 4.0 * c;
    v -= k.l ? l : 0.0;
    v -= k.r ? r : 0.0;
    v -= k.u ? u : 0.0;
    v -= k.d ? d : 0.0;
    return v;
}

__device__ __forceinline__ int pb_clampi(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }

// ---- setup: x0 = target, r0 = b - A x0, rhat = p = r0, v = 0 ---------------------------------
// src, tgt: uint8 [h][w][c] interleaved.  Sums of small integers: exact.
__global__ __launch_bounds__(PB_BLOCK) void pb_setup_kernel(
    const uint8_t *__restrict__ src, const uint8_t *__restrict__ tgt,
    const uint8_t *__restrict__ mask, int w, int n, int nc, int stride, double *__restrict__ x,
    double *__restrict__ r, double *__restrict__ rh, double *__restrict__ p,
    double *__restrict__ v, double *__restrict__ part, int nblk) {
    __shared__ double lds[2][PB_WAVES];
    const int c = blockIdx.y;
    const size_t plane = (size_t)c * stride;
    double bb = 0.0, rr = 0.0;
    for (int pass = 0; pass < 2 * PB_PASSES; ++pass) {
        const int j = blockIdx.x * PB_TILE + pass * PB_BLOCK + threadIdx.x;
        double x0 = 0.0, r0 = 0.0;
        if (j < n) {
            x0 = (double)tgt[(size_t)j * nc + c];
            double b = x0;
            if (mask[j]) {
                const int xj = j % w;
                const int jl = pb_clampi(j - 1, n), jr = pb_clampi(j + 1, n);
                const int ju = pb_clampi(j - w, n), jd = pb_clampi(j + w, n);
                b = pb_row(pb_links_P(j, xj, w, n), (double)src[(size_t)j * nc + c],
                           (double)src[(size_t)jl * nc + c], (double)src[(size_t)jr * nc + c],
                           (double)src[(size_t)ju * nc + c], (double)src[(size_t)jd * nc + c]);
                const double ax = pb_row(pb_links_A(j, xj, w, n), x0,
                                         (double)tgt[(size_t)jl * nc + c],
                                         (double)tgt[(size_t)jr * nc + c],
                                         (double)tgt[(size_t)ju * nc + c],
                                         (double)tgt[(size_t)jd * nc + c]);
                r0 = b - ax;
            }
            bb += b * b;
            rr += r0 * r0;
        }
        x[plane + j] = x0;
        r[plane + j] = r0;
        rh[plane + j] = r0;
        p[plane + j] = r0;
        v[plane + j] = 0.0;
    }
    bb = pb_block_sum(bb, lds[0]);
    rr = pb_block_sum(rr, lds[1]);
    if (threadIdx.x == 0) {
        part[((size_t)c * PB_PARTS + 0) * nblk + blockIdx.x] = bb;
        part[((size_t)c * PB_PARTS + 1) * nblk + blockIdx.x] = rr;
    }
}

__global__ __launch_bounds__(PB_BLOCK) void pb_start_kernel(const double *__restrict__ part,
                                                            int nblk, double rtol,
                                                            PbChan *__restrict__ chan) {
    __shared__ double lds[2][PB_WAVES];
    const int c = blockIdx.x;
    double sums[2];
    pb_block_totals<2>(part + (size_t)c * PB_PARTS * nblk, nblk, lds, sums);
    const double bb = sums[0], rr = sums[1];
    if (threadIdx.x == 0) {
        PbChan k;
        k.rho = rr;                      // (rhat, r0) with rhat = r0
        k.alpha = k.omega = 1.0;
        k.beta = 0.0;
        k.bnorm2 = bb;
        k.rr = rr;
        k.thr = rtol * rtol * bb;
        k.state = !isfinite(rr) ? PB_BREAKDOWN : (rr <= k.thr ? PB_CONVERGED : PB_RUNNING);
        k.iters = 0;
        chan[c] = k;
    }
}

// ---- v = A p, partial (rhat, v) ---------------------------------------------------------------
__global__ __launch_bounds__(PB_BLOCK) void pb_apply_p_kernel(
    const uint8_t *__restrict__ mask, int w, int n, int stride, const PbChan *__restrict__ chan,
    const double *__restrict__ p, const double *__restrict__ rh, double *__restrict__ v,
    double *__restrict__ part, int nblk) {
    __shared__ double lds[PB_WAVES];
    const int c = blockIdx.y;
    if (chan[c].state != PB_RUNNING) return;
    const size_t plane = (size_t)c * stride;
    p += plane, rh += plane, v += plane;
    double acc = 0.0;
#pragma unroll
    for (int pass = 0; pass < PB_PASSES; ++pass) {
        const int i = blockIdx.x * PB_TILE + pass * 2 * PB_BLOCK + 2 * threadIdx.x;
        const bool m0 = i < n && mask[i], m1 = i + 1 < n && mask[i + 1];
        if (__ballot(m0 || m1) == 0) continue;
        const double2 pc = *(const double2 *)(p + i);
        const double2 hc = *(const double2 *)(rh + i);
        const int x0 = i % w, x1 = x0 + 1 == w ? 0 : x0 + 1;
        const double pl = p[pb_clampi(i - 1, n)], pr = p[pb_clampi(i + 2, n)];
        const double u0 = p[pb_clampi(i - w, n)], u1 = p[pb_clampi(i + 1 - w, n)];
        const double d0 = p[pb_clampi(i + w, n)], d1 = p[pb_clampi(i + 1 + w, n)];
        double2 out;
        out.x = m0 ? pb_row(pb_links_A(i, x0, w, n), pc.x, pl, pc.y, u0, d0) : pc.x;
        out.y = m1 ? pb_row(pb_links_A(i + 1, x1, w, n), pc.y, pc.x, pr, u1, d1) : pc.y;
        *(double2 *)(v + i) = out;
        acc += hc.x * out.x + hc.y * out.y;
    }
    acc = pb_block_sum(acc, lds);
    if (threadIdx.x == 0) part[((size_t)c * PB_PARTS + 0) * nblk + blockIdx.x] = acc;
}

// after an iteration's update: (r, r) against the threshold, and what pb_omega found.  Every
// thread of the block holds the same rr and reaches the same verdict; thread 0 records it.
__device__ __forceinline__ int pb_verdict(double rr, int iter, PbChan *__restrict__ chan) {
    int state = PB_RUNNING;
    if (!isfinite(rr))
        state = PB_BREAKDOWN;
    else if (rr <= chan->thr)
        state = PB_CONVERGED;
    else if (isnan(chan->beta))
        state = PB_BREAKDOWN;
    if (threadIdx.x == 0) {
        chan->rr = rr;
        chan->iters = iter;
        chan->state = state;
    }
    return state;
}

// check_prev: first close iteration iter - 1 (pb_check's work, folded in here between the
// iterations of a chunk: one launch less per iteration; pb_apply_p has then run once more than
// needed for a channel that had just converged, which only writes v).
__global__ __launch_bounds__(PB_BLOCK) void pb_alpha_kernel(const double *__restrict__ part,
                                                            int nblk, int iter, int check_prev,
                                                            PbChan *__restrict__ chan) {
    __shared__ double lds[2][PB_WAVES];
    const int c = blockIdx.x;
    if (chan[c].state != PB_RUNNING) return;
    double sums[2];                                // (rhat, v), and (r, r) of iteration iter - 1
    pb_block_totals<2>(part + (size_t)c * PB_PARTS * nblk, nblk, lds, sums);
    if (check_prev && pb_verdict(sums[1], iter - 1, chan + c) != PB_RUNNING) return;
    const double rhv = sums[0];
    if (threadIdx.x == 0) {
        const double alpha = chan[c].rho / rhv;
        chan[c].alpha = alpha;
        if (rhv == 0.0 || !isfinite(alpha)) {      // (rhat, v) = 0: the method cannot step
            chan[c].state = PB_BREAKDOWN;
            chan[c].iters = iter;
        }
    }
}

// ---- t = A s with s = r - alpha v; partials (t,s), (t,t), (rhat,s), (rhat,t) -----------------
__global__ __launch_bounds__(PB_BLOCK) void pb_apply_s_kernel(
    const uint8_t *__restrict__ mask, int w, int n, int stride, const PbChan *__restrict__ chan,
    const double *__restrict__ r, const double *__restrict__ v, const double *__restrict__ rh,
    double *__restrict__ t, double *__restrict__ part, int nblk) {
    __shared__ double lds[PB_PARTS][PB_WAVES];
    const int c = blockIdx.y;
    if (chan[c].state != PB_RUNNING) return;
    const double alpha = chan[c].alpha;
    const size_t plane = (size_t)c * stride;
    r += plane, v += plane, rh += plane, t += plane;
    double ts = 0.0, tt = 0.0, hs = 0.0, ht = 0.0;
#pragma unroll
    for (int pass = 0; pass < PB_PASSES; ++pass) {
        const int i = blockIdx.x * PB_TILE + pass * 2 * PB_BLOCK + 2 * threadIdx.x;
        const bool m0 = i < n && mask[i], m1 = i + 1 < n && mask[i + 1];
        if (__ballot(m0 || m1) == 0) continue;
        const double2 rc = *(const double2 *)(r + i), vc = *(const double2 *)(v + i);
        const double2 hc = *(const double2 *)(rh + i);
        const int x0 = i % w, x1 = x0 + 1 == w ? 0 : x0 + 1;
        const int il = pb_clampi(i - 1, n), ir = pb_clampi(i + 2, n);
        const int iu0 = pb_clampi(i - w, n), iu1 = pb_clampi(i + 1 - w, n);
        const int id0 = pb_clampi(i + w, n), id1 = pb_clampi(i + 1 + w, n);
        const double s0 = rc.x - alpha * vc.x, s1 = rc.y - alpha * vc.y;
        const double sl = r[il] - alpha * v[il], sr = r[ir] - alpha * v[ir];
        const double u0 = r[iu0] - alpha * v[iu0], u1 = r[iu1] - alpha * v[iu1];
        const double d0 = r[id0] - alpha * v[id0], d1 = r[id1] - alpha * v[id1];
        double2 out;
        out.x = m0 ? pb_row(pb_links_A(i, x0, w, n), s0, sl, s1, u0, d0) : s0;
        out.y = m1 ? pb_row(pb_links_A(i + 1, x1, w, n), s1, s0, sr, u1, d1) : s1;
        *(double2 *)(t + i) = out;
        ts += out.x * s0 + out.y * s1;
        tt += out.x * out.x + out.y * out.y;
        hs += hc.x * s0 + hc.y * s1;
        ht += hc.x * out.x + hc.y * out.y;
    }
    ts = pb_block_sum(ts, lds[0]);
    tt = pb_block_sum(tt, lds[1]);
    hs = pb_block_sum(hs, lds[2]);
    ht = pb_block_sum(ht, lds[3]);
    if (threadIdx.x == 0) {
        double *out = part + (size_t)c * PB_PARTS * nblk + blockIdx.x;
        out[0 * (size_t)nblk] = ts;
        out[1 * (size_t)nblk] = tt;
        out[2 * (size_t)nblk] = hs;
        out[3 * (size_t)nblk] = ht;
    }
}

__global__ __launch_bounds__(PB_BLOCK) void pb_omega_kernel(const double *__restrict__ part,
                                                            int nblk, PbChan *__restrict__ chan) {
    __shared__ double lds[PB_PARTS][PB_WAVES];
    const int c = blockIdx.x;
    if (chan[c].state != PB_RUNNING) return;
    double sums[PB_PARTS];
    pb_block_totals<PB_PARTS>(part + (size_t)c * PB_PARTS * nblk, nblk, lds, sums);
    const double ts = sums[0], tt = sums[1], hs = sums[2], ht = sums[3];
    if (threadIdx.x == 0) {
        // t = 0 only when s = 0: x + alpha p is exact, the update leaves r = 0 and pb_check
        // stops the channel
        const double omega = tt > 0.0 ? ts / tt : 0.0;
        const double rho = hs - omega * ht;                 // (rhat, s - omega t)
        const double beta = (rho / chan[c].rho) * (chan[c].alpha / omega);
        chan[c].omega = omega;
        chan[c].rho = rho;
        // rho or omega at zero, or a scalar that is not finite: the next direction is undefined.
        // NaN in beta tells pb_check, which lets a channel that has just converged pass.
        chan[c].beta = (omega == 0.0 || rho == 0.0 || !isfinite(beta)) ? NAN : beta;
    }
}

// ---- x += alpha p + omega s; r = s - omega t; p = r + beta (p - omega v); partial (r, r) ------
__global__ __launch_bounds__(PB_BLOCK) void pb_update_kernel(
    const uint8_t *__restrict__ mask, int n, int stride, const PbChan *__restrict__ chan,
    double *__restrict__ x, double *__restrict__ r, double *__restrict__ p,
    const double *__restrict__ v, const double *__restrict__ t, double *__restrict__ part,
    int nblk) {
    __shared__ double lds[PB_WAVES];
    const int c = blockIdx.y;
    if (chan[c].state != PB_RUNNING) return;
    const double alpha = chan[c].alpha, omega = chan[c].omega;
    const double beta = isnan(chan[c].beta) ? 0.0 : chan[c].beta;
    const size_t plane = (size_t)c * stride;
    x += plane, r += plane, p += plane, v += plane, t += plane;
    double rr = 0.0;
#pragma unroll
    for (int pass = 0; pass < PB_PASSES; ++pass) {
        const int i = blockIdx.x * PB_TILE + pass * 2 * PB_BLOCK + 2 * threadIdx.x;
        const bool m0 = i < n && mask[i], m1 = i + 1 < n && mask[i + 1];
        if (__ballot(m0 || m1) == 0) continue;
        double2 xc = *(const double2 *)(x + i), pc = *(const double2 *)(p + i);
        double2 rc = *(const double2 *)(r + i);
        const double2 vc = *(const double2 *)(v + i), tc = *(const double2 *)(t + i);
        const double s0 = rc.x - alpha * vc.x, s1 = rc.y - alpha * vc.y;
        xc.x += alpha * pc.x + omega * s0;
        xc.y += alpha * pc.y + omega * s1;
        rc.x = s0 - omega * tc.x;
        rc.y = s1 - omega * tc.y;
        pc.x = rc.x + beta * (pc.x - omega * vc.x);
        pc.y = rc.y + beta * (pc.y - omega * vc.y);
        *(double2 *)(x + i) = xc;
        *(double2 *)(r + i) = rc;
        *(double2 *)(p + i) = pc;
        rr += rc.x * rc.x + rc.y * rc.y;
    }
    rr = pb_block_sum(rr, lds);
    // slot 1: the next pb_apply_p fills slot 0 before the folded check reads this
    if (threadIdx.x == 0) part[((size_t)c * PB_PARTS + 1) * nblk + blockIdx.x] = rr;
}

__global__ __launch_bounds__(PB_BLOCK) void pb_check_kernel(const double *__restrict__ part,
                                                            int nblk, int iter,
                                                            PbChan *__restrict__ chan) {
    __shared__ double lds[1][PB_WAVES];
    const int c = blockIdx.x;
    if (chan[c].state != PB_RUNNING) return;
    double rr[1];
    pb_block_totals<1>(part + ((size_t)c * PB_PARTS + 1) * nblk, nblk, lds, rr);
    (void)pb_verdict(rr[0], iter, chan + c);
}

// ---- np.array(np.clip(sol, 0, 255), uint8) into the target at the mask pixels ----------------
__global__ __launch_bounds__(PB_BLOCK) void pb_finish_kernel(const uint8_t *__restrict__ mask,
                                                             int n, int nc, int stride,
                                                             const double *__restrict__ x,
                                                             uint8_t *__restrict__ tgt,
                                                             double *__restrict__ solution) {
    const int j = blockIdx.x * PB_BLOCK + threadIdx.x, c = blockIdx.y;
    if (j >= n) return;
    const double s = x[(size_t)c * stride + j];
    if (solution) solution[(size_t)c * n + j] = s;
    if (mask[j]) {
        const double clipped = s < 0.0 ? 0.0 : (s > 255.0 ? 255.0 : s);
        tgt[(size_t)j * nc + c] = (uint8_t)(int)clipped;       // truncates, as astype does
    }
}

// ---- host ------------------------------------------------------------------------------------
static int pb_reserve(pano_ctx *ctx, size_t bytes) {
    if (int rc = pano_buf_reserve(ctx->buf[BUF_POISSON_HOST], 4 * sizeof(PbChan), true)) return rc;
    // (the last blend's finish kernel may still read the old buffer)
    return pano_buf_reserve_sync(ctx, BUF_POISSON_DEV, bytes, ctx->stream);
}

extern "C" int pano_poisson_blend(pano_ctx *ctx, const uint8_t *src, uint8_t *tgt,
                                  const uint8_t *mask, int h, int w, int c, double rtol,
                                  int max_iters, double *solution, int32_t *iters,
                                  double *resid) {
    PANO_ENTER(ctx, "pano_poisson_blend");
    PANO_REQUIRE(src && tgt && mask, "pano_poisson_blend: null pointer");
    PANO_REQUIRE(h >= 1 && w >= 2 && c >= 1 && c <= 4 && (int64_t)h * w <= (1 << 29),
                 "pano_poisson_blend: %d x %d x %d is outside h >= 1, w >= 2, 1 <= c <= 4, "
                 "h w <= 2^29", h, w, c);
    PANO_REQUIRE(rtol > 0.0 && rtol < 1.0 && max_iters >= 1,
                 "pano_poisson_blend: rtol %g, max_iters %d", rtol, max_iters);
    const hipStream_t s = (hipStream_t)stream;
    const int n = h * w, nblk = (n + PB_TILE - 1) / PB_TILE, stride = nblk * PB_TILE;
    const size_t vec = (size_t)c * stride * sizeof(double);
    const size_t part_bytes = (size_t)c * PB_PARTS * nblk * sizeof(double);
    if (int rc = pb_reserve(ctx, 6 * vec + part_bytes + 4 * sizeof(PbChan))) return rc;
    uint8_t *base = (uint8_t *)ctx->buf[BUF_POISSON_DEV].p;
    double *x = (double *)base, *r = (double *)(base + vec), *rh = (double *)(base + 2 * vec);
    double *p = (double *)(base + 3 * vec), *v = (double *)(base + 4 * vec);
    double *t = (double *)(base + 5 * vec), *part = (double *)(base + 6 * vec);
    PbChan *chan = (PbChan *)(base + 6 * vec + part_bytes), *host = (PbChan *)ctx->buf[BUF_POISSON_HOST].p;

    const dim3 grid(nblk, c), block(PB_BLOCK), one(c);
    hipLaunchKernelGGL(pb_setup_kernel, grid, block, 0, s, src, tgt, mask, w, n, c, stride, x, r,
                       rh, p, v, part, nblk);
    PANO_LAUNCH_CHECK("pb_setup_kernel");
    hipLaunchKernelGGL(pb_start_kernel, one, block, 0, s, part, nblk, rtol, chan);
    PANO_LAUNCH_CHECK("pb_start_kernel");
    bool running = true;
    for (int done = 0; running;) {
        const int chunk = max_iters - done < PB_CHUNK ? max_iters - done : PB_CHUNK;
        for (int k = 1; k <= chunk; ++k) {
            hipLaunchKernelGGL(pb_apply_p_kernel, grid, block, 0, s, mask, w, n, stride, chan, p,
                               rh, v, part, nblk);
            hipLaunchKernelGGL(pb_alpha_kernel, one, block, 0, s, part, nblk, done + k, k > 1,
                               chan);
            hipLaunchKernelGGL(pb_apply_s_kernel, grid, block, 0, s, mask, w, n, stride, chan, r,
                               v, rh, t, part, nblk);
            hipLaunchKernelGGL(pb_omega_kernel, one, block, 0, s, part, nblk, chan);
            hipLaunchKernelGGL(pb_update_kernel, grid, block, 0, s, mask, n, stride, chan, x, r,
                               p, v, t, part, nblk);
        }
        hipLaunchKernelGGL(pb_check_kernel, one, block, 0, s, part, nblk, done + chunk, chan);
        PANO_LAUNCH_CHECK("the Poisson iteration");
        done += chunk;
        PANO_HIP(hipMemcpyAsync(host, chan, c * sizeof(PbChan), hipMemcpyDeviceToHost, s));
        PANO_HIP(hipStreamSynchronize(s));
        running = false;
        for (int k = 0; k < c; ++k) running |= host[k].state == PB_RUNNING;
        if (done >= max_iters) break;
    }
    for (int k = 0; k < c; ++k) {
        const double rel = host[k].bnorm2 > 0.0 ? sqrt(host[k].rr / host[k].bnorm2) : 0.0;
        if (iters) iters[k] = host[k].iters;
        if (resid) resid[k] = rel;
        if (host[k].state == PB_CONVERGED) continue;
        if (host[k].state == PB_BREAKDOWN)
            pano_set_error("pano_poisson_blend: BiCGStab broke down in channel %d at iteration %d "
                           "(relative residual %.3e)", k, host[k].iters, rel);
        else
            pano_set_error("pano_poisson_blend: channel %d has not converged after %d iterations "
                           "(relative residual %.3e, wanted %.3e)", k, max_iters, rel, rtol);
        return PANO_ESOLVE;
    }
    const dim3 fgrid((n + PB_BLOCK - 1) / PB_BLOCK, c);
    hipLaunchKernelGGL(pb_finish_kernel, fgrid, block, 0, s, mask, n, c, stride, x, tgt, solution);
    PANO_LAUNCH_CHECK("pb_finish_kernel");
    return PANO_OK;
}
