// Pairwise registration's last step: Lowe's ratio test over a pano_knn2 result, packed into
// correspondences (pano_match_pack), then a RANSAC homography for every pair of a batch
// (pano_hom_ransac) - what features.py:235-252 gets from flann_matching and
// cv2.findHomography(..., cv2.RANSAC).  The contract (sampler, degeneracy test, 4-point solve,
// score, selection, refit) is pinned in include/pano360.h so that a NumPy model reproduces every
// score bit for bit; this file follows it operation for operation.
//
// Score kernel: one lane per hypothesis, (max_iters / 256, n_pairs) blocks of 256.  A lane draws
// its sample and solves the 8 x 8 system in f64 registers (fully unrolled: row swaps are selects,
// no run-time indexed per-lane array), rounds it to float32, then the block streams the pair's
// correspondences through LDS in tiles of 1024 float4; every lane reads the same LDS word (a
// broadcast) and runs the float32 test - ~30 VALU instructions per (hypothesis, correspondence),
// most of them the correctly rounded division.  Finish kernel: one block per pair - the argmax,
// the mask, the normalised DLT's sums (per-lane partials in a fixed order, a butterfly per wave,
// the four waves in order) and a cyclic Jacobi on one lane in LDS.
#include <math.h>

#include "common.h"
#include "wave.h"

#define RANSAC_BLOCK 256
#define RANSAC_TILE 1024
#define RANSAC_ATTEMPTS 64
#define RANSAC_MAX_ITERS (1 << 20)
#define RANSAC_GAMMA 0x9E3779B97F4A7C15ull
#define PACK_BLOCK 1024

__device__ __forceinline__ uint64_t ransac_splitmix64(uint64_t x) {
    uint64_t z = x + RANSAC_GAMMA;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ int ransac_draw(uint64_t seed, uint32_t h, int attempt, int k,
                                           uint32_t count) {
    const uint64_t key = (uint64_t)h * 256u + (uint64_t)(attempt * 4 + k + 1);
    const uint64_t r = ransac_splitmix64(seed + RANSAC_GAMMA * key);
    return (int)(((r >> 32) * (uint64_t)count) >> 32);
}

// twice the signed area of the triangle a b c
__device__ __forceinline__ double ransac_area(double ax, double ay, double bx, double by, double cx,
                                              double cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// the src and dst triangles a b c have the same strict orientation (a NaN fails)
__device__ __forceinline__ bool ransac_same_side(const double (&x)[4], const double (&y)[4],
                                                 const double (&u)[4], const double (&v)[4], int a,
                                                 int b, int c) {
    const double s = ransac_area(x[a], y[a], x[b], y[b], x[c], y[c]);
    const double d = ransac_area(u[a], v[a], u[b], v[b], u[c], v[c]);
    return s * d > 0.0;
}

// The first acceptable of RANSAC_ATTEMPTS draws of hypothesis h: four distinct indices whose
// four triples keep their orientation from src to dst.  false: none (the hypothesis is invalid).
__device__ bool ransac_sample(const float4 *P, uint32_t count, uint64_t seed, uint32_t h,
                              double (&x)[4], double (&y)[4], double (&u)[4], double (&v)[4]) {
    for (int a = 0; a < RANSAC_ATTEMPTS; ++a) {
        const int i0 = ransac_draw(seed, h, a, 0, count), i1 = ransac_draw(seed, h, a, 1, count);
        const int i2 = ransac_draw(seed, h, a, 2, count), i3 = ransac_draw(seed, h, a, 3, count);
        if (i0 == i1 || i0 == i2 || i0 == i3 || i1 == i2 || i1 == i3 || i2 == i3) continue;
        const float4 p0 = P[i0], p1 = P[i1], p2 = P[i2], p3 = P[i3];
        x[0] = p0.x, y[0] = p0.y, u[0] = p0.z, v[0] = p0.w;
        x[1] = p1.x, y[1] = p1.y, u[1] = p1.z, v[1] = p1.w;
        x[2] = p2.x, y[2] = p2.y, u[2] = p2.z, v[2] = p2.w;
        x[3] = p3.x, y[3] = p3.y, u[3] = p3.z, v[3] = p3.w;
        if (ransac_same_side(x, y, u, v, 0, 1, 2) && ransac_same_side(x, y, u, v, 0, 1, 3) &&
            ransac_same_side(x, y, u, v, 0, 2, 3) && ransac_same_side(x, y, u, v, 1, 2, 3))
            return true;
    }
    return false;
}

// The exact homography (h33 = 1) through four correspondences: the 8 x 8 system, Gaussian
// elimination with partial pivoting (the first maximal |pivot|; a NaN counts as maximal, as
// NumPy's argmax has it), back substitution.  Every index is a compile-time constant: the row
// swap is a select per element.  false: a zero or non-finite pivot.
__device__ __forceinline__ bool ransac_solve4(const double (&x)[4], const double (&y)[4],
                                              const double (&u)[4], const double (&v)[4],
                                              double (&h)[8]) {
    double A[8][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double *r0 = A[2 * i], *r1 = A[2 * i + 1];
        r0[0] = x[i], r0[1] = y[i], r0[2] = 1.0, r0[3] = 0.0, r0[4] = 0.0, r0[5] = 0.0;
        r0[6] = -(u[i] * x[i]), r0[7] = -(u[i] * y[i]), r0[8] = u[i];
        r1[0] = 0.0, r1[1] = 0.0, r1[2] = 0.0, r1[3] = x[i], r1[4] = y[i], r1[5] = 1.0;
        r1[6] = -(v[i] * x[i]), r1[7] = -(v[i] * y[i]), r1[8] = v[i];
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int p = c;
        double best = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double a = fabs(A[r][c]);
            const bool take = !(best != best) && (a != a || a > best);
            best = take ? a : best;
            p = take ? r : p;
        }
        ok = ok && best > 0.0 && best < INFINITY;
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int k = c; k < 9; ++k) {
                const double top = A[c][k];
                A[c][k] = sw ? A[r][k] : top;
                A[r][k] = sw ? top : A[r][k];
            }
        }
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double f = A[r][c] / A[c][c];
#pragma unroll
            for (int k = c + 1; k < 9; ++k) A[r][k] = A[r][k] - f * A[c][k];
        }
    }
#pragma unroll
    for (int r = 7; r >= 0; --r) {
        double s = A[r][8];
#pragma unroll
        for (int k = r + 1; k < 8; ++k) s = s - A[r][k] * h[k];
        h[r] = s / A[r][r];
    }
    return ok;
}

// hypothesis h of a pair, rounded to float32 (zeros when invalid)
__device__ __forceinline__ bool ransac_hypothesis(const float4 *P, uint32_t count, uint64_t seed,
                                                  uint32_t h, float (&hf)[8]) {
    double x[4], y[4], u[4], v[4], H[8];
    bool ok = ransac_sample(P, count, seed, h, x, y, u, v);
    if (ok) ok = ransac_solve4(x, y, u, v, H);
#pragma unroll
    for (int k = 0; k < 8; ++k) hf[k] = ok ? (float)H[k] : 0.0f;
    return ok;
}

// the reprojection test of one correspondence, float32 in this order
__device__ __forceinline__ bool ransac_inlier(const float (&hf)[8], float4 q, float t2) {
    const float ww = 1.0f / ((hf[6] * q.x + hf[7] * q.y) + 1.0f);
    const float dx = ((hf[0] * q.x + hf[1] * q.y) + hf[2]) * ww - q.z;
    const float dy = ((hf[3] * q.x + hf[4] * q.y) + hf[5]) * ww - q.w;
    const float err = dx * dx + dy * dy;
    return err <= t2;
}

__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_score_kernel(
    const float4 *__restrict__ pts, const int32_t *__restrict__ offsets,
    const int32_t *__restrict__ counts, int max_iters, float t2, uint64_t seed,
    int32_t *__restrict__ scores) {
    __shared__ float4 tile[RANSAC_TILE];
    const int pair = blockIdx.y;
    const int count = counts[pair];                 // the same for the whole block
    const int h = blockIdx.x * RANSAC_BLOCK + threadIdx.x;
    int32_t *out = scores + (size_t)pair * max_iters;
    if (count < 4) {
        if (h < max_iters) out[h] = -1;
        return;
    }
    const float4 *P = pts + offsets[pair];
    float hf[8];
    const bool valid = h < max_iters && ransac_hypothesis(P, (uint32_t)count, seed, (uint32_t)h, hf);
    int n = 0;
    for (int base = 0; base < count; base += RANSAC_TILE) {
        const int len = min(RANSAC_TILE, count - base);
        __syncthreads();                            // the previous tile has been read
        for (int i = threadIdx.x; i < len; i += RANSAC_BLOCK) tile[i] = P[base + i];
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < len; ++i) n += ransac_inlier(hf, tile[i], t2) ? 1 : 0;
    }
    if (h < max_iters) out[h] = valid ? n : -1;
}

// Sum of K doubles over the block in a fixed order: a butterfly in each wave (lane 0's value),
// then waves 0..3 in order.  The result lands in out[0..K) (LDS) for every thread.
template <int K>
__device__ __forceinline__ void ransac_block_sum(double (&v)[K], double *red, double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) red[wave * K + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        const int k = threadIdx.x;
        out[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
    }
    __syncthreads();
}

// index of entry (i, j), i <= j, of the upper triangle of a 9 x 9 matrix, row by row
__host__ __device__ constexpr int ransac_tri(int i, int j) { return i * 9 - i * (i - 1) / 2 + (j - i); }

// Smallest eigenvector of the symmetric a[9][9] (LDS), cyclic Jacobi on one lane; v: LDS [9][9].
__device__ void ransac_jacobi(double *a, double *v, double (&out)[9]) {
    for (int i = 0; i < 81; ++i) v[i] = (i % 10 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 9; ++p) {
            diag += a[p * 10] * a[p * 10];
            for (int q = p + 1; q < 9; ++q) off += a[p * 9 + q] * a[p * 9 + q];
        }
        if (!(off > 1e-32 * diag)) break;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = a[p * 9 + q];
                if (apq == 0.0) continue;
                const double theta = (a[q * 10] - a[p * 10]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 9; ++k) {
                    const double akp = a[k * 9 + p], akq = a[k * 9 + q];
                    a[k * 9 + p] = c * akp - s * akq;
                    a[k * 9 + q] = s * akp + c * akq;
                }
                for (int k = 0; k < 9; ++k) {
                    const double apk = a[p * 9 + k], aqk = a[q * 9 + k];
                    a[p * 9 + k] = c * apk - s * aqk;
                    a[q * 9 + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 9; ++k) {
                    const double vkp = v[k * 9 + p], vkq = v[k * 9 + q];
                    v[k * 9 + p] = c * vkp - s * vkq;
                    v[k * 9 + q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int i = 1; i < 9; ++i)
        if (a[i * 10] < a[m * 10]) m = i;
    for (int i = 0; i < 9; ++i) out[i] = v[i * 9 + m];
}

__global__ __launch_bounds__(RANSAC_BLOCK) void ransac_finish_kernel(
    const float4 *__restrict__ pts, const int32_t *__restrict__ offsets,
    const int32_t *__restrict__ counts, int max_iters, float t2, uint64_t seed,
    const int32_t *__restrict__ scores, double *__restrict__ hom, uint8_t *__restrict__ mask,
    int32_t *__restrict__ n_inliers) {
    __shared__ double red[4 * 45];
    __shared__ double sums[45];
    __shared__ double jac_a[81], jac_v[81];
    __shared__ double res[9];
    __shared__ int arg_s[4], arg_h[4], failed;
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = counts[pair];
    const float4 *P = pts + offsets[pair];
    uint8_t *M = mask + offsets[pair];
    // the best hypothesis: most inliers, the lowest index of a tie
    int best = -2, bh = 0x7fffffff;
    if (count >= 4)
        for (int h = tid; h < max_iters; h += RANSAC_BLOCK) {
            const int s = scores[(size_t)pair * max_iters + h];
            if (s > best) best = s, bh = h;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o), oh = __shfl_xor(bh, o);
        if (ob > best || (ob == best && oh < bh)) best = ob, bh = oh;
    }
    if (lane == 0) arg_s[wave] = best, arg_h[wave] = bh;
    __syncthreads();
    best = arg_s[0], bh = arg_h[0];
    for (int w = 1; w < 4; ++w)
        if (arg_s[w] > best || (arg_s[w] == best && arg_h[w] < bh)) best = arg_s[w], bh = arg_h[w];
    bool fail = count < 4 || best < 4;              // uniform
    float hf[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (!fail) fail = !ransac_hypothesis(P, (uint32_t)count, seed, (uint32_t)bh, hf);
    if (!fail) {
        // Hartley normalisation: centroids, then the mean distances to them
        double c4[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < count; i += RANSAC_BLOCK) {
            const float4 q = P[i];
            if (ransac_inlier(hf, q, t2)) c4[0] += q.x, c4[1] += q.y, c4[2] += q.z, c4[3] += q.w;
        }
        ransac_block_sum<4>(c4, red, sums);
        const double n = (double)best;
        const double cx = sums[0] / n, cy = sums[1] / n, cu = sums[2] / n, cv = sums[3] / n;
        __syncthreads();
        double d2[2] = {0.0, 0.0};
        for (int i = tid; i < count; i += RANSAC_BLOCK) {
            const float4 q = P[i];
            if (ransac_inlier(hf, q, t2)) {
                const double ax = q.x - cx, ay = q.y - cy, bx = q.z - cu, by = q.w - cv;
                d2[0] += sqrt(ax * ax + ay * ay);
                d2[1] += sqrt(bx * bx + by * by);
            }
        }
        ransac_block_sum<2>(d2, red, sums);
        const double s1 = sqrt(2.0) / (sums[0] / n), s2 = sqrt(2.0) / (sums[1] / n);
        __syncthreads();
        // the normal matrix of the normalised DLT (upper triangle)
        double m45[45];
#pragma unroll
        for (int k = 0; k < 45; ++k) m45[k] = 0.0;
        for (int i = tid; i < count; i += RANSAC_BLOCK) {
            const float4 q = P[i];
            if (!ransac_inlier(hf, q, t2)) continue;
            const double x = (q.x - cx) * s1, y = (q.y - cy) * s1;
            const double u = (q.z - cu) * s2, v = (q.w - cv) * s2;
            const double a1[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y), -u};
            const double a2[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y), -v};
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
                for (int c = r; c < 9; ++c) m45[ransac_tri(r, c)] += a1[r] * a1[c] + a2[r] * a2[c];
        }
        ransac_block_sum<45>(m45, red, sums);
        if (tid == 0) {
            for (int r = 0; r < 9; ++r)
                for (int c = 0; c < 9; ++c)
                    jac_a[r * 9 + c] = sums[r <= c ? ransac_tri(r, c) : ransac_tri(c, r)];
            double e[9];
            ransac_jacobi(jac_a, jac_v, e);
            // H = T2^-1 Hn T1
            double B[9], H[9];
            for (int r = 0; r < 3; ++r) {
                B[r * 3 + 0] = e[r * 3 + 0] * s1;
                B[r * 3 + 1] = e[r * 3 + 1] * s1;
                B[r * 3 + 2] = (e[r * 3 + 2] - e[r * 3 + 0] * (s1 * cx)) - e[r * 3 + 1] * (s1 * cy);
            }
            for (int c = 0; c < 3; ++c) {
                H[c] = B[c] / s2 + cu * B[6 + c];
                H[3 + c] = B[3 + c] / s2 + cv * B[6 + c];
                H[6 + c] = B[6 + c];
            }
            bool ok = H[8] != 0.0;
            for (int k = 0; k < 9; ++k) {
                res[k] = H[k] / H[8];
                ok = ok && isfinite(res[k]);
            }
            res[8] = 1.0;
            failed = ok ? 0 : 1;
        }
        __syncthreads();
        fail = failed != 0;
    }
    for (int i = tid; i < count; i += RANSAC_BLOCK)
        M[i] = (!fail && ransac_inlier(hf, P[i], t2)) ? 1 : 0;
    if (tid < 9) hom[(size_t)pair * 9 + tid] = fail ? 0.0 : res[tid];
    if (tid == 0) n_inliers[pair] = fail ? 0 : best;
}

extern "C" size_t pano_hom_ransac_work_bytes(int n_pairs, int max_iters) {
    if (n_pairs < 0 || max_iters < 1) return 0;
    return (size_t)n_pairs * (size_t)max_iters * sizeof(int32_t) + 256;
}

extern "C" int pano_hom_ransac(pano_ctx *ctx, const float *pts, const int32_t *offsets,
                               const int32_t *counts, int n_pairs, int max_iters, float thresh,
                               uint64_t seed, void *work, double *hom, uint8_t *mask,
                               int32_t *n_inliers, int32_t *hyp_inliers) {
    PANO_ENTER(ctx, "pano_hom_ransac");
    PANO_REQUIRE(n_pairs >= 0 && n_pairs <= 65535, "pano_hom_ransac: %d pairs (at most 65535)",
                 n_pairs);
    PANO_REQUIRE(max_iters >= 1 && max_iters <= RANSAC_MAX_ITERS,
                 "pano_hom_ransac: max_iters %d (1 .. %d)", max_iters, RANSAC_MAX_ITERS);
    PANO_REQUIRE(thresh >= 0.0f && thresh < INFINITY, "pano_hom_ransac: threshold %g",
                 (double)thresh);
    if (n_pairs == 0) return PANO_OK;
    PANO_REQUIRE(pts && offsets && counts && hom && mask && n_inliers && (work || hyp_inliers),
                 "pano_hom_ransac: null pointer");
    PANO_REQUIRE(((uintptr_t)pts & 15) == 0, "pano_hom_ransac: pts not 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const float t2 = (float)((double)thresh * (double)thresh);
    int32_t *scores = hyp_inliers ? hyp_inliers : (int32_t *)work;
    const float4 *P = (const float4 *)pts;
    PANO_TIMED(PK_RANSAC_SCORE, s,
               hipLaunchKernelGGL(ransac_score_kernel,
                                  dim3(ceil_div(max_iters, RANSAC_BLOCK), n_pairs), dim3(RANSAC_BLOCK),
                                  0, s, P, offsets, counts, max_iters, t2, seed, scores));
    PANO_LAUNCH_CHECK("ransac_score_kernel");
    PANO_TIMED(PK_RANSAC_FINISH, s,
               hipLaunchKernelGGL(ransac_finish_kernel, dim3(n_pairs), dim3(RANSAC_BLOCK), 0, s, P,
                                  offsets, counts, max_iters, t2, seed, scores, hom, mask, n_inliers));
    PANO_LAUNCH_CHECK("ransac_finish_kernel");
    return PANO_OK;
}

// ---- the ratio test and the stable compaction of one pair ---------------------------------------
// 1024 threads walk the queries in chunks; a wave ballot and the 16 wave counts (LDS) give every
// survivor its place, so the survivors keep the ascending query order.
__global__ __launch_bounds__(PACK_BLOCK) void match_pack_kernel(
    const int32_t *__restrict__ idx, const float2 *__restrict__ dist, int nq, double ratio,
    const float2 *__restrict__ kq, const float2 *__restrict__ kt, int nt, float4 *__restrict__ pts,
    int32_t *__restrict__ match, int32_t *__restrict__ count) {
    __shared__ int wave_n[PACK_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int done = 0;
    for (int base = 0; base < nq; base += PACK_BLOCK) {
        const int q = base + tid;
        int t = -1;
        bool keep = false;
        if (q < nq) {
            const float2 d = dist[q];
            t = idx[2 * q];
            keep = (double)d.x < ratio * (double)d.y && t >= 0 && t < nt;
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_n[wave] = __popcll(bal);
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PACK_BLOCK / 64; ++w) {
            const int c = wave_n[w];
            woff += w < wave ? c : 0;
            total += c;
        }
        if (keep) {
            const int o = done + woff + before;
            const float2 a = kq[q], b = kt[t];
            pts[o] = make_float4(a.x, a.y, b.x, b.y);
            match[2 * o] = q;
            match[2 * o + 1] = t;
        }
        done += total;
        __syncthreads();                            // wave_n is rewritten by the next chunk
    }
    if (tid == 0) *count = done;
}

extern "C" int pano_match_pack(pano_ctx *ctx, const int32_t *idx, const float *dist, int nq,
                               double ratio, const float *kp_query, const float *kp_train, int nt,
                               float *pts, int32_t *match, int32_t *count) {
    PANO_ENTER(ctx, "pano_match_pack");
    PANO_REQUIRE(count, "pano_match_pack: null count");
    PANO_REQUIRE(nq >= 0 && nt >= 0, "pano_match_pack: %d queries, %d train rows", nq, nt);
    PANO_REQUIRE(nq == 0 || (idx && dist && kp_query && kp_train && pts && match),
                 "pano_match_pack: null pointer");
    PANO_REQUIRE(((uintptr_t)pts & 15) == 0 && ((uintptr_t)dist & 7) == 0 &&
                     ((uintptr_t)kp_query & 7) == 0 && ((uintptr_t)kp_train & 7) == 0,
                 "pano_match_pack: misaligned buffer");
    const hipStream_t s = (hipStream_t)stream;
    PANO_TIMED(PK_MATCH_PACK, s,
               hipLaunchKernelGGL(match_pack_kernel, dim3(1), dim3(PACK_BLOCK), 0, s, idx,
                                  (const float2 *)dist, nq, ratio, (const float2 *)kp_query,
                                  (const float2 *)kp_train, nt, (float4 *)pts, match, count));
    PANO_LAUNCH_CHECK("match_pack_kernel");
    return PANO_OK;
}
