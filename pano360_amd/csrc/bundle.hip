// Bundle adjustment's per-match work: the per-pair sums of squared residuals
// (pano_ba_residuals) and the damped normal equations (pano_ba_normal) that the
// Levenberg-Marquardt loop of bundle_adj.py:311-345 solves.  The contract (layouts, the
// reference lines each step restates, the summation structure) is in include/pano360.h; the
// host derives every 3 x 3 table in NumPy and this file only forms sums of products in f64.
//
// Pair kernels: one block of BA_BLOCK lanes per pair, one lane per match.  The block walks the
// pair's rows in chunks of BA_BLOCK; per chunk every lane forms its match's terms in registers
// (12 Jacobian columns x 2 rows and the 2 residuals), each term is summed over the wave by a
// fixed xor butterfly and lane 0 adds the wave's sum to its own LDS row.  At the end the waves'
// rows are added in wave order.  The assembly kernel then adds the pairs' sums into the dense
// system in pair order.  Every sum has a fixed order: the same input gives the same bits.
#include "common.h"
#include "wave.h"

#define BA_BLOCK 256
#define BA_WAVES (BA_BLOCK / 64)
#define BA_TERMS 90          // 21 + 21 + 36 + 12 per pair (include/pano360.h)
#define BA_TABLE 90          // doubles per pair in the Jacobian table: ten 3 x 3 matrices
#define ASM_BLOCK 64

// M p with p = (x, y, 1), left to right as NumPy's dot: (m0 x + m1 y) + m2
__device__ __forceinline__ void ba_mul_p(const double *__restrict__ M, double x, double y,
                                         double (&o)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (M[3 * r] * x + M[3 * r + 1] * y) + M[3 * r + 2];
}

// M v for a general 3-vector
__device__ __forceinline__ void ba_mul(const double *__restrict__ M, const double (&v)[3],
                                       double (&o)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2];
}

// ---- per pair: sum of squared residuals at one camera state (bundle_adj.py:145-149) -----------
__global__ __launch_bounds__(BA_BLOCK) void ba_residual_kernel(const double *__restrict__ rows,
                                                               const int32_t *__restrict__ pairs,
                                                               const double *__restrict__ hom,
                                                               double *__restrict__ ssq) {
    __shared__ double wave_part[BA_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = pairs[4 * p + 2], count = pairs[4 * p + 3];
    const double *H = hom + 9 * (size_t)p;
    double acc = 0.0;
    for (int m = tid; m < count; m += BA_BLOCK) {
        const double *row = rows + 4 * ((size_t)first + m);
        double t[3];
        ba_mul_p(H, row[2], row[3], t);
        const double rx = row[0] - t[0] / t[2], ry = row[1] - t[1] / t[2];
        acc += rx * rx + ry * ry;
    }
    acc = wave_sum(acc);
    if (lane == 0) wave_part[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = wave_part[0];
#pragma unroll
        for (int w = 1; w < BA_WAVES; ++w) s += wave_part[w];
        ssq[p] = s;
    }
}

// ---- per pair: the 90 sums of the Jacobian's blocks (bundle_adj.py:199-256) -------------------
__global__ __launch_bounds__(BA_BLOCK) void ba_pair_kernel(const double *__restrict__ rows,
                                                           const int32_t *__restrict__ pairs,
                                                           const double *__restrict__ jtab,
                                                           const double *__restrict__ hom_r,
                                                           double *__restrict__ sums) {
    __shared__ double acc[BA_WAVES][BA_TERMS];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = pairs[4 * p + 2], count = pairs[4 * p + 3];
    const double *T = jtab + BA_TABLE * (size_t)p;
    const double *Hj = T, *Sb = T + 9, *Sr = T + 18, *Kai = T + 27, *N = T + 36, *Q = T + 63;
    const double *Hr = hom_r + 9 * (size_t)p;
    for (int k = tid; k < BA_WAVES * BA_TERMS; k += BA_BLOCK) (&acc[0][0])[k] = 0.0;
    __syncthreads();

    for (int base = 0; base < count; base += BA_BLOCK) {
        const int m = base + tid;
        double jx[12], jy[12], rx = 0.0, ry = 0.0;
#pragma unroll
        for (int c = 0; c < 12; ++c) jx[c] = jy[c] = 0.0;
        if (m < count) {
            const double *row = rows + 4 * ((size_t)first + m);
            const double xb = row[0], yb = row[1], xa = row[2], ya = row[3];
            double h[3], s[3], t[3], q[3], w[3];
            // dpdh at the Jacobian's state (:208-210)
            ba_mul_p(Hj, xa, ya, h);
            const double iz = 1.0 / h[2];
            const double d0 = h[0] * iz * iz, d1 = h[1] * iz * iz, d2 = -iz;
            // camera b: focal, ppx, ppy through the dK tables (:219-224)
            ba_mul_p(Sb, xa, ya, s);
            jx[0] = s[0] * d2 + 0.0 * d0, jy[0] = s[1] * d2 + 0.0 * d1;
            jx[1] = s[2] * d2 + 0.0 * d0, jy[1] = 0.0 * d2 + 0.0 * d1;
            jx[2] = 0.0 * d2 + 0.0 * d0, jy[2] = s[2] * d2 + 0.0 * d1;
            // camera b: rotation (:226-230)
            ba_mul_p(Sr, xa, ya, t);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ba_mul(N + 9 * k, t, w);
                jx[3 + k] = w[0] * d2 + w[2] * d0, jy[3 + k] = w[1] * d2 + w[2] * d1;
            }
            // camera a: focal, ppx, ppy: hom dK (-K_a^-1 p) (:233-238)
            ba_mul_p(Kai, xa, ya, q);
            const double n0 = -q[0], n1 = -q[1], n2 = -q[2];
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = (Hj[3 * r] * n0 + Hj[3 * r + 1] * n1) + 0.0 * n2;
            jx[6] = w[0] * d2 + w[2] * d0, jy[6] = w[1] * d2 + w[2] * d1;
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = (0.0 * n0 + 0.0 * n1) + Hj[3 * r] * n2;
            jx[7] = w[0] * d2 + w[2] * d0, jy[7] = w[1] * d2 + w[2] * d1;
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = (0.0 * n0 + 0.0 * n1) + Hj[3 * r + 1] * n2;
            jx[8] = w[0] * d2 + w[2] * d0, jy[8] = w[1] * d2 + w[2] * d1;
            // camera a: rotation (:240-243)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ba_mul(Q + 9 * k, q, w);
                jx[9 + k] = w[0] * d2 + w[2] * d0, jy[9 + k] = w[1] * d2 + w[2] * d1;
            }
            // the residual at the residual's state (get_diff, :145-149)
            ba_mul_p(Hr, xa, ya, h);
            rx = xb - h[0] / h[2], ry = yb - h[1] / h[2];
        }
        int k = 0;
#define BA_PUT(value)                                 \
    do {                                              \
        const double v_ = wave_sum(value);            \
        if (lane == 0) acc[wave][k] += v_;            \
        ++k;                                          \
    } while (0)
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = u; v < 6; ++v) BA_PUT(jx[u] * jx[v] + jy[u] * jy[v]);
#pragma unroll
        for (int u = 6; u < 12; ++u)
#pragma unroll
            for (int v = u; v < 12; ++v) BA_PUT(jx[u] * jx[v] + jy[u] * jy[v]);
#pragma unroll
        for (int u = 0; u < 6; ++u)
#pragma unroll
            for (int v = 6; v < 12; ++v) BA_PUT(jx[u] * jx[v] + jy[u] * jy[v]);
#pragma unroll
        for (int c = 0; c < 12; ++c) BA_PUT(jx[c] * rx + jy[c] * ry);
#undef BA_PUT
    }
    __syncthreads();
    if (tid < BA_TERMS) {
        double s = acc[0][tid];
#pragma unroll
        for (int w = 1; w < BA_WAVES; ++w) s += acc[w][tid];
        sums[BA_TERMS * (size_t)p + tid] = s;
    }
}

// index of (u, v), u <= v < 6, in a row-major upper triangle
__device__ __forceinline__ int ba_tri(int u, int v) {
    if (u > v) { const int t = u; u = v; v = t; }
    return u * 6 - u * (u - 1) / 2 + (v - u);
}

// ---- the dense system: block (sr, sc) of 6 x 6, the pairs added in pair order (:245-256, :323-324)
__global__ __launch_bounds__(ASM_BLOCK) void ba_assemble_kernel(
    const int32_t *__restrict__ pairs, int n_pairs, const int32_t *__restrict__ slot,
    int n_active, double lambda, const double *__restrict__ sums, double *__restrict__ jtj,
    double *__restrict__ jtr) {
    const int sr = blockIdx.x, sc = blockIdx.y, tid = threadIdx.x;
    const int n = 6 * n_active;
    if (tid < 36) {
        const int u = tid / 6, v = tid % 6;
        double s = 0.0;
        for (int p = 0; p < n_pairs; ++p) {
            const int ia = slot[pairs[4 * p]], ib = slot[pairs[4 * p + 1]];
            const double *S = sums + BA_TERMS * (size_t)p;
            if (sr == sc) {
                if (ib == sr) s += S[ba_tri(u, v)];
                else if (ia == sr) s += S[21 + ba_tri(u, v)];
            } else if (ib == sr && ia == sc) {
                s += S[42 + 6 * u + v];
            } else if (ia == sr && ib == sc) {
                s += S[42 + 6 * v + u];
            }
        }
        if (sr == sc && u == v) s += lambda;
        jtj[(size_t)(6 * sr + u) * n + 6 * sc + v] = s;
    } else if (sr == sc && tid < 42) {
        const int u = tid - 36;
        double s = 0.0;
        for (int p = 0; p < n_pairs; ++p) {
            const int ia = slot[pairs[4 * p]], ib = slot[pairs[4 * p + 1]];
            const double *S = sums + BA_TERMS * (size_t)p;
            if (ib == sr) s += S[78 + u];
            else if (ia == sr) s += S[84 + u];
        }
        jtr[6 * sr + u] = s;
    }
}

extern "C" size_t pano_ba_work_bytes(int n_pairs) {
    if (n_pairs < 0) return 0;
    return (size_t)n_pairs * BA_TERMS * sizeof(double) + 256;
}

extern "C" int pano_ba_residuals(pano_ctx *ctx, const double *rows, const int32_t *pairs,
                                 int n_pairs, const double *hom, double *ssq) {
    PANO_ENTER(ctx, "pano_ba_residuals");
    PANO_REQUIRE(n_pairs >= 0 && n_pairs <= (1 << 30), "pano_ba_residuals: %d pairs", n_pairs);
    if (n_pairs == 0) return PANO_OK;
    PANO_REQUIRE(rows && pairs && hom && ssq, "pano_ba_residuals: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    PANO_TIMED(PK_BA_RESIDUAL, s,
               hipLaunchKernelGGL(ba_residual_kernel, dim3(n_pairs), dim3(BA_BLOCK), 0, s, rows,
                                  pairs, hom, ssq));
    PANO_LAUNCH_CHECK("ba_residual_kernel");
    return PANO_OK;
}

extern "C" int pano_ba_normal(pano_ctx *ctx, const double *rows, const int32_t *pairs, int n_pairs,
                              const int32_t *slot, int n_active, const double *jtab,
                              const double *hom_r, double lambda, void *work, double *jtj,
                              double *jtr) {
    PANO_ENTER(ctx, "pano_ba_normal");
    PANO_REQUIRE(n_pairs >= 0 && n_pairs <= (1 << 30), "pano_ba_normal: %d pairs", n_pairs);
    PANO_REQUIRE(n_active >= 1 && n_active <= 65535, "pano_ba_normal: %d active cameras",
                 n_active);
    PANO_REQUIRE(slot && jtj && jtr && (n_pairs == 0 || (rows && pairs && jtab && hom_r && work)),
                 "pano_ba_normal: null pointer");
    const hipStream_t s = (hipStream_t)stream;
    double *sums = (double *)work;
    if (n_pairs > 0) {
        PANO_TIMED(PK_BA_PAIRS, s,
                   hipLaunchKernelGGL(ba_pair_kernel, dim3(n_pairs), dim3(BA_BLOCK), 0, s, rows,
                                      pairs, jtab, hom_r, sums));
        PANO_LAUNCH_CHECK("ba_pair_kernel");
    }
    PANO_TIMED(PK_BA_ASSEMBLE, s,
               hipLaunchKernelGGL(ba_assemble_kernel, dim3(n_active, n_active), dim3(ASM_BLOCK), 0,
                                  s, pairs, n_pairs, slot, n_active, lambda, sums, jtj, jtr));
    PANO_LAUNCH_CHECK("ba_assemble_kernel");
    return PANO_OK;
}
