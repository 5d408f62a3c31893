// The robust refinement behind bundle_adj.refine: per pair of cameras the Huber-weighted normal
// equations of the reprojection error under a shared radial distortion (k1, k2), with the TRUE
// derivative of the residual (pano_ba_refine; the contract, the Jacobian written out and the
// summation order are in include/pano360.h).  One block of RF_BLOCK threads per pair: thread t
// takes the pair's matches t, t + 256, ... in order and keeps the 70 sums of its matches in
// registers; block_sum_fixed<70> (wave.h) then combines the threads in its one fixed order.  All
// arithmetic is f64 with one rounding per operation; sqrt is the only function called.
#include "common.h"
#include "wave.h"

#define RF_BLOCK 256
#define RF_TERMS 70          // 55 + 10 + 5 per pair (include/pano360.h)
#define RF_PARAMS 10
#define RF_NEWTON 10

// One observation (x, y) of a camera (f, px, py): d = the distorted normalised point, u = the
// undistorted one, ihp = 1 / h'(r) at the Newton solution r, sr2 = s r^2 (what the derivatives by
// k1 and k2 are made from: du/dk1 = -(s r^2) d / h', du/dk2 = -(s r^2) r^2 d / h').  Returns
// false when an h' met on the way (the ten steps' and the solution's) is not positive.
__device__ __forceinline__ bool rf_undist(const double *__restrict__ cam, double x, double y,
                                          double k1, double k2, double (&d)[2], double (&u)[2],
                                          double &ihp, double &sr2, double &r2) {
    const double f = cam[0];
    d[0] = (x - cam[1]) / f, d[1] = (y - cam[2]) / f;
    const double rd = sqrt(d[0] * d[0] + d[1] * d[1]);
    double r = rd;
    bool ok = true;
#pragma unroll 1
    for (int it = 0; it < RF_NEWTON; ++it) {
        const double q = r * r, q2 = q * q;
        const double h = r * ((1.0 + k1 * q) + k2 * q2);
        const double hp = (1.0 + (3.0 * k1) * q) + (5.0 * k2) * q2;
        ok = ok && hp > 0.0;
        r = r - (h - rd) / hp;
    }
    r2 = r * r;
    const double hp = (1.0 + (3.0 * k1) * r2) + (5.0 * k2) * (r2 * r2);
    ok = ok && hp > 0.0;
    ihp = 1.0 / hp;
    const double s = rd > 0.0 ? r / rd : 1.0;
    u[0] = s * d[0], u[1] = s * d[1];
    sr2 = s * r2;
    return ok;
}

// R_b (R_a^T w): (m0 w0 + m1 w1) + m2 w2 per row, R_a^T read down R_a's columns
__device__ __forceinline__ void rf_rot(const double *__restrict__ Ra, const double *__restrict__ Rb,
                                       double w0, double w1, double w2, double (&o)[3]) {
    double t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = (Ra[r] * w0 + Ra[3 + r] * w1) + Ra[6 + r] * w2;
#pragma unroll
    for (int r = 0; r < 3; ++r)
        o[r] = (Rb[3 * r] * t[0] + Rb[3 * r + 1] * t[1]) + Rb[3 * r + 2] * t[2];
}

__global__ __launch_bounds__(RF_BLOCK) void ba_refine_kernel(
    const double *__restrict__ rows, long long n_rows, const int32_t *__restrict__ pairs,
    const double *__restrict__ cams, int n_cameras, double k1, double k2, double delta,
    double *__restrict__ out) {
    __shared__ double part[RF_BLOCK / 64][RF_TERMS];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int a = pairs[4 * p], b = pairs[4 * p + 1];
    const int first = pairs[4 * p + 2], count = pairs[4 * p + 3];
    // a pair that names a camera or a row outside the tables reads nothing: its matches are invalid
    const bool inside = a >= 0 && a < n_cameras && b >= 0 && b < n_cameras && first >= 0 &&
                        count >= 0 && (long long)first + count <= n_rows;
    const double *ca = cams + 12 * (size_t)(inside ? a : 0);
    const double *cb = cams + 12 * (size_t)(inside ? b : 0);
    const double *Ra = ca + 3, *Rb = cb + 3;
    const double fb = cb[0], ifa = 1.0 / ca[0];

    double acc[RF_TERMS];
#pragma unroll
    for (int k = 0; k < RF_TERMS; ++k) acc[k] = 0.0;

    for (int m = tid; m < count; m += RF_BLOCK) {
        if (!inside) {
            acc[67] += 1.0;
            continue;
        }
        const double *row = rows + 4 * ((size_t)first + m);
        double db[2], ub[2], da[2], ua[2], ihb, iha, sb2, sa2, rb2, ra2;
        bool ok = rf_undist(cb, row[0], row[1], k1, k2, db, ub, ihb, sb2, rb2);
        ok = rf_undist(ca, row[2], row[3], k1, k2, da, ua, iha, sa2, ra2) && ok;
        double v[3], w[3];
        rf_rot(Ra, Rb, ua[0], ua[1], 1.0, v);
        ok = ok && v[2] > 0.0;
        const double iz = 1.0 / v[2];
        const double p0 = v[0] * iz, p1 = v[1] * iz;
        const double g = fb * iz;       // -f_b Dpi w = (-(w0 - p0 w2) g, -(w1 - p1 w2) g)
        const double ex = fb * (ub[0] - p0), ey = fb * (ub[1] - p1);

        double jx[RF_PARAMS], jy[RF_PARAMS];
        // camera b, f: (u_b - pi(v)) - d_b / h'_b
        jx[0] = (ub[0] - p0) - db[0] * ihb, jy[0] = (ub[1] - p1) - db[1] * ihb;
        // camera b, omega_k: -f_b Dpi (e_k x v)
        jx[1] = (p0 * v[1]) * g, jy[1] = (v[2] + p1 * v[1]) * g;
        jx[2] = -(v[2] + p0 * v[0]) * g, jy[2] = -(p1 * v[0]) * g;
        jx[3] = v[1] * g, jy[3] = -(v[0] * g);
        // camera a, f: -f_b Dpi M (du_a/df_a, 0), du_a/df_a = -d_a / (h'_a f_a)
        const double ca_f = -(iha * ifa);
        rf_rot(Ra, Rb, da[0] * ca_f, da[1] * ca_f, 0.0, w);
        jx[4] = -((w[0] - p0 * w[2]) * g), jy[4] = -((w[1] - p1 * w[2]) * g);
        // camera a, omega_k: +f_b Dpi M (e_k x q), q = (u_a, 1)
        rf_rot(Ra, Rb, 0.0, -1.0, ua[1], w);
        jx[5] = (w[0] - p0 * w[2]) * g, jy[5] = (w[1] - p1 * w[2]) * g;
        rf_rot(Ra, Rb, 1.0, 0.0, -ua[0], w);
        jx[6] = (w[0] - p0 * w[2]) * g, jy[6] = (w[1] - p1 * w[2]) * g;
        rf_rot(Ra, Rb, -ua[1], ua[0], 0.0, w);
        jx[7] = (w[0] - p0 * w[2]) * g, jy[7] = (w[1] - p1 * w[2]) * g;
        // k1, k2: f_b (du_b/dk - Dpi M (du_a/dk, 0)), du/dk1 = -(s r^2) d / h', du/dk2 = r^2 du/dk1
        {
            const double tb = -(sb2 * ihb), ta = -(sa2 * iha);
            rf_rot(Ra, Rb, da[0] * ta, da[1] * ta, 0.0, w);
            jx[8] = fb * (db[0] * tb) - (w[0] - p0 * w[2]) * g;
            jy[8] = fb * (db[1] * tb) - (w[1] - p1 * w[2]) * g;
            const double tb2 = tb * rb2, ta2 = ta * ra2;
            rf_rot(Ra, Rb, da[0] * ta2, da[1] * ta2, 0.0, w);
            jx[9] = fb * (db[0] * tb2) - (w[0] - p0 * w[2]) * g;
            jy[9] = fb * (db[1] * tb2) - (w[1] - p1 * w[2]) * g;
        }

        // finite: the residual and every entry of J
        double mag = fabs(ex) + fabs(ey);
#pragma unroll
        for (int c = 0; c < RF_PARAMS; ++c) mag += fabs(jx[c]) + fabs(jy[c]);
        ok = ok && mag <= 1.7976931348623157e308;
        if (!ok) {
            acc[67] += 1.0;
            continue;
        }
        const double n2 = ex * ex + ey * ey, n = sqrt(n2);
        const bool in = n <= delta;
        const double wt = in ? 1.0 : delta / n;
        int k = 0;
#pragma unroll
        for (int c = 0; c < RF_PARAMS; ++c) {
            const double wx = wt * jx[c], wy = wt * jy[c];
#pragma unroll
            for (int e = c; e < RF_PARAMS; ++e) acc[k++] += wx * jx[e] + wy * jy[e];
        }
#pragma unroll
        for (int c = 0; c < RF_PARAMS; ++c) acc[55 + c] += (wt * jx[c]) * ex + (wt * jy[c]) * ey;
        acc[65] += in ? n2 * 0.5 : delta * (n - delta * 0.5);
        acc[66] += wt;
        acc[68] += in ? n2 : 0.0;
        acc[69] += in ? 1.0 : 0.0;
    }
    const double s = block_sum_fixed<RF_TERMS>(acc, part, tid & 63, tid >> 6);
    if (tid < RF_TERMS) out[RF_TERMS * (size_t)p + tid] = s;
}

extern "C" int pano_ba_refine(pano_ctx *ctx, const double *rows, int64_t n_rows,
                              const int32_t *pairs, int n_pairs, const double *cams, int n_cameras,
                              double k1, double k2, double delta, double *out) {
    PANO_ENTER(ctx, "pano_ba_refine");
    PANO_REQUIRE(rows && pairs && cams && out, "pano_ba_refine: null pointer");
    PANO_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 30), "pano_ba_refine: %d pairs", n_pairs);
    PANO_REQUIRE(n_cameras >= 1, "pano_ba_refine: %d cameras", n_cameras);
    PANO_REQUIRE(n_rows >= 0, "pano_ba_refine: %lld rows", (long long)n_rows);
    PANO_REQUIRE(delta > 0.0 && delta <= 1.7976931348623157e308, "pano_ba_refine: delta %g",
                 delta);
    const hipStream_t s = (hipStream_t)stream;
    PANO_TIMED(PK_BA_REFINE, s,
               hipLaunchKernelGGL(ba_refine_kernel, dim3(n_pairs), dim3(RF_BLOCK), 0, s, rows,
                                  (long long)n_rows, pairs, cams, n_cameras, k1, k2, delta, out));
    PANO_LAUNCH_CHECK("ba_refine_kernel");
    return PANO_OK;
}
