// Views of a finished mosaic (pano_mip_u8, pano_view_render): the mip chain of a uint8 mosaic and
// a renderer that turns every output pixel of a batch of views - rectilinear, equirectangular,
// stereographic - into a direction, the direction into mosaic coordinates and a footprint, and
// samples the chain trilinearly.  The contract is in include/pano360.h, the host side is
// pano360_amd/view.py and a float64 NumPy statement of the arithmetic is tests/view_model.py.
#include <math.h>

#include "batch.h"

#define MIP_BLOCK 256
#define MIP_MAX_GROUPS 4096         // grid cap of the mip kernel (it loops beyond it)
#define VIEW_TX 32                  // output pixels of a workgroup: 32 x 8, a wave is 32 x 2
#define VIEW_TY 8

// ---- 1. the mip chain -------------------------------------------------------------------------------
// level l has ((H - 1) >> l) + 1 rows: halving and rounding up l times
__host__ __device__ static inline int mip_side(int side, int l) { return ((side - 1) >> l) + 1; }

static int mip_count(int h, int w) {
    int n = 1;
    while (n < PANO_VIEW_MAX_LEVELS && (mip_side(h, n - 1) > 1 || mip_side(w, n - 1) > 1)) ++n;
    return n;
}

// One thread per pixel of the destination level: (a + b + c + d + 2) >> 2 over its 2 x 2 block of
// the source level, the odd index clamped to the last row or column.
__global__ __launch_bounds__(MIP_BLOCK) void mip_u8_kernel(const uint8_t *__restrict__ src, int sh,
                                                           int sw, uint8_t *__restrict__ dst) {
    const int dh = (sh + 1) >> 1, dw = (sw + 1) >> 1;
    const int64_t n = (int64_t)dh * dw;
    for (int64_t i = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * MIP_BLOCK) {
        const int y = (int)(i / dw), x = (int)(i - (int64_t)y * dw);
        const int y0 = 2 * y, x0 = 2 * x;
        const int y1 = min(y0 + 1, sh - 1), x1 = min(x0 + 1, sw - 1);
        const uint8_t *a = src + ((int64_t)y0 * sw + x0) * 3, *b = src + ((int64_t)y0 * sw + x1) * 3;
        const uint8_t *c = src + ((int64_t)y1 * sw + x0) * 3, *d = src + ((int64_t)y1 * sw + x1) * 3;
        for (int k = 0; k < 3; ++k) dst[i * 3 + k] = (uint8_t)((a[k] + b[k] + c[k] + d[k] + 2) >> 2);
    }
}

// the chain's levels lie inside the buffer, in order, without overlap
static int mip_table_check(const char *who, int h, int w, const int64_t *offsets, int n_levels) {
    PANO_REQUIRE(h >= 1 && w >= 1 && h <= PANO_VIEW_MAX_SIDE && w <= PANO_VIEW_MAX_SIDE,
                 "%s: a mosaic of %d x %d (sides 1 .. %d)", who, w, h, PANO_VIEW_MAX_SIDE);
    PANO_REQUIRE(offsets && n_levels == mip_count(h, w), "%s: %d levels for %d x %d, the chain has %d",
                 who, n_levels, w, h, mip_count(h, w));
    PANO_REQUIRE(offsets[0] >= 0, "%s: negative offset", who);
    for (int l = 0; l < n_levels; ++l)
        PANO_REQUIRE(offsets[l + 1] >= offsets[l] + 3 * (int64_t)mip_side(h, l) * mip_side(w, l),
                     "%s: level %d overlaps the next", who, l);
    return PANO_OK;
}

extern "C" int pano_mip_u8(pano_ctx *ctx, const uint8_t *img, int h, int w, int64_t pitch,
                           uint8_t *mips, const int64_t *offsets, int n_levels) {
    PANO_ENTER(ctx, "pano_mip_u8");
    PANO_REQUIRE(img && mips, "pano_mip_u8: null pointer");
    if (int rc = mip_table_check("pano_mip_u8", h, w, offsets, n_levels)) return rc;
    PANO_REQUIRE(pitch >= 3 * (int64_t)w, "pano_mip_u8: pitch %lld for %d pixels", (long long)pitch, w);
    const hipStream_t s = (hipStream_t)stream;
    PANO_HIP(hipMemcpy2DAsync(mips + offsets[0], 3 * (size_t)w, img, (size_t)pitch, 3 * (size_t)w,
                              (size_t)h, hipMemcpyDeviceToDevice, s));
    for (int l = 0; l + 1 < n_levels; ++l) {
        const int sh = mip_side(h, l), sw = mip_side(w, l);
        const int64_t n = (int64_t)mip_side(h, l + 1) * mip_side(w, l + 1);
        hipLaunchKernelGGL(mip_u8_kernel, capped_grid(ceil_div(n, MIP_BLOCK), MIP_MAX_GROUPS),
                           dim3(MIP_BLOCK), 0, s, mips + offsets[l], sh, sw, mips + offsets[l + 1]);
        PANO_LAUNCH_CHECK("mip_u8_kernel");
    }
    return PANO_OK;
}

// ---- 2. the renderer --------------------------------------------------------------------------------
struct ViewDev {
    float m[9];                     // RECTILINEAR: R K^-1, else R (row-major)
    float p[4];                     // EQUIRECT: a0, sa, b0, sb; STEREOGRAPHIC: cx, cy, f
    uint8_t *image, *mask;
    int kind, w, h;
    TileSlot slot;
};

struct ViewBatch {                  // a launch's arguments, by value: nothing to upload or keep alive
    const uint8_t *mips;
    int64_t off[PANO_VIEW_MAX_LEVELS];
    float low0, low1, res0, res1;
    float period;                   // 2 pi / res0: fx is brought into [0, period)
    float scale;                    // closed: W / period, so that the period is exactly W; else 1
    int h, w, closed, levels, n;
    ViewDev v[PANO_VIEW_MAX_VIEWS];
};
static_assert(sizeof(ViewBatch) <= 4096, "the batch travels as a kernel argument");

// (theta, phi) of output pixel (u, v): its direction by the view's kind, turned by the view's matrix
__device__ __forceinline__ void view_angles(const ViewDev &V, float u, float v, float &theta,
                                            float &phi) {
    float cx, cy, cz;
    if (V.kind == PANO_VIEW_RECTILINEAR) {
        cx = u;
        cy = v;
        cz = 1.0f;
    } else if (V.kind == PANO_VIEW_EQUIRECT) {
        const float th = V.p[0] + u * V.p[1], ph = V.p[2] + v * V.p[3];
        const float c = cosf(ph);
        cx = c * sinf(th);
        cy = sinf(ph);
        cz = c * cosf(th);
    } else {
        const float X = (u - V.p[0]) / V.p[2], Y = (v - V.p[1]) / V.p[2];
        cx = 4.0f * X;
        cy = 4.0f * Y;
        cz = 4.0f - (X * X + Y * Y);
    }
    const float dx = V.m[0] * cx + V.m[1] * cy + V.m[2] * cz;
    const float dy = V.m[3] * cx + V.m[4] * cy + V.m[5] * cz;
    const float dz = V.m[6] * cx + V.m[7] * cy + V.m[8] * cz;
    theta = atan2f(dx, dz);
    phi = atan2f(dy, sqrtf(dx * dx + dz * dz));
}

// length, in mosaic pixels, of the step from (theta, phi) to (t1, p1); the theta difference is
// wrapped into (-pi, pi]
__device__ __forceinline__ float view_step(const ViewBatch &B, float theta, float phi, float t1,
                                           float p1) {
    const float pi = 3.14159265358979323846f;
    float dth = t1 - theta;
    if (dth > pi) dth -= 2.0f * pi;
    if (dth <= -pi) dth += 2.0f * pi;
    const float ax = dth / B.res0 * B.scale, ay = (p1 - phi) / B.res1;
    return sqrtf(ax * ax + ay * ay);
}

// bilinear sample of level l at the level coordinate (f - (2^l - 1) / 2) / 2^l: rows clamped,
// columns clamped (open) or modulo the level's width (closed).  0 <= fx <= W, 0 <= fy <= H - 1.
__device__ __forceinline__ void view_sample(const ViewBatch &B, int l, float fx, float fy,
                                            float out[3]) {
    const int wl = mip_side(B.w, l), hl = mip_side(B.h, l);
    const float size = (float)(1 << l), half = (size - 1.0f) * 0.5f;
    const float cx = (fx - half) / size, cy = (fy - half) / size;
    const float x0f = floorf(cx), y0f = floorf(cy);
    const float ax = cx - x0f, ay = cy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    int xa, xb;
    if (B.closed) {
        xa = x0 % wl;
        if (xa < 0) xa += wl;
        xb = xa + 1 == wl ? 0 : xa + 1;
    } else {
        xa = min(max(x0, 0), wl - 1);
        xb = min(max(x0 + 1, 0), wl - 1);
    }
    const int ya = min(max(y0, 0), hl - 1), yb = min(max(y0 + 1, 0), hl - 1);
    const uint8_t *base = B.mips + B.off[l];
    const uint8_t *p00 = base + ((int64_t)ya * wl + xa) * 3, *p01 = base + ((int64_t)ya * wl + xb) * 3;
    const uint8_t *p10 = base + ((int64_t)yb * wl + xa) * 3, *p11 = base + ((int64_t)yb * wl + xb) * 3;
    for (int k = 0; k < 3; ++k) {
        const float a = p00[k], b = p01[k], c = p10[k], d = p11[k];
        const float top = a + ax * (b - a), bot = c + ax * (d - c);
        out[k] = top + ay * (bot - top);
    }
}

// One thread per output pixel, one workgroup per 32 x 8 tile of one view (found as in batch.h).  The
// footprint comes from the thread's own evaluation of its right and lower neighbours' angles.
__global__ __launch_bounds__(VIEW_TX *VIEW_TY) void view_render_kernel(const ViewBatch B) {
    int tile;
    const ViewDev &V = batch_record(B.v, B.n, tile);
    const int u = (tile % V.slot.tiles_x) * VIEW_TX + (int)threadIdx.x;
    const int v = (tile / V.slot.tiles_x) * VIEW_TY + (int)threadIdx.y;
    if (u >= V.w || v >= V.h) return;

    float theta, phi;
    view_angles(V, (float)u, (float)v, theta, phi);

    float fx = (theta - B.low0) / B.res0;
    fx -= floorf(fx / B.period) * B.period;
    if (fx >= B.period) fx -= B.period;
    if (fx < 0.0f) fx = 0.0f;
    fx *= B.scale;
    const float fy = (phi - B.low1) / B.res1;
    // (written so that a NaN is not covered)
    const bool covered = fy >= 0.0f && fy <= (float)(B.h - 1) && fx >= 0.0f &&
                         (B.closed ? fx <= (float)B.w : fx <= (float)(B.w - 1));

    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if (covered) {                                       // (an uncovered pixel needs no footprint)
        float t1, p1, t2, p2;
        view_angles(V, (float)(u + 1), (float)v, t1, p1);
        view_angles(V, (float)u, (float)(v + 1), t2, p2);
        const float rho = fmaxf(view_step(B, theta, phi, t1, p1), view_step(B, theta, phi, t2, p2));
        float lod = rho > 1.0f ? log2f(rho) : 0.0f;
        lod = fminf(lod, (float)(B.levels - 1));
        const float l0f = floorf(lod), t = lod - l0f;
        const int l0 = (int)l0f;
        view_sample(B, l0, fx, fy, rgb);
        if (t > 0.0f) {                                  // (then l0 + 1 <= levels - 1)
            float up[3];
            view_sample(B, l0 + 1, fx, fy, up);
            for (int k = 0; k < 3; ++k) rgb[k] = rgb[k] + t * (up[k] - rgb[k]);
        }
    }
    const int64_t at = (int64_t)v * V.w + u;
    for (int k = 0; k < 3; ++k)
        V.image[at * 3 + k] = covered ? (uint8_t)fminf(fmaxf(floorf(rgb[k] + 0.5f), 0.0f), 255.0f) : 0;
    V.mask[at] = covered ? 1 : 0;
}

extern "C" int pano_view_render(pano_ctx *ctx, const uint8_t *mips, const int64_t *offsets,
                                int n_levels, const pano_view_mosaic *mosaic,
                                const pano_view *views, int n) {
    PANO_ENTER(ctx, "pano_view_render");
    PANO_REQUIRE(mips && mosaic && views, "pano_view_render: null pointer");
    PANO_REQUIRE(n >= 1 && n <= PANO_VIEW_MAX_VIEWS, "pano_view_render: %d views (1 .. %d)", n,
                 PANO_VIEW_MAX_VIEWS);
    if (int rc = mip_table_check("pano_view_render", mosaic->h, mosaic->w, offsets, n_levels))
        return rc;
    const double two_pi = 6.283185307179586476925286766559;
    const double res0 = mosaic->res[0], res1 = mosaic->res[1];
    PANO_REQUIRE(isfinite(mosaic->low[0]) && isfinite(mosaic->low[1]) && isfinite(res0) &&
                     isfinite(res1) && res0 > 0 && res1 > 0,
                 "pano_view_render: the mosaic's low / res are not finite and positive");
    PANO_REQUIRE(mosaic->w * res0 <= two_pi + res0 / 2,
                 "pano_view_render: %d columns of %g rad are more than one turn", mosaic->w, res0);
    PANO_REQUIRE(!mosaic->closed || fabs(mosaic->w * res0 - two_pi) < res0 / 2,
                 "pano_view_render: %d columns of %g rad do not close", mosaic->w, res0);

    ViewBatch B = {};
    B.mips = mips;
    for (int l = 0; l < PANO_VIEW_MAX_LEVELS; ++l) B.off[l] = l < n_levels ? offsets[l] : 0;
    B.low0 = (float)mosaic->low[0];
    B.low1 = (float)mosaic->low[1];
    B.res0 = (float)res0;
    B.res1 = (float)res1;
    B.period = (float)(two_pi / res0);
    B.scale = mosaic->closed ? (float)(mosaic->w / (two_pi / res0)) : 1.0f;
    B.h = mosaic->h;
    B.w = mosaic->w;
    B.closed = mosaic->closed != 0;
    B.levels = n_levels;
    B.n = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const pano_view &S = views[i];
        ViewDev &D = B.v[i];
        PANO_REQUIRE(S.kind >= PANO_VIEW_RECTILINEAR && S.kind <= PANO_VIEW_STEREOGRAPHIC,
                     "pano_view_render: view %d: kind %d", i, S.kind);
        PANO_REQUIRE(S.w >= 1 && S.h >= 1 && S.w <= PANO_VIEW_MAX_SIDE && S.h <= PANO_VIEW_MAX_SIDE,
                     "pano_view_render: view %d: %d x %d (sides 1 .. %d)", i, S.w, S.h,
                     PANO_VIEW_MAX_SIDE);
        PANO_REQUIRE(S.image && S.mask, "pano_view_render: view %d: null output", i);
        for (int k = 0; k < 9; ++k) {
            PANO_REQUIRE(isfinite(S.m[k]), "pano_view_render: view %d: matrix not finite", i);
            D.m[k] = (float)S.m[k];
        }
        for (int k = 0; k < 4; ++k) {
            PANO_REQUIRE(isfinite(S.p[k]), "pano_view_render: view %d: parameter not finite", i);
            D.p[k] = (float)S.p[k];
        }
        PANO_REQUIRE(S.kind != PANO_VIEW_STEREOGRAPHIC || S.p[2] > 0,
                     "pano_view_render: view %d: focal length %g", i, S.p[2]);
        D.image = S.image;
        D.mask = S.mask;
        D.kind = S.kind;
        D.w = S.w;
        D.h = S.h;
        batch_assign<PANO_VIEW_MAX_SIDE, VIEW_TX, VIEW_TY, PANO_VIEW_MAX_VIEWS>(D.slot, &blocks, i, S.w, S.h);
    }
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(view_render_kernel, dim3((unsigned)blocks), dim3(VIEW_TX, VIEW_TY), 0, s, B);
    PANO_LAUNCH_CHECK("view_render_kernel");
    return PANO_OK;
}
