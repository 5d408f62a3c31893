// Lens correction at the ingest (pano_lens_undistort_u8): every frame of a batch is resampled once
// into the ideal centred pinhole image the rest of the pipeline assumes.  An output pixel goes
// through the calibration's FORWARD model (OpenCV's Brown-Conrady or fisheye coefficients) in
// float64 - correcting needs no iteration -, the position is quantised to 1/32 pixel and sampled
// with Catmull-Rom or bilinear weights in float32, the border replicated.  The contract is in
// include/pano360.h, the host side is pano360_amd/lens.py and a NumPy statement of the arithmetic
// is tests/lens_model.py.  No atomics, every pixel is written by one thread: the same input gives
// the same bytes.
#include <math.h>

#include "batch.h"
#include "geom.h"

#define LENS_PX 4                   // neighbouring pixels of a row a thread owns: 12 bytes, 3 dwords
#define LENS_GX 16                  // threads across a tile: 64 pixels
#define LENS_GY 16                  // rows of a tile; a wave is 64 pixels x 4 rows
#define LENS_TX (LENS_GX * LENS_PX)
#define LENS_CHUNK 64               // frames of one launch (pano_lens_undistort_u8 takes any number)

struct LensDev {                    // a frame of a launch, in device memory
    pano_lens_frame f;
    TileSlot slot;
    int reserved[2];
};

// the sampling position of output pixel (u, v), quantised: integer parts and 1/32 fractions
__device__ __forceinline__ void lens_position(const pano_lens_frame &F, int u, int v, int &ix,
                                              int &iy, int &fx5, int &fy5) {
    const double x = ((double)u - (double)F.w / 2.0) / F.f_new;
    const double y = ((double)v - (double)F.h / 2.0) / F.f_new;
    double xd, yd;
    if (F.model == PANO_LENS_BROWN) {
        const double k1 = F.k[0], k2 = F.k[1], p1 = F.k[2], p2 = F.k[3], k3 = F.k[4];
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
    } else {
        const double r = sqrt(x * x + y * y);
        const double th = atan(r), t2 = th * th;
        const double thd = th * (1.0 + t2 * (F.k[0] + t2 * (F.k[1] + t2 * (F.k[2] + t2 * F.k[3]))));
        const double s = r > 0.0 ? thd / r : 1.0;
        xd = x * s;
        yd = y * s;
    }
    // (fmax / fmin: a position that is not a number samples at -2)
    const double px = fmin(fmax(F.fx * xd + F.cx, -2.0), (double)(F.w + 1));
    const double py = fmin(fmax(F.fy * yd + F.cy, -2.0), (double)(F.h + 1));
    const int sx = (int)rint(px * 32.0), sy = (int)rint(py * 32.0);
    ix = sx >> 5;
    fx5 = sx & 31;
    iy = sy >> 5;
    fy5 = sy & 31;
}

// the TAPS weights at t = f5 / 32: Catmull-Rom (dyadic, exact in float32) or 1 - t, t
template <int TAPS>
__device__ __forceinline__ void lens_weights(int f5, float w[TAPS]) {
    const float t = (float)f5 * (1.0f / 32.0f);
    if constexpr (TAPS == 4) {
        w[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
        w[1] = (1.5f * t - 2.5f) * t * t + 1.0f;
        w[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
        w[3] = (0.5f * t - 0.5f) * t * t;
    } else {
        w[0] = 1.0f - t;
        w[1] = t;
    }
}

// ((p0 w0 + p1 w1) + p2 w2) + p3 w3, one rounding per operation
template <int TAPS>
__device__ __forceinline__ float lens_dot(const float p[TAPS], const float w[TAPS]) {
    float a = p[0] * w[0];
#pragma unroll
    for (int t = 1; t < TAPS; ++t) a = a + p[t] * w[t];
    return a;
}

// One pixel: TAPS x TAPS taps around (ix, iy), every index clamped to the frame.  Away from the
// left and right border a row's taps are 3 TAPS neighbouring bytes: three dwords (cubic) or a
// dword and a halfword (linear) at any alignment; they end at byte 3 (x + TAPS) - 1 <= 3 w - 1.
template <int TAPS>
__device__ __forceinline__ void lens_sample(frame_ptr src, int64_t pitch, int w, int h, int ix,
                                            int iy, int fx5, int fy5, uint32_t out[3]) {
    float wx[TAPS], wy[TAPS];
    lens_weights<TAPS>(fx5, wx);
    lens_weights<TAPS>(fy5, wy);
    const int x0 = TAPS == 4 ? ix - 1 : ix, y0 = TAPS == 4 ? iy - 1 : iy;
    const bool inside = x0 >= 0 && x0 + TAPS - 1 <= w - 1;
    float rows[3][TAPS];
#pragma unroll
    for (int r = 0; r < TAPS; ++r) {
        const int yy = min(max(y0 + r, 0), h - 1);
        const frame_ptr row = src + (int64_t)yy * pitch;
        float p[3][TAPS];
        if (inside) {
            const frame_ptr a = row + 3 * x0;
            uint32_t px[TAPS][3];
            if constexpr (TAPS == 4)
                rgb4_unpack(*(frame_ptr32)a, *(frame_ptr32)(a + 4), *(frame_ptr32)(a + 8), px);
            else
                rgb2_load(a, px);
#pragma unroll
            for (int t = 0; t < TAPS; ++t)
                p[0][t] = (float)px[t][0], p[1][t] = (float)px[t][1], p[2][t] = (float)px[t][2];
        } else {
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const frame_ptr a = row + 3 * min(max(x0 + t, 0), w - 1);
                p[0][t] = (float)a[0], p[1][t] = (float)a[1], p[2][t] = (float)a[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) rows[c][r] = lens_dot<TAPS>(p[c], wx);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        out[c] = (uint32_t)fminf(fmaxf(rintf(lens_dot<TAPS>(rows[c], wy)), 0.0f), 255.0f);
}

// One workgroup per 64 x 16 tile of one frame, one thread per four neighbouring pixels of a row.
// The frame comes from the table's prefix of workgroup counts (batch.h).
__global__ __launch_bounds__(LENS_GX *LENS_GY) void lens_undistort_kernel(
    const LensDev *__restrict__ table, int n) {
    int tile;
    const LensDev &D = batch_record(table, n, tile);
    const pano_lens_frame &F = D.f;
    const int u0 = (tile % D.slot.tiles_x) * LENS_TX + ((int)threadIdx.x % LENS_GX) * LENS_PX;
    const int v = (tile / D.slot.tiles_x) * LENS_GY + (int)threadIdx.x / LENS_GX;
    const int w = F.w, h = F.h;
    if (u0 >= w || v >= h) return;
    const frame_ptr src = (frame_ptr)F.src;
    const int64_t pitch = F.src_pitch;
    const bool cubic = F.interp == PANO_LENS_CUBIC;

    uint32_t b[LENS_PX][3];
#pragma unroll
    for (int j = 0; j < LENS_PX; ++j) {
        b[j][0] = b[j][1] = b[j][2] = 0;
        if (u0 + j < w) {
            int ix, iy, fx5, fy5;
            lens_position(F, u0 + j, v, ix, iy, fx5, fy5);
            if (cubic)
                lens_sample<4>(src, pitch, w, h, ix, iy, fx5, fy5, b[j]);
            else
                lens_sample<2>(src, pitch, w, h, ix, iy, fx5, fy5, b[j]);
        }
    }
    rgb4_store((rgb_out_ptr)F.dst + (int64_t)v * F.dst_pitch + 3 * u0, u0, w, b);
}

static int lens_check(const pano_lens_frame &F, int i) {
    PANO_REQUIRE(F.src && F.dst, "pano_lens_undistort_u8: frame %d: null pointer", i);
    if (int rc = rgb_frames_check("pano_lens_undistort_u8", i, F.src, F.src_pitch, F.dst, F.dst_pitch, F.w,
                                  F.h, PANO_LENS_MAX_SIDE, false))
        return rc;
    bool finite = isfinite(F.fx) && isfinite(F.fy) && isfinite(F.cx) && isfinite(F.cy) &&
                  isfinite(F.f_new);
    for (int k = 0; k < 5; ++k) finite = finite && isfinite(F.k[k]);
    PANO_REQUIRE(finite, "pano_lens_undistort_u8: frame %d: a parameter is not finite", i);
    PANO_REQUIRE(F.fx > 0 && F.fy > 0 && F.f_new > 0,
                 "pano_lens_undistort_u8: frame %d: focal lengths %g, %g, %g", i, F.fx, F.fy, F.f_new);
    PANO_REQUIRE(F.model == PANO_LENS_BROWN || F.model == PANO_LENS_FISHEYE,
                 "pano_lens_undistort_u8: frame %d: model %d", i, F.model);
    PANO_REQUIRE(F.interp == PANO_LENS_CUBIC || F.interp == PANO_LENS_LINEAR,
                 "pano_lens_undistort_u8: frame %d: interpolation %d", i, F.interp);
    return PANO_OK;
}

extern "C" int pano_lens_undistort_u8(pano_ctx *ctx, const pano_lens_frame *frames, int n) {
    PANO_ENTER(ctx, "pano_lens_undistort_u8");
    PANO_REQUIRE(frames, "pano_lens_undistort_u8: null pointer");
    PANO_REQUIRE(n >= 1, "pano_lens_undistort_u8: %d frames", n);
    for (int i = 0; i < n; ++i)                         // (nothing is queued for a refused batch)
        if (int rc = lens_check(frames[i], i)) return rc;

    std::vector<LensDev> table((size_t)n);
    std::vector<int> blocks((size_t)ceil_div(n, LENS_CHUNK), 0);
    for (int i = 0; i < n; ++i) {
        LensDev &D = table[i];
        D.f = frames[i];
        D.reserved[0] = D.reserved[1] = 0;
        batch_assign<PANO_LENS_MAX_SIDE, LENS_TX, LENS_GY, LENS_CHUNK>(D.slot, blocks.data(), i, D.f.w, D.f.h);
    }
    const hipStream_t s = (hipStream_t)stream;
    return batch_run(ctx, BUF_LENS_DEV, table, LENS_CHUNK, blocks.data(), s, "lens_undistort_kernel",
                     [&](const LensDev *records, int count, int grid) {
        hipLaunchKernelGGL(lens_undistort_kernel, dim3((unsigned)grid), dim3(LENS_GX * LENS_GY), 0, s, records,
                           count);
    });
}
