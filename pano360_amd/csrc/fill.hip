// Pull-push fill of a uint8 image's invalid pixels (pano_fill_u8) and the per-pixel choice between
// two images (pano_select_u8).  The pull averages the valid pixels down the chain of
// view.mip_shapes until one pixel is left, the push walks back up and gives every invalid pixel
// the 9 : 3 : 3 : 1 mix of the four nearest pixels of the level above.  The contract is in
// include/pano360.h, the host side is pano360_amd/fill.py and a float64 statement of the arithmetic
// is tests/fill_model.py.  A level >= 1 is float4 texels (r, g, b, validity): one 16-byte access
// per pixel.  No atomics; every pixel is written by one thread from values that do not depend on
// the grid, so the same input gives the same bytes.
#include "common.h"
#include "fill_layout.h"

#define FILL_BLOCK 256
#define FILL_MAX_GROUPS 4096        // grid cap of the per-level kernels (they loop beyond it)
#define FILL_TAIL_BLOCK 1024        // the tail is ONE workgroup
#define SELECT_GROUP 16             // pixels of one vector step of select_kernel: 3 x 16 bytes

// ---- sources of texels ------------------------------------------------------------------------------
struct FillU8 {                     // level 0: the image and its mask, at their pitches
    const uint8_t *img, *mask;
    int64_t pitch, mpitch;
    __device__ __forceinline__ float4 at(int y, int x) const {
        const uint8_t *p = img + (int64_t)y * pitch + 3 * (int64_t)x;
        return make_float4((float)p[0], (float)p[1], (float)p[2],
                           mask[(int64_t)y * mpitch + x] ? 1.0f : 0.0f);
    }
};
struct FillF4 {                     // a level >= 1, dense (global memory or LDS)
    const float4 *p;
    int w;
    __device__ __forceinline__ float4 at(int y, int x) const { return p[(int64_t)y * w + x]; }
};

// pixel (Y, X) of the level below a source of sh x sw: the mean of its valid children, summed in the
// order (0,0), (0,1), (1,0), (1,1); children outside the source do not exist
template <class S>
__device__ __forceinline__ float4 fill_pull(const S &src, int sh, int sw, int Y, int X) {
    float r = 0.0f, g = 0.0f, b = 0.0f;
    int count = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int y = 2 * Y + dy, x = 2 * X + dx;
            if (y < sh && x < sw) {
                const float4 t = src.at(y, x);
                if (t.w != 0.0f) {
                    r += t.x;
                    g += t.y;
                    b += t.z;
                    ++count;
                }
            }
        }
    if (count == 0) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float n = (float)count;
    return make_float4(r / n, g / n, b / n, 1.0f);
}

// the filled colour of the invalid pixel (y, x) from the level above (uh x uw, already filled):
// rows clamped, columns clamped (open) or modulo uw (closed); four terms added left to right
template <class S>
__device__ __forceinline__ float4 fill_push(const S &up, int uh, int uw, int closed, int y, int x) {
    const int Y = y >> 1, X = x >> 1;
    const int Y2 = min(max(Y + ((y & 1) ? 1 : -1), 0), uh - 1);
    int X2 = X + ((x & 1) ? 1 : -1);
    if (closed)
        X2 = X2 < 0 ? uw - 1 : (X2 >= uw ? 0 : X2);
    else
        X2 = min(max(X2, 0), uw - 1);
    const float4 a = up.at(Y, X), b = up.at(Y, X2), c = up.at(Y2, X), d = up.at(Y2, X2);
    return make_float4(((0.5625f * a.x + 0.1875f * b.x) + 0.1875f * c.x) + 0.0625f * d.x,
                       ((0.5625f * a.y + 0.1875f * b.y) + 0.1875f * c.y) + 0.0625f * d.y,
                       ((0.5625f * a.z + 0.1875f * b.z) + 0.1875f * c.z) + 0.0625f * d.z, 0.0f);
}

__device__ __forceinline__ uint8_t fill_round(float v) {
    return (uint8_t)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f);
}

// ---- 1. pull: one thread per pixel of the destination level -------------------------------------------
template <class S>
__global__ __launch_bounds__(FILL_BLOCK) void fill_pull_kernel(const S src, int sh, int sw,
                                                               float4 *__restrict__ dst) {
    const int dh = (sh + 1) >> 1, dw = (sw + 1) >> 1;
    const unsigned n = (unsigned)dh * (unsigned)dw;     // (at most 2^28: the source has at most 2^30)
    for (unsigned i = blockIdx.x * FILL_BLOCK + threadIdx.x; i < n; i += gridDim.x * FILL_BLOCK) {
        const int Y = (int)(i / (unsigned)dw), X = (int)(i - (unsigned)Y * (unsigned)dw);
        dst[i] = fill_pull(src, sh, sw, Y, X);
    }
}

// ---- 2. push of a level >= 1, in place: only the invalid texels are written ---------------------------
__global__ __launch_bounds__(FILL_BLOCK) void fill_push_kernel(float4 *__restrict__ cur, int h, int w,
                                                               const float4 *__restrict__ up, int uh,
                                                               int uw, int closed) {
    const unsigned n = (unsigned)h * (unsigned)w;
    const FillF4 above = {up, uw};
    for (unsigned i = blockIdx.x * FILL_BLOCK + threadIdx.x; i < n; i += gridDim.x * FILL_BLOCK) {
        if (cur[i].w != 0.0f) continue;
        const int y = (int)(i / (unsigned)w), x = (int)(i - (unsigned)y * (unsigned)w);
        cur[i] = fill_push(above, uh, uw, closed, y, x);
    }
}

// ---- 3. push of level 0: uint8 at the output's pitch ---------------------------------------------------
// `out` may be `img` (then the pitches are equal and only the invalid pixels are written).  *any == 0:
// no pixel of the image is valid and the output is the input.
__global__ __launch_bounds__(FILL_BLOCK) void fill_push_u8_kernel(
    const uint8_t *img, int64_t pitch, const uint8_t *__restrict__ mask, int64_t mpitch, int h, int w,
    const float4 *__restrict__ up, int uh, int uw, int closed, const uint32_t *__restrict__ any,
    uint8_t *out, int64_t opitch) {
    const unsigned n = (unsigned)h * (unsigned)w;       // (at most 2^30)
    const FillF4 above = {up, uw};
    const bool fill = *any != 0, same = out == img;
    for (unsigned i = blockIdx.x * FILL_BLOCK + threadIdx.x; i < n; i += gridDim.x * FILL_BLOCK) {
        const int y = (int)(i / (unsigned)w), x = (int)(i - (unsigned)y * (unsigned)w);
        uint8_t *q = out + (int64_t)y * opitch + 3 * (int64_t)x;
        if (fill && mask[(int64_t)y * mpitch + x] == 0) {
            const float4 f = fill_push(above, uh, uw, closed, y, x);
            q[0] = fill_round(f.x);
            q[1] = fill_round(f.y);
            q[2] = fill_round(f.z);
        } else if (!same) {
            const uint8_t *p = img + (int64_t)y * pitch + 3 * (int64_t)x;
            q[0] = p[0];
            q[1] = p[1];
            q[2] = p[2];
        }
    }
}

// ---- 4. the tail: one workgroup, every level from `tail` to 1 x 1 in LDS ---------------------------------
struct FillTail {
    const uint8_t *img, *mask;      // level 0
    int64_t pitch, mpitch;
    const float4 *below;            // level tail - 1 when tail >= 2 (pulled by the launches before)
    float4 *level;                  // level tail in the workspace when tail >= 1: gets its filled texels
    uint8_t *out;                   // tail == 0: the output
    int64_t opitch;
    uint32_t *any;                  // gets 1 when the image has a valid pixel, else 0
    int n, tail, closed;
    int h[FILL_MAX_LEVELS], w[FILL_MAX_LEVELS], lds[FILL_MAX_LEVELS + 1];
};

__global__ __launch_bounds__(FILL_TAIL_BLOCK) void fill_tail_kernel(const FillTail A) {
    extern __shared__ __attribute__((aligned(16))) float4 fill_lds[];
    const int T = A.tail, tid = (int)threadIdx.x;
    const FillU8 image = {A.img, A.mask, A.pitch, A.mpitch};
    float4 *const top = fill_lds + A.lds[T];
    const int th = A.h[T], tw = A.w[T], tn = th * tw;   // (at most PANO_FILL_TAIL_PIXELS)
    // level T: the image itself, or pulled from level T - 1 in global memory
    for (int i = tid; i < tn; i += FILL_TAIL_BLOCK) {
        const int y = i / tw, x = i - y * tw;
        float4 t;
        if (T == 0)
            t = image.at(y, x);
        else if (T == 1)
            t = fill_pull(image, A.h[0], A.w[0], y, x);
        else
            t = fill_pull(FillF4{A.below, A.w[T - 1]}, A.h[T - 1], A.w[T - 1], y, x);
        top[i] = t;
    }
    __syncthreads();
    for (int l = T + 1; l < A.n; ++l) {                 // pull down to 1 x 1
        const FillF4 src = {fill_lds + A.lds[l - 1], A.w[l - 1]};
        float4 *const dst = fill_lds + A.lds[l];
        const int lw = A.w[l], ln = A.h[l] * lw;
        for (int i = tid; i < ln; i += FILL_TAIL_BLOCK) {
            const int y = i / lw, x = i - y * lw;
            dst[i] = fill_pull(src, A.h[l - 1], A.w[l - 1], y, x);
        }
        __syncthreads();
    }
    const bool any = fill_lds[A.lds[A.n - 1]].w != 0.0f;  // (the 1 x 1 level: valid if any pixel is)
    for (int l = A.n - 2; l >= T; --l) {                // push back up to level T
        const FillF4 up = {fill_lds + A.lds[l + 1], A.w[l + 1]};
        float4 *const cur = fill_lds + A.lds[l];
        const int lw = A.w[l], ln = A.h[l] * lw;
        for (int i = tid; i < ln; i += FILL_TAIL_BLOCK) {
            if (cur[i].w != 0.0f) continue;
            const int y = i / lw, x = i - y * lw;
            cur[i] = fill_push(up, A.h[l + 1], A.w[l + 1], A.closed, y, x);
        }
        __syncthreads();
    }
    if (tid == 0) *A.any = any ? 1u : 0u;
    if (T >= 1) {
        for (int i = tid; i < tn; i += FILL_TAIL_BLOCK) A.level[i] = top[i];
        return;
    }
    const bool same = A.out == A.img;
    for (int i = tid; i < tn; i += FILL_TAIL_BLOCK) {
        const int y = i / tw, x = i - y * tw;
        const float4 t = top[i];
        uint8_t *q = A.out + (int64_t)y * A.opitch + 3 * (int64_t)x;
        if (any && t.w == 0.0f) {
            q[0] = fill_round(t.x);
            q[1] = fill_round(t.y);
            q[2] = fill_round(t.z);
        } else if (!same) {
            const uint8_t *p = A.img + (int64_t)y * A.pitch + 3 * (int64_t)x;
            q[0] = p[0];
            q[1] = p[1];
            q[2] = p[2];
        }
    }
}

extern "C" int pano_fill_u8(pano_ctx *ctx, const uint8_t *img, int64_t img_pitch, const uint8_t *mask,
                            int64_t mask_pitch, int h, int w, int closed, uint8_t *out,
                            int64_t out_pitch) {
    PANO_ENTER(ctx, "pano_fill_u8");
    PANO_REQUIRE(img && mask && out, "pano_fill_u8: null pointer");
    FillLayout L;
    PANO_REQUIRE(fill_layout(h, w, &L), "pano_fill_u8: an image of %d x %d (sides 1 .. %d)", w, h,
                 PANO_VIEW_MAX_SIDE);
    PANO_REQUIRE(img_pitch >= 3 * (int64_t)w && out_pitch >= 3 * (int64_t)w && mask_pitch >= w,
                 "pano_fill_u8: pitches %lld, %lld, %lld for %d pixels", (long long)img_pitch,
                 (long long)mask_pitch, (long long)out_pitch, w);
    PANO_REQUIRE(out != img || out_pitch == img_pitch,
                 "pano_fill_u8: in place, but the pitches are %lld and %lld", (long long)img_pitch,
                 (long long)out_pitch);
    const hipStream_t s = (hipStream_t)stream;
    // (the last fill's kernels may still use the old buffer)
    if (int rc = pano_buf_reserve_sync(ctx, BUF_FILL_DEV, (size_t)L.bytes, s)) return rc;
    uint8_t *const base = (uint8_t *)ctx->buf[BUF_FILL_DEV].p;
    uint32_t *const any = (uint32_t *)base;
    const auto level = [&](int l) { return (float4 *)(base + L.off[l]); };
    const auto grid = [](int64_t pixels) { return capped_grid(ceil_div(pixels, FILL_BLOCK), FILL_MAX_GROUPS); };
    const FillU8 image = {img, mask, img_pitch, mask_pitch};

    for (int l = 1; l < L.tail; ++l) {                  // the levels of more than 4096 pixels
        const int64_t n = (int64_t)L.h[l] * L.w[l];
        if (l == 1)
            hipLaunchKernelGGL(fill_pull_kernel<FillU8>, grid(n), dim3(FILL_BLOCK), 0, s, image, h, w,
                               level(1));
        else
            hipLaunchKernelGGL(fill_pull_kernel<FillF4>, grid(n), dim3(FILL_BLOCK), 0, s,
                               FillF4{level(l - 1), L.w[l - 1]}, L.h[l - 1], L.w[l - 1], level(l));
        PANO_LAUNCH_CHECK("fill_pull_kernel");
    }

    FillTail A = {};
    A.img = img;
    A.mask = mask;
    A.pitch = img_pitch;
    A.mpitch = mask_pitch;
    A.below = L.tail >= 2 ? level(L.tail - 1) : nullptr;
    A.level = L.tail >= 1 ? level(L.tail) : nullptr;
    A.out = out;
    A.opitch = out_pitch;
    A.any = any;
    A.n = L.n;
    A.tail = L.tail;
    A.closed = closed != 0;
    for (int l = 0; l < L.n; ++l) {
        A.h[l] = L.h[l];
        A.w[l] = L.w[l];
    }
    for (int l = 0; l <= L.n; ++l) A.lds[l] = L.lds[l];
    const size_t lds_bytes = (size_t)FILL_TEXEL * L.lds[L.n];
    // (a level of 4096 pixels and everything below it: less than 2 x 64 KB)
    PANO_REQUIRE(lds_bytes <= 128 * 1024, "pano_fill_u8: the tail needs %zu bytes of LDS", lds_bytes);
    PANO_HIP(hipFuncSetAttribute((const void *)fill_tail_kernel,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    hipLaunchKernelGGL(fill_tail_kernel, dim3(1), dim3(FILL_TAIL_BLOCK), lds_bytes, s, A);
    PANO_LAUNCH_CHECK("fill_tail_kernel");

    for (int l = L.tail - 1; l >= 1; --l) {
        hipLaunchKernelGGL(fill_push_kernel, grid((int64_t)L.h[l] * L.w[l]), dim3(FILL_BLOCK), 0, s,
                           level(l), L.h[l], L.w[l], level(l + 1), L.h[l + 1], L.w[l + 1], A.closed);
        PANO_LAUNCH_CHECK("fill_push_kernel");
    }
    if (L.tail >= 1) {
        hipLaunchKernelGGL(fill_push_u8_kernel, grid((int64_t)h * w), dim3(FILL_BLOCK), 0, s, img,
                           img_pitch, mask, mask_pitch, h, w, level(1), L.h[1], L.w[1], A.closed, any,
                           out, out_pitch);
        PANO_LAUNCH_CHECK("fill_push_u8_kernel");
    }
    return PANO_OK;
}

// ---- 5. select -------------------------------------------------------------------------------------
// out = mask ? a : b per pixel (out may be a or b: a thread reads its pixels before it writes them).
// With every pointer on 16 bytes a thread takes 16 pixels at a time
// (three 16-byte words of each image, one of the mask); the pixels left over, or all of them, go one
// per thread.
__global__ __launch_bounds__(FILL_BLOCK) void select_kernel(const uint8_t *a,
                                                            const uint8_t *__restrict__ mask,
                                                            const uint8_t *b, uint8_t *out,
                                                            int64_t groups, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * FILL_BLOCK;
    const int64_t first = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
    for (int64_t g = first; g < groups; g += stride) {
        const uint4 m4 = ((const uint4 *)mask)[g];
        const uint32_t m[4] = {m4.x, m4.y, m4.z, m4.w};
        uint32_t va[12], vb[12], vo[12];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 x = ((const uint4 *)a)[3 * g + k], y = ((const uint4 *)b)[3 * g + k];
            va[4 * k] = x.x, va[4 * k + 1] = x.y, va[4 * k + 2] = x.z, va[4 * k + 3] = x.w;
            vb[4 * k] = y.x, vb[4 * k + 1] = y.y, vb[4 * k + 2] = y.z, vb[4 * k + 3] = y.w;
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {                  // byte j of word k belongs to pixel (4 k + j) / 3
            uint32_t take = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pixel = (4 * k + j) / 3;
                if ((m[pixel >> 2] >> (8 * (pixel & 3))) & 0xffu) take |= 0xffu << (8 * j);
            }
            vo[k] = (va[k] & take) | (vb[k] & ~take);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            ((uint4 *)out)[3 * g + k] = make_uint4(vo[4 * k], vo[4 * k + 1], vo[4 * k + 2], vo[4 * k + 3]);
    }
    for (int64_t i = groups * SELECT_GROUP + first; i < n; i += stride) {
        const uint8_t *p = mask[i] ? a + 3 * i : b + 3 * i;
        out[3 * i] = p[0];
        out[3 * i + 1] = p[1];
        out[3 * i + 2] = p[2];
    }
}

extern "C" int pano_select_u8(pano_ctx *ctx, const uint8_t *a, const uint8_t *mask, const uint8_t *b,
                              uint8_t *out, int64_t n_pixels) {
    PANO_ENTER(ctx, "pano_select_u8");
    PANO_REQUIRE(a && mask && b && out, "pano_select_u8: null pointer");
    PANO_REQUIRE(n_pixels >= 1 && n_pixels <= (int64_t)PANO_VIEW_MAX_SIDE * PANO_VIEW_MAX_SIDE,
                 "pano_select_u8: %lld pixels (1 .. %d x %d)", (long long)n_pixels, PANO_VIEW_MAX_SIDE,
                 PANO_VIEW_MAX_SIDE);
    const bool aligned = (((uintptr_t)a | (uintptr_t)mask | (uintptr_t)b | (uintptr_t)out) & 15) == 0;
    const int64_t groups = aligned ? n_pixels / SELECT_GROUP : 0;
    const int64_t threads = groups > n_pixels - groups * SELECT_GROUP ? groups
                                                                      : n_pixels - groups * SELECT_GROUP;
    hipLaunchKernelGGL(select_kernel, capped_grid(ceil_div(threads, FILL_BLOCK), FILL_MAX_GROUPS),
                       dim3(FILL_BLOCK), 0, (hipStream_t)stream, a, mask, b, out, groups, n_pixels);
    PANO_LAUNCH_CHECK("select_kernel");
    return PANO_OK;
}
