// Exposure fusion of bracketed frames at the ingest (pano_fuse_u8, pano_fuse_work_bytes): Mertens,
// Kautz and Van Reeth's fusion of k exposures of one view into one 8-bit frame, with no exposure
// times and no response curve.  Per pixel a weight from contrast, saturation and well-exposedness,
// normalised over the exposures; Gaussian pyramids of the frames and the weights; the weighted sum
// of the frames' Laplacian levels, collapsed.  The contract is in include/pano360.h, a NumPy
// statement of the arithmetic is tests/fuse_model.py; the pyramid filters are those of
// laplacian.hip (pyr.h).
//
// A stack's workspace holds, per level, the k packed images (float4 B, G, R, weight per pixel)
// and the fused level (float4, channel 3 unused).  Four kernels, 3 L + 2 launches per stack:
//   fuse_pack_kernel      the k frames -> weights, normalised, packed level 0
//   fuse_down_kernel      one pyrDown step of all k packed images
//   fuse_level_kernel     R_l = sum_i N_i,l (P_i,l - pyrUp(P_i,l+1)): the Laplacian level of every
//                         exposure is formed in registers from an LDS copy of the level below
//                         and never stored
//   fuse_collapse_kernel  R_l += pyrUp(R_l+1); at level 0 the quantised frame
// No atomics, every sum in a fixed order.
#include <math.h>

#include "geom.h"
#include "pyr.h"

// N floats with the arithmetic of one: what the filters of pyr.h are evaluated on.
template <int N>
struct fvec {
    float v[N];
    __device__ __forceinline__ fvec() {}
    __device__ __forceinline__ fvec(float s) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = s;
    }
};
#define FVEC_OP(op)                                                                          \
    template <int N>                                                                         \
    __device__ __forceinline__ fvec<N> operator op(const fvec<N> &a, const fvec<N> &b) {     \
        fvec<N> r;                                                                           \
        _Pragma("unroll") for (int i = 0; i < N; ++i) r.v[i] = a.v[i] op b.v[i];             \
        return r;                                                                            \
    }
FVEC_OP(+)
FVEC_OP(-)
FVEC_OP(*)
#undef FVEC_OP
typedef fvec<3> bgr_t;
typedef fvec<4> px_t;

__device__ __forceinline__ px_t px_of(float4 p) {
    px_t r;
    r.v[0] = p.x, r.v[1] = p.y, r.v[2] = p.z, r.v[3] = p.w;
    return r;
}
__device__ __forceinline__ bgr_t bgr_of(float4 p) {
    bgr_t r;
    r.v[0] = p.x, r.v[1] = p.y, r.v[2] = p.z;
    return r;
}

struct FuseSrc {                    // the frames of a stack: a kernel argument
    const uint8_t *p[PANO_FUSE_MAX_EXPOSURES];
    int64_t pitch[PANO_FUSE_MAX_EXPOSURES];
};

// ---- stage A and B -----------------------------------------------------------------
#define FP_TX 32                    // pixels across a tile of the pack kernel
#define FP_TY 8                     // its rows: one pixel per thread
#define FP_GW (FP_TX + 2)           // the gray tile with its halo
#define FP_GH (FP_TY + 2)

// prod * v^e: an exponent of 1 multiplies v as it is, of 0 leaves it out
__device__ __forceinline__ float fuse_factor(float prod, float v, float e) {
    if (e == 1.0f) return prod * v;
    if (e == 0.0f) return prod;
    return prod * powf(v, e);
}

// One workgroup per 32 x 8 tile, one thread per pixel, the k exposures one after another: the
// tile's gray values and a 1-pixel halo (reflected at the frame's border, so every entry is a
// pixel of the frame) go through LDS for the Laplacian; a thread keeps its k weights and pixels in
// LDS columns of its own, then normalises and writes one float4 per exposure.
__global__ __launch_bounds__(FP_TX *FP_TY) void fuse_pack_kernel(FuseSrc src, int h, int w, int k, float wc,
                                                                 float ws, float we,
                                                                 float4 *__restrict__ packed,
                                                                 float *__restrict__ raw) {
    __shared__ float s_g[FP_GH][FP_GW + 1];
    __shared__ float s_w[PANO_FUSE_MAX_EXPOSURES][FP_TX * FP_TY];
    __shared__ uint32_t s_px[PANO_FUSE_MAX_EXPOSURES][FP_TX * FP_TY];
    const int tid = threadIdx.x, tx = tid % FP_TX, ty = tid / FP_TX;
    const int x0 = blockIdx.x * FP_TX, y0 = blockIdx.y * FP_TY;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < w && y < h;
    float total = 0.0f;
    for (int i = 0; i < k; ++i) {
        const frame_ptr f = (frame_ptr)src.p[i];
        const int64_t pitch = src.pitch[i];
        __syncthreads();                                // (the exposure before has read its tile)
        for (int e = tid; e < FP_GH * FP_GW; e += FP_TX * FP_TY) {
            const int r = e / FP_GW, c = e - r * FP_GW;
            const frame_ptr q = f + (int64_t)reflect_101(y0 - 1 + r, h) * pitch + 3 * reflect_101(x0 - 1 + c, w);
            const float B = (float)q[0] / 255.0f, G = (float)q[1] / 255.0f, R = (float)q[2] / 255.0f;
            s_g[r][c] = (0.114f * B + 0.587f * G) + 0.299f * R;
        }
        __syncthreads();
        if (!inside) continue;
        const frame_ptr q = f + (int64_t)y * pitch + 3 * x;
        const uint32_t b0 = q[0], b1 = q[1], b2 = q[2];
        const float B = (float)b0 / 255.0f, G = (float)b1 / 255.0f, R = (float)b2 / 255.0f;
        const float g = s_g[ty + 1][tx + 1];
        const float lap = ((s_g[ty + 1][tx] + s_g[ty + 1][tx + 2]) + (s_g[ty][tx + 1] + s_g[ty + 2][tx + 1])) - 4.0f * g;
        const float C = fabsf(lap);
        const float m = ((B + G) + R) / 3.0f;
        const float S = sqrtf((((B - m) * (B - m) + (G - m) * (G - m)) + (R - m) * (R - m)) / 3.0f);
        const float E = expf(-((((B - 0.5f) * (B - 0.5f) + (G - 0.5f) * (G - 0.5f)) + (R - 0.5f) * (R - 0.5f)) / 0.08f));
        const float W = fuse_factor(fuse_factor(fuse_factor(1.0f, C, wc), S, ws), E, we) + 1e-12f;
        total = i == 0 ? W : total + W;
        s_w[i][tid] = W;
        s_px[i][tid] = b0 | (b1 << 8) | (b2 << 16);
    }
    if (!inside) return;
    for (int i = 0; i < k; ++i) {
        const size_t o = ((size_t)i * h + y) * w + x;
        const float W = s_w[i][tid];
        const uint32_t p = s_px[i][tid];
        if (raw) raw[o] = W;
        packed[o] = make_float4((float)(p & 255) / 255.0f, (float)((p >> 8) & 255) / 255.0f,
                                (float)(p >> 16) / 255.0f, W / total);
    }
}

// ---- stage C -------------------------------------------------------------------------
#define FD_TX 32                    // output pixels across a tile of the down kernel
#define FD_TY 8                     // its output rows
#define FD_ROWS (2 * FD_TY + 3)     // the source rows they read

// One pyrDown step of the k packed images: blockIdx.z is the exposure.  Rows, then columns, as the
// shim does: the row pass of the tile's 19 source rows (reflected) at its 32 output columns goes
// to LDS with five 16-byte loads each, the column pass reads it back.
__global__ __launch_bounds__(FD_TX *FD_TY) void fuse_down_kernel(const float4 *__restrict__ src, int h, int w,
                                                                 float4 *__restrict__ dst, int oh, int ow) {
    __shared__ float4 s_row[FD_ROWS][FD_TX];
    src += (size_t)blockIdx.z * h * w;
    dst += (size_t)blockIdx.z * oh * ow;
    const int tid = threadIdx.x, tx = tid % FD_TX, ty = tid / FD_TX;
    const int ox0 = blockIdx.x * FD_TX, oy0 = blockIdx.y * FD_TY;
    for (int e = tid; e < FD_ROWS * FD_TX; e += FD_TX * FD_TY) {
        const int r = e / FD_TX, c = e - r * FD_TX;
        const float4 *row = src + (size_t)reflect_101(2 * oy0 - 2 + r, h) * w;
        px_t a[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) a[j] = px_of(row[reflect_101(2 * (ox0 + c) - 2 + j, w)]);
        const px_t s = pyr_down_taps(a[0], a[1], a[2], a[3], a[4]);
        s_row[r][c] = make_float4(s.v[0], s.v[1], s.v[2], s.v[3]);
    }
    __syncthreads();
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= ow || oy >= oh) return;
    const px_t s = pyr_down_taps(px_of(s_row[2 * ty][tx]), px_of(s_row[2 * ty + 1][tx]), px_of(s_row[2 * ty + 2][tx]),
                                 px_of(s_row[2 * ty + 3][tx]), px_of(s_row[2 * ty + 4][tx])) * px_t(1.0f / 256.0f);
    dst[(size_t)oy * ow + ox] = make_float4(s.v[0], s.v[1], s.v[2], s.v[3]);
}

// ---- stages D and E ----------------------------------------------------------------------
#define FL_TX 64                    // the level and collapse kernels: 64 x 4 pixels, one per thread
#define FL_TY 4

#define FL_CW (FL_TX / 2 + 2)        // the tile's footprint in the level below: 34 x 4 pixels
#define FL_CH (FL_TY / 2 + 2)

// pyrUp(c)[y][x] of the B, G, R of a ch x cw image (ch, cw >= 2; y < 2 ch, x < 2 cw) whose pixel
// in row r, column i is at(r, i)
template <class At>
__device__ __forceinline__ bgr_t fuse_up_at(At at, int ch, int cw, int x, int y) {
    const int sy = y >> 1, ra = sy == 0 ? 1 : sy - 1, rb = sy == ch - 1 ? sy : sy + 1;
    const bgr_t v1 = pyr_up_row<bgr_t>([=](int i) { return at(sy, i); }, cw, x);
    const bgr_t v2 = pyr_up_row<bgr_t>([=](int i) { return at(rb, i); }, cw, x);
    if (y & 1) return pyr_up_col_odd(v1, v2);
    const bgr_t v0 = pyr_up_row<bgr_t>([=](int i) { return at(ra, i); }, cw, x);
    return pyr_up_col_even(v0, v1, v2);
}
// ... of a float4 image in global memory
__device__ __forceinline__ bgr_t fuse_up(const float4 *__restrict__ c, int ch, int cw, int x, int y) {
    return fuse_up_at([=](int r, int i) { return bgr_of(c[(size_t)r * cw + i]); }, ch, cw, x, y);
}

// R_l of one level: the sum over the exposures, in their order, of the level's weight times the
// level's Laplacian (TOP: times the level itself).  fine: [k][h][w], coarse: [k][ch][cw].  Per
// exposure the tile's footprint in the level below - the rows y0 / 2 - 1 .. y0 / 2 + 2 and the
// columns x0 / 2 - 1 .. x0 / 2 + 32, clamped to the image (a clamped entry is never one pyrUp
// reads) - is staged in LDS and up-sampled from there; the sum stays in registers.
template <bool TOP>
__global__ __launch_bounds__(FL_TX *FL_TY) void fuse_level_kernel(const float4 *__restrict__ fine, int h, int w,
                                                                  const float4 *__restrict__ coarse, int ch,
                                                                  int cw, int k, float4 *__restrict__ out) {
    __shared__ float4 s_c[FL_CH][FL_CW];
    const int tid = threadIdx.y * FL_TX + threadIdx.x;
    const int x = blockIdx.x * FL_TX + threadIdx.x, y = blockIdx.y * FL_TY + threadIdx.y;
    const int cx0 = blockIdx.x * (FL_TX / 2) - 1, cy0 = blockIdx.y * (FL_TY / 2) - 1;
    const bool inside = x < w && y < h;
    bgr_t acc(0.0f);
    for (int i = 0; i < k; ++i) {
        if (!TOP) {
            const float4 *c = coarse + (size_t)i * ch * cw;
            __syncthreads();                            // (the exposure before has been read)
            if (tid < FL_CH * FL_CW) {
                const int r = tid / FL_CW, col = tid - r * FL_CW;
                s_c[r][col] = c[(size_t)min(max(cy0 + r, 0), ch - 1) * cw + min(max(cx0 + col, 0), cw - 1)];
            }
            __syncthreads();
        }
        if (!inside) continue;
        const float4 p = fine[((size_t)i * h + y) * w + x];
        bgr_t d = bgr_of(p);
        if (!TOP) d = d - fuse_up_at([&](int r, int j) { return bgr_of(s_c[r - cy0][j - cx0]); }, ch, cw, x, y);
        const bgr_t term = bgr_t(p.w) * d;
        acc = i == 0 ? term : acc + term;
    }
    if (inside) out[(size_t)y * w + x] = make_float4(acc.v[0], acc.v[1], acc.v[2], 0.0f);
}

// R_l += pyrUp(R_l+1) (coarse NULL: R_l as it is, the stack without a level below the frame).
// FINAL, level 0: the sum goes to `fused` if asked and, times 255, clamped and rounded, to dst.
template <bool FINAL>
__global__ __launch_bounds__(FL_TX *FL_TY) void fuse_collapse_kernel(float4 *__restrict__ level, int h, int w,
                                                                     const float4 *__restrict__ coarse, int ch,
                                                                     int cw, uint8_t *__restrict__ dst,
                                                                     int64_t dst_pitch, float *__restrict__ fused) {
    const int x = blockIdx.x * FL_TX + threadIdx.x, y = blockIdx.y * FL_TY + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t o = (size_t)y * w + x;
    bgr_t v = bgr_of(level[o]);
    if (coarse) v = v + fuse_up(coarse, ch, cw, x, y);
    if (!FINAL) {
        level[o] = make_float4(v.v[0], v.v[1], v.v[2], 0.0f);
        return;
    }
    uint8_t *q = dst + (int64_t)y * dst_pitch + 3 * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (fused) fused[3 * o + c] = v.v[c];
        q[c] = (uint8_t)rintf(fminf(fmaxf(v.v[c] * 255.0f, 0.0f), 255.0f));
    }
}

// ---- C ABI -----------------------------------------------------------------------------
static inline int fuse_levels(int h, int w) {           // max(0, bit_length(min(h, w)) - 2)
    int side = h < w ? h : w, bits = 0;
    while (side) ++bits, side >>= 1;
    return bits > 2 ? bits - 2 : 0;
}

struct FuseLevel {                  // a level of a stack in the workspace
    int h, w;
    size_t packed, fused;           // byte offsets: float4 [k][h][w], float4 [h][w]
};

// The levels 0 .. L of an h x w stack of k exposures; returns the bytes they take.
static size_t fuse_layout(int h, int w, int k, FuseLevel *lv) {
    const int L = fuse_levels(h, w);
    size_t at = 0;
    for (int l = 0; l <= L; ++l) {
        if (lv) lv[l].h = h, lv[l].w = w, lv[l].packed = at;
        at += align_up((size_t)16 * k * h * w);
        if (lv) lv[l].fused = at;
        at += align_up((size_t)16 * h * w);
        h = (h + 1) / 2, w = (w + 1) / 2;
    }
    return at;
}

extern "C" size_t pano_fuse_work_bytes(int h, int w, int k) {
    return pano_stack_ok(h, w, k) ? fuse_layout(h, w, k, nullptr) : 0;
}

static int fuse_check(const pano_fuse_stack &S, int i, int n_levels, const void *work, int64_t work_bytes) {
    PANO_REQUIRE(pano_stack_ok(S.h, S.w, S.k), "pano_fuse_u8: stack %d: %d exposures of %d x %d (2 .. %d, sides 1 .. %d)",
                 i, S.k, S.w, S.h, PANO_FUSE_MAX_EXPOSURES, PANO_FUSE_MAX_SIDE);
    PANO_REQUIRE(S.dst, "pano_fuse_u8: stack %d: null dst", i);
    PANO_REQUIRE(S.dst_pitch >= 3 * (int64_t)S.w, "pano_fuse_u8: stack %d: dst pitch %lld for %d pixels", i,
                 (long long)S.dst_pitch, S.w);
    PANO_REQUIRE(n_levels <= fuse_levels(S.h, S.w), "pano_fuse_u8: stack %d: %d levels, %d x %d has at most %d", i,
                 n_levels, S.w, S.h, fuse_levels(S.h, S.w));
    PANO_REQUIRE((int64_t)fuse_layout(S.h, S.w, S.k, nullptr) <= work_bytes,
                 "pano_fuse_u8: stack %d needs a workspace of %zu bytes, %lld given", i,
                 fuse_layout(S.h, S.w, S.k, nullptr), (long long)work_bytes);
    const size_t dst_bytes = (size_t)(S.h - 1) * S.dst_pitch + 3 * (size_t)S.w;
    PANO_REQUIRE(!pano_overlap(S.dst, dst_bytes, work, (size_t)work_bytes),
                 "pano_fuse_u8: stack %d: dst overlaps the workspace", i);
    for (int e = 0; e < S.k; ++e) {
        PANO_REQUIRE(S.src[e], "pano_fuse_u8: stack %d: exposure %d: null pointer", i, e);
        PANO_REQUIRE(S.src_pitch[e] >= 3 * (int64_t)S.w, "pano_fuse_u8: stack %d: exposure %d: pitch %lld for %d pixels",
                     i, e, (long long)S.src_pitch[e], S.w);
        PANO_REQUIRE(!pano_overlap(S.dst, dst_bytes, S.src[e], (size_t)(S.h - 1) * S.src_pitch[e] + 3 * (size_t)S.w),
                     "pano_fuse_u8: stack %d: dst overlaps exposure %d", i, e);
    }
    return PANO_OK;
}

static inline dim3 fuse_grid(int w, int h, int tx, int ty, int z = 1) {
    return dim3((unsigned)ceil_div(w, tx), (unsigned)ceil_div(h, ty), (unsigned)z);
}

static int fuse_stack(const pano_fuse_stack &S, const pano_fuse_params &P, char *work, hipStream_t s) {
    FuseLevel lv[16];
    fuse_layout(S.h, S.w, S.k, lv);
    const int L = P.n_levels < 0 ? fuse_levels(S.h, S.w) : P.n_levels;
    auto packed = [&](int l) { return (float4 *)(work + lv[l].packed); };
    auto level = [&](int l) { return (float4 *)(work + lv[l].fused); };
    FuseSrc src;
    for (int e = 0; e < PANO_FUSE_MAX_EXPOSURES; ++e) {
        src.p[e] = e < S.k ? S.src[e] : nullptr;
        src.pitch[e] = e < S.k ? S.src_pitch[e] : 0;
    }
    hipLaunchKernelGGL(fuse_pack_kernel, fuse_grid(S.w, S.h, FP_TX, FP_TY), dim3(FP_TX * FP_TY), 0, s, src, S.h, S.w,
                       S.k, P.contrast, P.saturation, P.exposure, packed(0), S.raw);
    PANO_LAUNCH_CHECK("fuse_pack_kernel");
    for (int l = 0; l < L; ++l) {
        hipLaunchKernelGGL(fuse_down_kernel, fuse_grid(lv[l + 1].w, lv[l + 1].h, FD_TX, FD_TY, S.k),
                           dim3(FD_TX * FD_TY), 0, s, (const float4 *)packed(l), lv[l].h, lv[l].w, packed(l + 1),
                           lv[l + 1].h, lv[l + 1].w);
        PANO_LAUNCH_CHECK("fuse_down_kernel");
    }
    const dim3 block(FL_TX, FL_TY);
    for (int l = 0; l < L; ++l) {
        hipLaunchKernelGGL(fuse_level_kernel<false>, fuse_grid(lv[l].w, lv[l].h, FL_TX, FL_TY), block, 0, s,
                           (const float4 *)packed(l), lv[l].h, lv[l].w, (const float4 *)packed(l + 1), lv[l + 1].h,
                           lv[l + 1].w, S.k, level(l));
        PANO_LAUNCH_CHECK("fuse_level_kernel");
    }
    hipLaunchKernelGGL(fuse_level_kernel<true>, fuse_grid(lv[L].w, lv[L].h, FL_TX, FL_TY), block, 0, s,
                       (const float4 *)packed(L), lv[L].h, lv[L].w, (const float4 *)nullptr, 0, 0, S.k, level(L));
    PANO_LAUNCH_CHECK("fuse_level_kernel");
    for (int l = L - 1; l >= 1; --l) {
        hipLaunchKernelGGL(fuse_collapse_kernel<false>, fuse_grid(lv[l].w, lv[l].h, FL_TX, FL_TY), block, 0, s,
                           level(l), lv[l].h, lv[l].w, (const float4 *)level(l + 1), lv[l + 1].h, lv[l + 1].w,
                           (uint8_t *)nullptr, (int64_t)0, (float *)nullptr);
        PANO_LAUNCH_CHECK("fuse_collapse_kernel");
    }
    hipLaunchKernelGGL(fuse_collapse_kernel<true>, fuse_grid(S.w, S.h, FL_TX, FL_TY), block, 0, s, level(0), S.h, S.w,
                       L > 0 ? (const float4 *)level(1) : (const float4 *)nullptr, L > 0 ? lv[1].h : 0,
                       L > 0 ? lv[1].w : 0, S.dst, S.dst_pitch, S.fused);
    PANO_LAUNCH_CHECK("fuse_collapse_kernel");
    return PANO_OK;
}

extern "C" int pano_fuse_u8(pano_ctx *ctx, const pano_fuse_stack *stacks, int n, const pano_fuse_params *params,
                            void *work, int64_t work_bytes) {
    PANO_ENTER(ctx, "pano_fuse_u8");
    PANO_REQUIRE(stacks && params && work, "pano_fuse_u8: null pointer");
    PANO_REQUIRE(n >= 1, "pano_fuse_u8: %d stacks", n);
    PANO_REQUIRE(work_bytes >= 0, "pano_fuse_u8: a workspace of %lld bytes", (long long)work_bytes);
    const float expo[3] = {params->contrast, params->saturation, params->exposure};
    for (int c = 0; c < 3; ++c)
        PANO_REQUIRE(isfinite(expo[c]) && expo[c] >= 0.0f, "pano_fuse_u8: exponent %d is %g (finite, >= 0)", c,
                     (double)expo[c]);
    PANO_REQUIRE(params->n_levels >= -1, "pano_fuse_u8: %d levels (-1: the default)", params->n_levels);
    for (int i = 0; i < n; ++i)                         // (nothing is queued for a refused call)
        if (int rc = fuse_check(stacks[i], i, params->n_levels, work, work_bytes)) return rc;
    for (int i = 0; i < n; ++i)
        if (int rc = fuse_stack(stacks[i], *params, (char *)work, (hipStream_t)stream)) return rc;
    return PANO_OK;
}
