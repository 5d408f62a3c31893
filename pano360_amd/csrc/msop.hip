// The MSOP detector of the reference (features.py:27-156, 204-212) on the device: Harris
// corners, the cut of the strongest local maxima, the greedy walk of the adaptive non-maximal
// suppression (ssc) and the oriented 8 x 8 descriptors.
//
// What the reference gets from OpenCV (cornerHarris, Sobel, warpPerspective) is restated from
// OpenCV's published behaviour, float32 with one rounding per operation and double where OpenCV
// uses double.  PARITY UNPINNED: OpenCV is not in the reference repo.  tests/msop_model.py states
// the same arithmetic in NumPy and is the specification of these kernels; DESIGN 5i lists the
// reference's quirks that are kept (the cut is handed on weakest first; ssc reads the row as x;
// theta = atan2(g_x, g_y)).
//
//   pano_harris           gray -> response, one fused pass: the Sobel pair and the three products
//                         of a 33 x 9 apron go to LDS, the 2 x 2 box sum and the response follow
//   pano_sobel            the unscaled dx / dy planes that feed pano_msop_smooth
//   pano_msop_smooth      gaussian_filter in sepFilter2D's own operation order (no FMA)
//   pano_msop_candidates  3 x 3 local maxima, compacted in row-major order with ordered keys
//   pano_msop_cut         one stable radix sort (rocPRIM) and the tail of the strongest
//   pano_ssc_probe        one greedy walk of ssc for one width, one wave, 64 points a step
//   pano_msop_describe    angle, bilinear 8 x 8 tile, NumPy's mean / std, one wave per point
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "common.h"

namespace {

constexpr int HT_W = 32, HT_H = 8;            // pano_harris: outputs per block
constexpr int SSC_LDS_WORDS = PANO_SSC_ONCHIP_CELLS / 32;   // the on-chip bitmap: 64 KiB

// Sobel 3 x 3 at (y, x), REFLECT_101, row pass then column pass (cv::Sobel, ksize 3): the
// difference is p[+1] - p[-1], the smoothing (p[-1] + p[+1]) + 2 p[0].
__device__ __forceinline__ void sobel_at(const float *__restrict__ g, int h, int w, int y, int x,
                                         float &dx, float &dy) {
    const int xm = reflect_101(x - 1, w), xp = reflect_101(x + 1, w);
    float d[3], s[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float *row = g + (size_t)reflect_101(y - 1 + r, h) * w;
        const float a = row[xm], b = row[x], c = row[xp];
        d[r] = c - a;
        s[r] = (a + c) + b * 2.0f;
    }
    dx = (d[0] + d[2]) + d[1] * 2.0f;
    dy = s[2] - s[0];
}

// cv2.cornerHarris(gray, blockSize 2, ksize 3, k): Sobel scaled by 1/8, the products, the
// unnormalised 2 x 2 box sum with anchor (1, 1) - rows y-1 .. y, columns x-1 .. x, REFLECT_101 on
// the product planes, i.e. the product AT the reflected coordinate - and the response.
__global__ __launch_bounds__(HT_W *HT_H) void harris_kernel(const float *__restrict__ gray, int h,
                                                            int w, float k,
                                                            float *__restrict__ out) {
    __shared__ float pxx[HT_H + 1][HT_W + 1], pxy[HT_H + 1][HT_W + 1], pyy[HT_H + 1][HT_W + 1];
    const int x0 = blockIdx.x * HT_W, y0 = blockIdx.y * HT_H;
    const int tid = threadIdx.y * HT_W + threadIdx.x;
    for (int q = tid; q < (HT_H + 1) * (HT_W + 1); q += HT_W * HT_H) {
        const int j = q / (HT_W + 1), i = q % (HT_W + 1);
        const int yy = reflect_101(y0 - 1 + j, h), xx = reflect_101(x0 - 1 + i, w);
        float dx, dy;
        sobel_at(gray, h, w, yy, xx, dx, dy);
        dx *= 0.125f;
        dy *= 0.125f;
        pxx[j][i] = dx * dx;
        pxy[j][i] = dx * dy;
        pyy[j][i] = dy * dy;
    }
    __syncthreads();
    const int tx = threadIdx.x, ty = threadIdx.y, x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    const float a = (pxx[ty][tx] + pxx[ty][tx + 1]) + (pxx[ty + 1][tx] + pxx[ty + 1][tx + 1]);
    const float b = (pxy[ty][tx] + pxy[ty][tx + 1]) + (pxy[ty + 1][tx] + pxy[ty + 1][tx + 1]);
    const float c = (pyy[ty][tx] + pyy[ty][tx + 1]) + (pyy[ty + 1][tx] + pyy[ty + 1][tx + 1]);
    const float det = a * c - b * b;
    out[(size_t)y * w + x] = det - (k * (a + c)) * (a + c);
}

__global__ __launch_bounds__(256) void sobel_kernel(const float *__restrict__ gray, int h, int w,
                                                    float *__restrict__ dx,
                                                    float *__restrict__ dy) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    float gx, gy;
    sobel_at(gray, h, w, y, x, gx, gy);
    dx[(size_t)y * w + x] = gx;
    dy[(size_t)y * w + x] = gy;
}

// cv2.GaussianBlur of features.py:24 in the operation order of OpenCV's sepFilter2D, multiply and
// add rounded separately (the Makefile's -ffp-contract=off keeps them apart): g_x, g_y and the
// blurred plane decide theta and the tiles, which are held to the model bit for bit, so they
// cannot take pano_blur_plane's one-FMA-per-tap sums (those differ in the last bit).
struct SmoothTaps {
    float k[PANO_MSOP_SMOOTH_TAPS];
    int n;
};

// NT: the aperture when it is one of gaussian_filter's two (5, 11), so that the tap loops unroll
// and the taps stay in scalar registers; 0: t.n decides.  Only a pixel within the radius of the
// border pays for reflect_101; the order of the operations is the same on both paths.
// row pass: s = k[0] x[0]; s += k[j] x[j], j ascending, REFLECT_101
template <int NT>
__global__ __launch_bounds__(256) void smooth_rows_kernel(const float *__restrict__ src, int h,
                                                          int w, SmoothTaps t,
                                                          float *__restrict__ dst) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const float *row = src + (size_t)y * w;
    const int n = NT ? NT : t.n, r = n >> 1;
    float s;
    if (x >= r && x + r < w) {
        const float *p = row + (x - r);
        s = p[0] * t.k[0];
        for (int j = 1; j < n; ++j) s = s + p[j] * t.k[j];
    } else {
        s = row[reflect_101(x - r, w)] * t.k[0];
        for (int j = 1; j < n; ++j) s = s + row[reflect_101(x - r + j, w)] * t.k[j];
    }
    dst[(size_t)y * w + x] = s;
}

// column pass, the symmetric engine: s = k[r] y[0]; s += k[r + j] (y[+j] + y[-j]), j = 1 .. r
template <int NT>
__global__ __launch_bounds__(256) void smooth_cols_kernel(const float *__restrict__ src, int h,
                                                          int w, SmoothTaps t,
                                                          float *__restrict__ dst) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const int n = NT ? NT : t.n, r = n >> 1;
    const float *col = src + x;
    const bool inner = y >= r && y + r < h;
    float s = col[(size_t)y * w] * t.k[r];
    for (int j = 1; j <= r; ++j) {
        const int yb = inner ? y + j : reflect_101(y + j, h);
        const int ya = inner ? y - j : reflect_101(y - j, h);
        s = s + (col[(size_t)yb * w] + col[(size_t)ya * w]) * t.k[r + j];
    }
    dst[(size_t)y * w + x] = s;
}

template <int NT>
void launch_smooth(hipStream_t s, const float *src, int h, int w, const SmoothTaps &t, float *tmp,
                   float *dst) {
    const dim3 grid(ceil_div(w, 64), ceil_div(h, 4)), block(64, 4);
    hipLaunchKernelGGL(smooth_rows_kernel<NT>, grid, block, 0, s, src, h, w, t, tmp);
    hipLaunchKernelGGL(smooth_cols_kernel<NT>, grid, block, 0, s, tmp, h, w, t, dst);
}

// float -> uint32 whose unsigned order is the float's order, -0 counted as +0 (sift_sort.hip)
__device__ __forceinline__ uint32_t ordered(float v) {
    const uint32_t b = __float_as_uint(v + 0.0f);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

// 1 = the pixel is >= its 8 neighbours (maximum_filter(size 3) == hrs; SciPy's `reflect` border
// repeats the edge, so what lies outside adds nothing to the neighbourhood)
__global__ __launch_bounds__(256) void local_max_kernel(const float *__restrict__ hrs, int h, int w,
                                                        int *__restrict__ flags) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= w || y >= h) return;
    const float v = hrs[(size_t)y * w + x];
    bool keep = v == v;
    for (int oy = -1; oy <= 1; ++oy)
        for (int ox = -1; ox <= 1; ++ox) {
            const int yy = y + oy, xx = x + ox;
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            keep = keep && v >= hrs[(size_t)yy * w + xx];
        }
    flags[(size_t)y * w + x] = keep ? 1 : 0;
}

__global__ __launch_bounds__(256) void compact_kernel(const float *__restrict__ hrs,
                                                      const int *__restrict__ flags,
                                                      const int *__restrict__ slot, int n,
                                                      uint32_t *__restrict__ keys,
                                                      uint32_t *__restrict__ pos,
                                                      int *__restrict__ count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) *count = slot[i] + flags[i];
    if (!flags[i]) return;
    keys[slot[i]] = ordered(hrs[i]);
    pos[slot[i]] = (uint32_t)i;
}

// the last `keep` of the n sorted candidates as (row, col), weakest first
__global__ __launch_bounds__(256) void cut_tail_kernel(const uint32_t *__restrict__ pos, int n,
                                                       int keep, int w, int32_t *__restrict__ pts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= keep) return;
    const uint32_t p = pos[n - keep + i];
    pts[2 * i] = (int32_t)(p / (uint32_t)w);
    pts[2 * i + 1] = (int32_t)(p % (uint32_t)w);
}

struct CandLayout {
    size_t temp_bytes, flags, slot, total;
};

CandLayout cand_layout(size_t n) {
    CandLayout L = {};
    int *iu = nullptr;
    size_t scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, iu, iu, 0, n, rocprim::plus<int>());
    L.temp_bytes = align_up(scan_bytes);
    L.flags = L.temp_bytes;
    L.slot = L.flags + align_up(n * 4);
    L.total = L.slot + align_up(n * 4);
    return L;
}

struct CutLayout {
    size_t temp_bytes, keys, pos, total;
};

CutLayout cut_layout(size_t n) {
    CutLayout L = {};
    uint32_t *ku = nullptr;
    size_t sort_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, ku, ku, ku, ku, n, 0u, 32u);
    L.temp_bytes = align_up(sort_bytes);
    L.keys = L.temp_bytes;
    L.pos = L.keys + align_up(n * 4);
    L.total = L.pos + align_up(n * 4);
    return L;
}

// One greedy walk of ssc (features.py:71-89) by ONE wave, 64 points a step.  The walk is serial
// only through the coverage bitmap, and a taken point changes it only within `reach` cells of its
// own: so each lane looks its cell up once per step, the first uncovered lane is taken (ballot),
// its cell is broadcast (shuffle), the lanes it covers drop out by comparing coordinates - no
// memory round trip - and the next uncovered lane follows.  Only then the taken lanes' blocks are
// ORed into the bitmap, by all lanes together.  ONCHIP: the bitmap is in LDS; else in `gbits`
// (zeroed by the caller), read past the L1 and fenced after every step that wrote.
template <bool ONCHIP>
__global__ __launch_bounds__(64) void ssc_probe_kernel(const int32_t *__restrict__ pts, int n,
                                                       double cgr, int ncr, int ncc, int reach,
                                                       uint32_t *gbits, int32_t *__restrict__ sel,
                                                       int32_t *__restrict__ count) {
    __shared__ uint32_t lbits[ONCHIP ? SSC_LDS_WORDS : 1];
    const int lane = threadIdx.x;
    const size_t stride = (size_t)ncc + 1;
    if (ONCHIP) {
        const size_t words = (((size_t)ncr + 1) * stride + 31) / 32;
        for (size_t q = lane; q < words; q += 64) lbits[q] = 0;
        __syncthreads();
    }
    const int side = 2 * reach + 1;
    int taken = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        int r = -1, c = -1;
        bool open = false;
        if (i < n) {
            // the reference's swap: the cell row comes from kpt[1], the cell column from kpt[0]
            r = (int)floor((double)pts[2 * i + 1] / cgr);
            c = (int)floor((double)pts[2 * i] / cgr);
            if (r >= 0 && r <= ncr && c >= 0 && c <= ncc) {
                const size_t cell = (size_t)r * stride + c;
                const uint32_t word =
                    ONCHIP ? lbits[cell >> 5]
                           : __hip_atomic_load(&gbits[cell >> 5], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                open = !((word >> (cell & 31)) & 1u);
            }
        }
        unsigned long long todo = __ballot(open), chosen = 0;
        while (todo) {
            const int first = __ffsll(todo) - 1;
            const int r0 = __shfl(r, first), c0 = __shfl(c, first);
            chosen |= 1ull << first;
            const bool near = abs(r - r0) <= reach && abs(c - c0) <= reach;
            todo &= ~__ballot(near);
        }
        if (!chosen) continue;
        if ((chosen >> lane) & 1ull)
            sel[taken + __popcll(chosen & ((1ull << lane) - 1ull))] = i;
        taken += __popcll(chosen);
        for (unsigned long long m = chosen; m; m &= m - 1) {
            const int first = __ffsll(m) - 1;
            const int r0 = __shfl(r, first), c0 = __shfl(c, first);
            for (int q = lane; q < side * side; q += 64) {
                const int rr = r0 - reach + q / side, cc = c0 - reach + q % side;
                if (rr < 0 || rr > ncr || cc < 0 || cc > ncc) continue;
                const size_t cell = (size_t)rr * stride + cc;
                atomicOr(ONCHIP ? &lbits[cell >> 5] : &gbits[cell >> 5], 1u << (cell & 31));
            }
        }
        if (!ONCHIP) __threadfence();
        __syncthreads();
    }
    if (lane == 0) *count = taken;
}

// NumPy's pairwise sum of 64 contiguous float32 held one per lane (lane = index): 8 strided
// accumulators r[j] = t[j] + t[8 + j] + ... in order, then ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)).
// (Not wave.h's wave_sum, whose butterfly adds in another order.)
__device__ __forceinline__ float sum64(float t, int lane) {
    const int u = lane & 7;
    float acc = __shfl(t, u);
#pragma unroll
    for (int v = 1; v < 8; ++v) acc = acc + __shfl(t, 8 * v + u);
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = __shfl(acc, j);
    return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
}

// features.py:116-128 for one point per wave; lane 8v + u samples tap (u, v) of the tile
__global__ __launch_bounds__(256) void describe_kernel(
    const float *__restrict__ gx, const float *__restrict__ gy, const float *__restrict__ blurred,
    int h, int w, const int32_t *__restrict__ pts, const int32_t *__restrict__ sel, int n,
    int scale, double *__restrict__ points, float *__restrict__ theta_out,
    float *__restrict__ tiles, float *__restrict__ desc) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    const int src = sel ? sel[p] : p;
    const int r = pts[2 * src], c = pts[2 * src + 1];
    if (r < 0 || r >= h || c < 0 || c >= w) return;       // (not a pixel: nothing to describe)
    // the reference's quirk: dx is the first argument
    const float theta = atan2f(gx[(size_t)r * w + c], gy[(size_t)r * w + c]);
    const double cs = (double)(float)cos((double)theta), sn = (double)(float)sin((double)theta);
    const double u = (double)((lane & 7) - 4), v = (double)((lane >> 3) - 4);
    const double x_src = (cs * u + sn * v) + (double)c;
    const double y_src = (-sn * u + cs * v) + (double)r;
    // OpenCV's fixed-point sampling: 5 fraction bits, the weights as float32 products
    const long long X = llrint(32.0 * x_src), Y = llrint(32.0 * y_src);
    const long long sx = X >> 5, sy = Y >> 5;
    const float ax = (float)(int)(X & 31) * 0.03125f, ay = (float)(int)(Y & 31) * 0.03125f;
    auto tap = [&](long long yy, long long xx) -> float {
        return (yy >= 0 && yy < h && xx >= 0 && xx < w) ? blurred[(size_t)yy * w + (size_t)xx]
                                                        : 0.0f;
    };
    float t = tap(sy, sx) * ((1.0f - ay) * (1.0f - ax));
    t = t + tap(sy, sx + 1) * ((1.0f - ay) * ax);
    t = t + tap(sy + 1, sx) * (ay * (1.0f - ax));
    t = t + tap(sy + 1, sx + 1) * (ay * ax);
    if (tiles) tiles[(size_t)p * 64 + lane] = t;
    const float mean = sum64(t, lane) / 64.0f;
    const float dev = t - mean;
    const float sd = sqrtf(sum64(dev * dev, lane) / 64.0f);
    desc[(size_t)p * 64 + lane] = (t - mean) / (sd + 1e-8f);
    if (lane == 0) {
        if (theta_out) theta_out[p] = theta;
        if (points) {
            points[4 * (size_t)p] = (double)scale * (double)r;
            points[4 * (size_t)p + 1] = (double)scale * (double)c;
            points[4 * (size_t)p + 2] = (double)theta;
            points[4 * (size_t)p + 3] = (double)scale;
        }
    }
}

}  // namespace

extern "C" int pano_harris(pano_ctx *ctx, const float *gray, int h, int w, float k, float *out) {
    PANO_ENTER(ctx, "pano_harris");
    PANO_REQUIRE(gray && out && gray != out && h > 0 && w > 0, "pano_harris: bad argument");
    hipLaunchKernelGGL(harris_kernel, dim3(ceil_div(w, HT_W), ceil_div(h, HT_H)),
                       dim3(HT_W, HT_H), 0, (hipStream_t)stream, gray, h, w, k, out);
    PANO_LAUNCH_CHECK("harris_kernel");
    return PANO_OK;
}

extern "C" int pano_sobel(pano_ctx *ctx, const float *gray, int h, int w, float *dx, float *dy) {
    PANO_ENTER(ctx, "pano_sobel");
    PANO_REQUIRE(gray && dx && dy && dx != dy && gray != dx && gray != dy && h > 0 && w > 0,
                 "pano_sobel: bad argument");
    hipLaunchKernelGGL(sobel_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4)), dim3(64, 4), 0,
                       (hipStream_t)stream, gray, h, w, dx, dy);
    PANO_LAUNCH_CHECK("sobel_kernel");
    return PANO_OK;
}

extern "C" int pano_msop_smooth(pano_ctx *ctx, const float *src, int h, int w, const float *taps,
                                int ntaps, float *tmp, float *dst) {
    PANO_ENTER(ctx, "pano_msop_smooth");
    PANO_REQUIRE(src && taps && tmp && dst && tmp != src && tmp != dst && h > 0 && w > 0,
                 "pano_msop_smooth: bad argument");
    PANO_REQUIRE(ntaps >= 1 && (ntaps & 1) && ntaps <= PANO_MSOP_SMOOTH_TAPS,
                 "pano_msop_smooth: aperture %d must be odd and within [1, %d]", ntaps,
                 PANO_MSOP_SMOOTH_TAPS);
    SmoothTaps t = {};
    t.n = ntaps;
    for (int j = 0; j < ntaps; ++j) t.k[j] = taps[j];
    if (ntaps == 5)
        launch_smooth<5>((hipStream_t)stream, src, h, w, t, tmp, dst);
    else if (ntaps == 11)
        launch_smooth<11>((hipStream_t)stream, src, h, w, t, tmp, dst);
    else
        launch_smooth<0>((hipStream_t)stream, src, h, w, t, tmp, dst);
    PANO_LAUNCH_CHECK("smooth_cols_kernel");
    return PANO_OK;
}

extern "C" size_t pano_msop_candidates_work_bytes(int h, int w) {
    return cand_layout(h > 0 && w > 0 ? (size_t)h * w : 1).total;
}

extern "C" int pano_msop_candidates(pano_ctx *ctx, const float *hrs, int h, int w, void *work,
                                    uint32_t *keys, uint32_t *pos, int *count) {
    PANO_ENTER(ctx, "pano_msop_candidates");
    PANO_REQUIRE(hrs && work && keys && pos && count && h > 0 && w > 0,
                 "pano_msop_candidates: bad argument");
    PANO_REQUIRE((size_t)h * w < ((size_t)1 << 31), "pano_msop_candidates: %d x %d is too large",
                 h, w);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)h * w;
    const CandLayout L = cand_layout(n);
    unsigned char *base = (unsigned char *)work;
    int *flags = (int *)(base + L.flags), *slot = (int *)(base + L.slot);
    hipLaunchKernelGGL(local_max_kernel, dim3(ceil_div(w, 64), ceil_div(h, 4)), dim3(64, 4), 0, s,
                       hrs, h, w, flags);
    PANO_LAUNCH_CHECK("local_max_kernel");
    size_t temp = L.temp_bytes;
    PANO_HIP(rocprim::exclusive_scan(base, temp, flags, slot, 0, n, rocprim::plus<int>(), s));
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hrs,
                       flags, slot, (int)n, keys, pos, count);
    PANO_LAUNCH_CHECK("compact_kernel");
    return PANO_OK;
}

extern "C" size_t pano_msop_cut_work_bytes(int n) { return cut_layout(n > 0 ? n : 1).total; }

extern "C" int pano_msop_cut(pano_ctx *ctx, const uint32_t *keys, const uint32_t *pos, int n,
                             int keep, int w, void *work, int32_t *points) {
    PANO_ENTER(ctx, "pano_msop_cut");
    PANO_REQUIRE(n >= 0 && keep >= 0 && keep <= n && w > 0, "pano_msop_cut: bad argument");
    if (keep == 0) return PANO_OK;
    PANO_REQUIRE(keys && pos && work && points, "pano_msop_cut: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const CutLayout L = cut_layout((size_t)n);
    unsigned char *base = (unsigned char *)work;
    uint32_t *keys_b = (uint32_t *)(base + L.keys), *pos_b = (uint32_t *)(base + L.pos);
    size_t temp = L.temp_bytes;
    // stable: equal responses keep the compaction's row-major order
    PANO_HIP(rocprim::radix_sort_pairs(base, temp, keys, keys_b, pos, pos_b, (size_t)n, 0u, 32u, s));
    hipLaunchKernelGGL(cut_tail_kernel, dim3(ceil_div(keep, 256)), dim3(256), 0, s, pos_b, n, keep,
                       w, points);
    PANO_LAUNCH_CHECK("cut_tail_kernel");
    return PANO_OK;
}

static size_t ssc_words(int n_cell_rows, int n_cell_cols) {
    return (((size_t)n_cell_rows + 1) * ((size_t)n_cell_cols + 1) + 31) / 32;
}

extern "C" size_t pano_ssc_probe_work_bytes(int n_cell_rows, int n_cell_cols) {
    if (n_cell_rows < 0 || n_cell_cols < 0) return 0;
    return align_up(ssc_words(n_cell_rows, n_cell_cols) * 4);
}

extern "C" int pano_ssc_probe(pano_ctx *ctx, const int32_t *points, int n, double cgr,
                              int n_cell_rows, int n_cell_cols, int reach, int path, void *work,
                              int32_t *sel, int32_t *count) {
    PANO_ENTER(ctx, "pano_ssc_probe");
    PANO_REQUIRE(n >= 0 && count && cgr > 0.0 && n_cell_rows >= 0 && n_cell_cols >= 0 &&
                     reach >= 0 && reach <= 1024,
                 "pano_ssc_probe: bad argument");
    PANO_REQUIRE(path >= PANO_SSC_AUTO && path <= PANO_SSC_GLOBAL, "pano_ssc_probe: path %d", path);
    PANO_REQUIRE(n == 0 || (points && sel), "pano_ssc_probe: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const size_t words = ssc_words(n_cell_rows, n_cell_cols);
    PANO_REQUIRE(words <= ((size_t)1 << 28), "pano_ssc_probe: a grid of %d x %d cells is too large",
                 n_cell_rows + 1, n_cell_cols + 1);
    const bool fits = words <= (size_t)SSC_LDS_WORDS;
    PANO_REQUIRE(path != PANO_SSC_ONCHIP || fits,
                 "pano_ssc_probe: %zu bitmap words do not fit the on-chip path (%d)", words,
                 SSC_LDS_WORDS);
    if (path == PANO_SSC_ONCHIP || (path == PANO_SSC_AUTO && fits)) {
        hipLaunchKernelGGL(ssc_probe_kernel<true>, dim3(1), dim3(64), 0, s, points, n, cgr,
                           n_cell_rows, n_cell_cols, reach, (uint32_t *)nullptr, sel, count);
    } else {
        PANO_REQUIRE(work, "pano_ssc_probe: the global path needs its scratch");
        PANO_HIP(hipMemsetAsync(work, 0, words * 4, s));
        hipLaunchKernelGGL(ssc_probe_kernel<false>, dim3(1), dim3(64), 0, s, points, n, cgr,
                           n_cell_rows, n_cell_cols, reach, (uint32_t *)work, sel, count);
    }
    PANO_LAUNCH_CHECK("ssc_probe_kernel");
    return PANO_OK;
}

extern "C" int pano_msop_describe(pano_ctx *ctx, const float *gx, const float *gy,
                                  const float *blurred, int h, int w, const int32_t *points,
                                  const int32_t *sel, int n, int scale, double *points_out,
                                  float *theta, float *tiles, float *desc) {
    PANO_ENTER(ctx, "pano_msop_describe");
    PANO_REQUIRE(n >= 0 && h > 0 && w > 0 && scale > 0, "pano_msop_describe: bad argument");
    if (n == 0) return PANO_OK;
    PANO_REQUIRE(gx && gy && blurred && points && desc, "pano_msop_describe: null pointer");
    hipLaunchKernelGGL(describe_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream,
                       gx, gy, blurred, h, w, points, sel, n, scale, points_out, theta, tiles,
                       desc);
    PANO_LAUNCH_CHECK("describe_kernel");
    return PANO_OK;
}
