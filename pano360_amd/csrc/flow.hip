// Local alignment of overlapping frames between the warp and the blend (--local-align; DESIGN.md
// section 5u).  The contract - grey and validity levels on the mosaic's grid, pairs, the block
// search coarse to fine with its tie and hysteresis rules, the median smoothing, the field per
// pixel and the apply - is in include/pano360.h; tests/flow_model.py restates all of it in NumPy.
// Integers up to the block vectors; the two float32 stages do one rounding per operation in the
// header's order (the Makefile's -ffp-contract=off), so the same input gives the model's bytes.
//
// One record table (batch.h's slots) is uploaded once per call and every launch reads a section:
//   flow_pyramid_kernel   a 16 x 16 tile of a camera's box -> grey | valid << 8 of level 0 and, in
//                         LDS, the tile's samples of the levels above (the levels nest), stored
//   flow_search_kernel    one launch per level L .. 0, a wave per (pair, block): 16 x 16 samples
//                         of i and the 18 x 18 window of j round s + v in LDS, nine counts and nine
//                         sums by wave_sum, every lane takes the decision and lane 0 stores it
//   flow_smooth_kernel    a thread per level-0 block: the lower median by rank counting
//   flow_apply_kernel     a thread per patch pixel of every camera with a partner
// No atomics on floats; the two pixel counts of the statistics are integer sums.
#include <cstring>

#include "batch.h"
#include "wave.h"

#define FLOW_LEVELS (PANO_FLOW_MAX_LEVELS + 1)

struct FlowCam {                    // a camera of the call, in device memory
    const float *planes;            // [4][h][pitch]
    const uint8_t *mask;            // [h][w]
    float *out;                     // [4][h][pitch], or null
    uint16_t *gv[FLOW_LEVELS];      // level l of its box: [bh >> l][bw >> l], grey | valid << 8
    int y0, x0, h, w, pitch;
    int ay0, ax0, bh, bw;           // the box: the rect grown to multiples of 16 mosaic pixels
    int top;                        // the levels 0 .. top are stored
    int part0, nparts;              // its partners in the partner table, by camera index
    TileSlot slot;
};

struct FlowPair {                   // a pair (at a level) of a launch
    int i, j, L, level;
    int by0[FLOW_LEVELS], bx0[FLOW_LEVELS], nby[FLOW_LEVELS], nbx[FLOW_LEVELS];
    int16_t *vec[FLOW_LEVELS];      // [nby][nbx][4] = (dx, dy, known, 0)
    int16_t *smooth;                // [nby[0]][nbx[0]][2]
    TileSlot slot;
};

struct FlowPart {                   // a partner of a camera: F_cj = sign * F of the pair
    const int16_t *smooth;
    int j, by0, bx0, nby, nbx;
    float sign;
};

__device__ __forceinline__ int flow_quant(float v) { return (uint8_t)(int)(255.0f * v); }

// sample (y, x) of level l of a camera: 0 (invalid) outside its box
__device__ __forceinline__ uint32_t flow_sample(const FlowCam &C, int l, int y, int x) {
    const int ry = y - (C.ay0 >> l), rx = x - (C.ax0 >> l), bw = C.bw >> l;
    if ((unsigned)ry >= (unsigned)(C.bh >> l) || (unsigned)rx >= (unsigned)bw) return 0u;
    return C.gv[l][(size_t)ry * bw + rx];
}

// ---- grey, validity, levels ------------------------------------------------------------------
__global__ __launch_bounds__(256) void flow_pyramid_kernel(const FlowCam *__restrict__ table, int n) {
    __shared__ uint16_t s[256 + 64 + 16 + 4 + 1];
    int tile;
    const FlowCam &C = batch_record(table, n, tile);
    const int tid = threadIdx.x, tx = tile % C.slot.tiles_x, ty = tile / C.slot.tiles_x;
    {
        const int r = tid >> 4, c = tid & 15;
        const int py = C.ay0 + 16 * ty + r - C.y0, px = C.ax0 + 16 * tx + c - C.x0;
        uint32_t v = 0;
        if ((unsigned)py < (unsigned)C.h && (unsigned)px < (unsigned)C.w && C.mask[(size_t)py * C.w + px] == 0) {
            const size_t plane = (size_t)C.h * C.pitch, at = (size_t)py * C.pitch + px;
            const int q0 = flow_quant(C.planes[at]), q1 = flow_quant(C.planes[plane + at]),
                      q2 = flow_quant(C.planes[2 * plane + at]);
            v = (uint32_t)((q0 + 2 * q1 + q2 + 2) >> 2) | 256u;
        }
        s[tid] = (uint16_t)v;
        C.gv[0][(size_t)(16 * ty + r) * C.bw + 16 * tx + c] = (uint16_t)v;
    }
    int off = 0;
    for (int l = 1; l <= C.top; ++l) {
        __syncthreads();
        const int ns = 16 >> (l - 1), nd = 16 >> l, noff = off + ns * ns;
        if (tid < nd * nd) {
            const int r = tid / nd, c = tid % nd;
            const uint16_t *q = s + off + 2 * r * ns + 2 * c;
            const uint32_t a = q[0], b = q[1], d = q[ns], e = q[ns + 1];
            const uint32_t v = (((a & 255u) + (b & 255u) + (d & 255u) + (e & 255u) + 2u) >> 2) | (a & b & d & e & 256u);
            s[noff + tid] = (uint16_t)v;
            C.gv[l][(size_t)(nd * ty + r) * (C.bw >> l) + nd * tx + c] = (uint16_t)v;
        }
        off = noff;
    }
}

// ---- the search of one level -------------------------------------------------------------------
__global__ __launch_bounds__(64) void flow_search_kernel(const FlowPair *__restrict__ table, int n,
                                                         const FlowCam *__restrict__ cams, int gain) {
    __shared__ uint16_t si[256], sj[18 * 18];
    int tile;
    const FlowPair &P = batch_record(table, n, tile);
    const int l = P.level, lane = threadIdx.x;
    const int ry = tile / P.nbx[l], rx = tile % P.nbx[l];
    const int by = P.by0[l] + ry, bx = P.bx0[l] + rx;
    int vx = 0, vy = 0;
    if (l < P.L) {
        const int16_t *up = P.vec[l + 1] +
                            4 * ((size_t)((by >> 1) - P.by0[l + 1]) * P.nbx[l + 1] + ((bx >> 1) - P.bx0[l + 1]));
        vx = 2 * up[0], vy = 2 * up[1];
    }
    const FlowCam &A = cams[P.i], &B = cams[P.j];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        si[e] = (uint16_t)flow_sample(A, l, 16 * by + (e >> 4), 16 * bx + (e & 15));
    }
    for (int e = lane; e < 18 * 18; e += 64)
        sj[e] = (uint16_t)flow_sample(B, l, 16 * by + vy - 1 + e / 18, 16 * bx + vx - 1 + e % 18);
    __syncthreads();
    int cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k, r = e >> 4, c = e & 15;
        const int a = si[e];
        if (!(a & 256)) continue;
#pragma unroll
        for (int q = 0; q < 9; ++q) {                   // q = 3 (dy + 1) + dx + 1
            const int idx = q == 4 ? 0 : (q < 4 ? q + 1 : q);
            const int b = sj[(r + q / 3) * 18 + c + q % 3];
            if (b & 256) {
                cnt[idx] += 1;
                sum[idx] += abs((a & 255) - (b & 255));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) cnt[k] = wave_sum(cnt[k]), sum[k] = wave_sum(sum[k]);
    int w = -1;
    int64_t Sw = 0, nw = 1;
#pragma unroll
    for (int k = 0; k < 9; ++k)
        if (cnt[k] >= PANO_FLOW_MIN_COUNT && (w < 0 || (int64_t)sum[k] * nw < Sw * (int64_t)cnt[k]))
            w = k, Sw = sum[k], nw = cnt[k];
    const int known = w >= 0;
    if (known && cnt[0] >= PANO_FLOW_MIN_COUNT) {
        const int64_t nc = cnt[0];
        if (!(16 * Sw * nc + (int64_t)gain * nw * nc <= 16 * (int64_t)sum[0] * nw)) w = 0;
    }
    if (lane == 0) {
        int dx = 0, dy = 0;
        if (w > 0) {
            const int q = w <= 4 ? w - 1 : w;
            dx = q % 3 - 1, dy = q / 3 - 1;
        }
        int16_t *dst = P.vec[l] + 4 * ((size_t)ry * P.nbx[l] + rx);
        dst[0] = (int16_t)(vx + dx), dst[1] = (int16_t)(vy + dy), dst[2] = (int16_t)known, dst[3] = 0;
    }
}

// ---- smoothing ---------------------------------------------------------------------------------
// Element (m - 1) >> 1 of the m known values in sorted order: the one with that many before it,
// equal values in neighbourhood order.
__global__ __launch_bounds__(64) void flow_smooth_kernel(const FlowPair *__restrict__ table, int n) {
    int tile;
    const FlowPair &P = batch_record(table, n, tile);
    const int nby = P.nby[0], nbx = P.nbx[0], b = tile * 64 + (int)threadIdx.x;
    if (b >= nby * nbx) return;
    const int by = b / nbx, bx = b % nbx;
    const int16_t *vec = P.vec[0];
    const int ya = max(by - 1, 0), yb = min(by + 1, nby - 1), xa = max(bx - 1, 0), xb = min(bx + 1, nbx - 1);
    int m = 0;
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x) m += vec[4 * ((size_t)y * nbx + x) + 2] != 0;
    int out[2] = {0, 0};
    if (vec[4 * (size_t)b + 2] != 0 || m >= 3) {
        const int want = (m - 1) >> 1;
        for (int c = 0; c < 2; ++c) {
            int k = 0;
            for (int y = ya; y <= yb; ++y)
                for (int x = xa; x <= xb; ++x) {
                    const int16_t *p = vec + 4 * ((size_t)y * nbx + x);
                    if (!p[2]) continue;
                    int before = 0, k2 = 0;
                    for (int y2 = ya; y2 <= yb; ++y2)
                        for (int x2 = xa; x2 <= xb; ++x2) {
                            const int16_t *p2 = vec + 4 * ((size_t)y2 * nbx + x2);
                            if (!p2[2]) continue;
                            before += p2[c] < p[c] || (p2[c] == p[c] && k2 < k);
                            ++k2;
                        }
                    if (before == want) out[c] = p[c];
                    ++k;
                }
        }
    }
    P.smooth[2 * (size_t)b] = (int16_t)out[0];
    P.smooth[2 * (size_t)b + 1] = (int16_t)out[1];
}

// ---- field and apply -----------------------------------------------------------------------------
__device__ __forceinline__ float flow_lerp(float a, float b, float f) { return a + f * (b - a); }

// index of block centre floor(t) and of the next, clamped into [lo, lo + n), relative to lo
__device__ __forceinline__ void flow_axis(int p, int lo, int n, int &a, int &b, float &f) {
    const float t = (float)(2 * p - 15) / 32.0f, fl = floorf(t);
    f = t - fl;
    const int i = (int)fl;
    a = min(max(i, lo), lo + n - 1) - lo;
    b = min(max(i + 1, lo), lo + n - 1) - lo;
}

// alpha of camera K at mosaic pixel (Y, X) where it covers it, else -1
__device__ __forceinline__ float flow_alpha(const FlowCam &K, int Y, int X) {
    const int py = Y - K.y0, px = X - K.x0;
    if ((unsigned)py >= (unsigned)K.h || (unsigned)px >= (unsigned)K.w) return -1.0f;
    if (K.mask[(size_t)py * K.w + px]) return -1.0f;
    return K.planes[3 * (size_t)K.h * K.pitch + (size_t)py * K.pitch + px];
}

__global__ __launch_bounds__(256) void flow_apply_kernel(const FlowCam *__restrict__ table, int n,
                                                         const FlowCam *__restrict__ cams, int ncams,
                                                         const FlowPart *__restrict__ parts,
                                                         int32_t *__restrict__ stats) {
    int tile;
    const FlowCam &C = batch_record(table, n, tile);
    const int x = (tile % C.slot.tiles_x) * 64 + ((int)threadIdx.x & 63);
    const int y = (tile / C.slot.tiles_x) * 4 + ((int)threadIdx.x >> 6);
    bool moved = false, valid = false;
    if (x < C.w && y < C.h) {
        const size_t plane = (size_t)C.h * C.pitch, at = (size_t)y * C.pitch + x;
        float c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = C.planes[k * plane + at];
        if (C.mask[(size_t)y * C.w + x] == 0) {
            valid = true;
            const int Y = C.y0 + y, X = C.x0 + x;
            bool any = false;
            for (int q = 0; q < C.nparts; ++q) any |= flow_alpha(cams[parts[C.part0 + q].j], Y, X) > 0.0f;
            if (any) {
                float W = 0.0f, dx = 0.0f, dy = 0.0f;
                for (int k = 0; k < ncams; ++k) {
                    const float a = flow_alpha(cams[k], Y, X);
                    if (a >= 0.0f) W = W + a;
                }
                for (int q = 0; q < C.nparts; ++q) {
                    const FlowPart &R = parts[C.part0 + q];
                    const float a = flow_alpha(cams[R.j], Y, X);
                    if (!(a > 0.0f)) continue;
                    const float share = a / W;
                    int xa, xb, ya, yb;
                    float fx, fy;
                    flow_axis(X, R.bx0, R.nbx, xa, xb, fx);
                    flow_axis(Y, R.by0, R.nby, ya, yb, fy);
                    const int16_t *r0 = R.smooth + 2 * (size_t)ya * R.nbx, *r1 = R.smooth + 2 * (size_t)yb * R.nbx;
                    float F[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const float top = flow_lerp((float)r0[2 * xa + k], (float)r0[2 * xb + k], fx);
                        const float bot = flow_lerp((float)r1[2 * xa + k], (float)r1[2 * xb + k], fx);
                        F[k] = flow_lerp(top, bot, fy);
                    }
                    dx = dx + share * (R.sign * F[0]);
                    dy = dy + share * (R.sign * F[1]);
                }
                if (dx != 0.0f || dy != 0.0f) {
                    const float sx = (float)x - dx, sy = (float)y - dy;
                    const float flx = floorf(sx), fly = floorf(sy);
                    const float fx = sx - flx, fy = sy - fly;
                    const int x0 = (int)flx, y0 = (int)fly;
                    if (x0 >= 0 && x0 + 1 < C.w && y0 >= 0 && y0 + 1 < C.h) {
                        const uint8_t *m0 = C.mask + (size_t)y0 * C.w + x0;
                        if (!(m0[0] | m0[1] | m0[C.w] | m0[C.w + 1])) {
                            const size_t a0 = (size_t)y0 * C.pitch + x0;
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const float *p = C.planes + k * plane + a0;
                                const float top = flow_lerp(p[0], p[1], fx);
                                const float bot = flow_lerp(p[C.pitch], p[C.pitch + 1], fx);
                                c[k] = flow_lerp(top, bot, fy);
                            }
                            moved = true;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) C.out[k * plane + at] = c[k];
    }
    const uint64_t mm = __ballot(moved), mv = __ballot(valid);
    if ((threadIdx.x & 63) == 0) {
        if (mm) atomicAdd(&stats[0], (int)__popcll(mm));
        if (mv) atomicAdd(&stats[1], (int)__popcll(mv));
    }
}

// ---- C ABI -----------------------------------------------------------------------------------
struct FlowRect {                   // a pair: its cameras, L_ij and the intersection of their rects
    int i, j, levels, y0, y1, x0, x1;
};

struct FlowPlan {                   // what a call's rects and parameters decide, and its workspace
    std::vector<FlowRect> pairs;
    std::vector<uint8_t> paired;    // [n]
    int top;
    std::vector<size_t> gv;         // [n][FLOW_LEVELS]: byte offsets of the cameras' levels
    std::vector<size_t> vec;        // [pairs][FLOW_LEVELS]
    std::vector<size_t> smooth;     // [pairs]
    size_t pyramid_bytes, vectors_at, vectors_bytes, fields_at, fields_bytes, stats_at, total;
};

static void flow_blocks(const FlowRect &p, int l, int &by0, int &bx0, int &nby, int &nbx) {
    const int s = l + 4;
    by0 = p.y0 >> s, bx0 = p.x0 >> s;
    nby = ((p.y1 - 1) >> s) - by0 + 1, nbx = ((p.x1 - 1) >> s) - bx0 + 1;
}

static int flow_bits(int v) {
    int bits = 0;
    while (v) ++bits, v >>= 1;
    return bits;
}

static int flow_check(const char *who, const pano_patch *host, int n, int H, int W, const pano_flow_params *P) {
    PANO_REQUIRE(host && P, "%s: null table", who);
    PANO_REQUIRE(n >= 2 && n <= 32767, "%s: %d cameras (2 .. 32767)", who, n);
    PANO_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 29), "%s: a %d x %d mosaic is outside H, W >= 1, H W <= 2^29",
                 who, H, W);
    PANO_REQUIRE(P->levels >= 0 && P->levels <= PANO_FLOW_MAX_LEVELS, "%s: levels %d (0 .. %d)", who, P->levels,
                 PANO_FLOW_MAX_LEVELS);
    PANO_REQUIRE(P->gain >= 1 && P->gain <= PANO_FLOW_MAX_GAIN, "%s: gain %d (1 .. %d)", who, P->gain, PANO_FLOW_MAX_GAIN);
    PANO_REQUIRE(P->min_overlap >= 16, "%s: min_overlap %d (>= 16)", who, P->min_overlap);
    for (int c = 0; c < n; ++c) {
        const pano_patch &p = host[c];
        PANO_REQUIRE(p.planes && p.mask, "%s: patch %d: null planes or mask", who, c);
        PANO_REQUIRE(p.h >= 1 && p.w >= 1 && p.y0 >= 0 && p.x0 >= 0 && p.y0 + (int64_t)p.h <= H && p.x0 + (int64_t)p.w <= W,
                     "%s: patch %d: its rect leaves the mosaic", who, c);
        PANO_REQUIRE(p.vy0 == 0 && p.vx0 == 0 && p.vh == p.h && p.vw == p.w && p.vpitch >= p.w,
                     "%s: patch %d is not a stage-level patch (its window is not the whole patch)", who, c);
    }
    return PANO_OK;
}

static FlowPlan flow_plan(const pano_patch *host, int n, const pano_flow_params &P) {
    FlowPlan F;
    F.paired.assign(n, 0);
    F.top = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const pano_patch &a = host[i], &b = host[j];
            FlowRect p = {};
            p.i = i, p.j = j;
            p.y0 = a.y0 > b.y0 ? a.y0 : b.y0, p.y1 = a.y0 + a.h < b.y0 + b.h ? a.y0 + a.h : b.y0 + b.h;
            p.x0 = a.x0 > b.x0 ? a.x0 : b.x0, p.x1 = a.x0 + a.w < b.x0 + b.w ? a.x0 + a.w : b.x0 + b.w;
            if (p.y1 - p.y0 < P.min_overlap || p.x1 - p.x0 < P.min_overlap) continue;
            const int side = p.y1 - p.y0 < p.x1 - p.x0 ? p.y1 - p.y0 : p.x1 - p.x0;
            const int L = flow_bits(side) > 6 ? flow_bits(side) - 6 : 0;
            p.levels = L < P.levels ? L : P.levels;
            F.top = p.levels > F.top ? p.levels : F.top;
            F.paired[i] = F.paired[j] = 1;
            F.pairs.push_back(p);
        }
    size_t at = 0;
    F.gv.assign((size_t)n * FLOW_LEVELS, 0);
    for (int c = 0; c < n; ++c) {
        if (!F.paired[c]) continue;
        const pano_patch &p = host[c];
        const size_t bh = ((p.y0 + p.h + 15) & ~15) - (p.y0 & ~15), bw = ((p.x0 + p.w + 15) & ~15) - (p.x0 & ~15);
        for (int l = 0; l <= F.top; ++l) {
            F.gv[(size_t)c * FLOW_LEVELS + l] = at;
            at += 2 * (bh >> l) * (bw >> l);
        }
    }
    F.pyramid_bytes = at;
    F.vectors_at = at = align_up(at);
    F.vec.assign(F.pairs.size() * FLOW_LEVELS, 0);
    for (size_t q = 0; q < F.pairs.size(); ++q)
        for (int l = 0; l <= F.pairs[q].levels; ++l) {
            int by0, bx0, nby, nbx;
            flow_blocks(F.pairs[q], l, by0, bx0, nby, nbx);
            F.vec[q * FLOW_LEVELS + l] = at;
            at += (size_t)8 * nby * nbx;
        }
    F.vectors_bytes = at - F.vectors_at;
    F.fields_at = at = align_up(at);
    F.smooth.assign(F.pairs.size(), 0);
    for (size_t q = 0; q < F.pairs.size(); ++q) {
        int by0, bx0, nby, nbx;
        flow_blocks(F.pairs[q], 0, by0, bx0, nby, nbx);
        F.smooth[q] = at;
        at += (size_t)4 * nby * nbx;
    }
    F.fields_bytes = at - F.fields_at;
    F.stats_at = align_up(at);
    F.total = F.stats_at + 256;
    return F;
}

extern "C" size_t pano_flow_work_bytes(const pano_patch *patches_host, int n, int H, int W,
                                       const pano_flow_params *params) {
    if (flow_check("pano_flow_work_bytes", patches_host, n, H, W, params)) return 0;
    return flow_plan(patches_host, n, *params).total;
}

enum { FLOW_PYRAMID = 1, FLOW_SEARCH = 2, FLOW_SMOOTH = 4, FLOW_APPLY = 8 };

template <class Rec>
static bool flow_slot(Rec &R, int &blocks, int tiles_x, int64_t tiles) {
    R.slot.tiles_x = tiles_x, R.slot.block0 = blocks;
    if (blocks + tiles > 0x7fffffff) return false;
    blocks += (int)tiles;
    return true;
}

static int flow_run(pano_ctx *ctx, const char *who, int stages, const pano_patch *host, int n,
                    int H, int W, const pano_flow_params *params, void *work, int64_t work_bytes, float *const *out,
                    uint16_t *pyramid_out, int16_t *vectors_out, int16_t *fields_out, int32_t *stats_out) {
    PANO_ENTER(ctx, who);
    if (int rc = flow_check(who, host, n, H, W, params)) return rc;
    PANO_REQUIRE(work && work_bytes >= 0, "%s: no workspace", who);
    const FlowPlan F = flow_plan(host, n, *params);
    PANO_REQUIRE(F.total <= (size_t)work_bytes, "%s: the patches need a workspace of %zu bytes, %lld given", who, F.total,
                 (long long)work_bytes);
    if (stages & FLOW_APPLY) {
        PANO_REQUIRE(out, "%s: null output table", who);
        for (int c = 0; c < n; ++c)
            PANO_REQUIRE(!F.paired[c] || (out[c] && out[c] != host[c].planes), "%s: patch %d: no output planes of its own",
                         who, c);
    }
    const hipStream_t s = (hipStream_t)stream;
    char *base = (char *)work;
    const int np = (int)F.pairs.size();

    // the records: cameras by index, then a section per launch
    std::vector<FlowCam> cams((size_t)n);
    std::vector<FlowPart> parts;
    for (int c = 0; c < n; ++c) {
        const pano_patch &p = host[c];
        FlowCam &C = cams[c];
        C = FlowCam{};
        C.planes = p.planes, C.mask = p.mask, C.out = out && F.paired[c] ? out[c] : nullptr;
        C.y0 = p.y0, C.x0 = p.x0, C.h = p.h, C.w = p.w, C.pitch = p.vpitch;
        C.ay0 = p.y0 & ~15, C.ax0 = p.x0 & ~15;
        C.bh = ((p.y0 + p.h + 15) & ~15) - C.ay0, C.bw = ((p.x0 + p.w + 15) & ~15) - C.ax0;
        C.top = F.top;
        for (int l = 0; l <= F.top; ++l) C.gv[l] = (uint16_t *)(base + F.gv[(size_t)c * FLOW_LEVELS + l]);
        C.part0 = (int)parts.size();
        // (the pairs are sorted by (i, j): the pairs (k, c), k < c, precede the pairs (c, k), so a
        // camera's partners ascend by index, the order of the contract's sum)
        for (int q = 0; q < np; ++q) {
            const FlowRect &p2 = F.pairs[q];
            if (p2.i != c && p2.j != c) continue;
            FlowPart R = {};
            R.smooth = (const int16_t *)(base + F.smooth[q]);
            R.j = p2.i == c ? p2.j : p2.i;
            R.sign = p2.i == c ? 1.0f : -1.0f;
            flow_blocks(p2, 0, R.by0, R.bx0, R.nby, R.nbx);
            parts.push_back(R);
        }
        C.nparts = (int)parts.size() - C.part0;
    }
    std::vector<FlowCam> pyr, app;
    int pyr_blocks = 0, app_blocks = 0;
    bool fits = true;
    for (int c = 0; c < n; ++c) {
        if (!F.paired[c]) continue;
        FlowCam C = cams[c];
        fits &= flow_slot(C, pyr_blocks, C.bw / 16, (int64_t)(C.bw / 16) * (C.bh / 16));
        pyr.push_back(C);
        fits &= flow_slot(C, app_blocks, ceil_div(C.w, 64), (int64_t)ceil_div(C.w, 64) * ceil_div(C.h, 4));
        app.push_back(C);
    }
    std::vector<FlowPair> search[FLOW_LEVELS], smooth;
    int search_blocks[FLOW_LEVELS] = {}, smooth_blocks = 0;
    for (int q = 0; q < np; ++q) {
        FlowPair R = {};
        R.i = F.pairs[q].i, R.j = F.pairs[q].j, R.L = F.pairs[q].levels;
        for (int l = 0; l <= R.L; ++l) {
            flow_blocks(F.pairs[q], l, R.by0[l], R.bx0[l], R.nby[l], R.nbx[l]);
            R.vec[l] = (int16_t *)(base + F.vec[(size_t)q * FLOW_LEVELS + l]);
        }
        R.smooth = (int16_t *)(base + F.smooth[q]);
        for (int l = 0; l <= R.L; ++l) {
            R.level = l;
            fits &= flow_slot(R, search_blocks[l], R.nbx[l], (int64_t)R.nbx[l] * R.nby[l]);
            search[l].push_back(R);
        }
        R.level = 0;
        const int64_t nblk = (int64_t)R.nbx[0] * R.nby[0];
        fits &= flow_slot(R, smooth_blocks, (int)ceil_div(nblk, 64), ceil_div(nblk, 64));
        smooth.push_back(R);
    }
    PANO_REQUIRE(fits, "%s: more workgroups than a launch holds", who);

    PANO_HIP(hipMemsetAsync(base + F.stats_at, 0, 256, s));
    if (np) {
        std::vector<char> bytes;
        auto put = [&bytes](const void *p, size_t nbytes) {
            const size_t at = bytes.size();
            bytes.resize(at + (nbytes + 15) / 16 * 16);
            if (nbytes) memcpy(bytes.data() + at, p, nbytes);
            return at;
        };
        const size_t cams_at = put(cams.data(), cams.size() * sizeof(FlowCam));
        const size_t parts_at = put(parts.data(), parts.size() * sizeof(FlowPart));
        const size_t pyr_at = put(pyr.data(), pyr.size() * sizeof(FlowCam));
        const size_t app_at = put(app.data(), app.size() * sizeof(FlowCam));
        size_t search_at[FLOW_LEVELS];
        for (int l = 0; l <= F.top; ++l) search_at[l] = put(search[l].data(), search[l].size() * sizeof(FlowPair));
        const size_t smooth_at = put(smooth.data(), smooth.size() * sizeof(FlowPair));
        if (int rc = pano_buf_upload(ctx, BUF_FLOW_DEV, bytes.data(), bytes.size(), s)) return rc;
        const char *tab = (const char *)ctx->buf[BUF_FLOW_DEV].p;
        const FlowCam *cams_dev = (const FlowCam *)(tab + cams_at);
        if (stages & FLOW_PYRAMID) {
            hipLaunchKernelGGL(flow_pyramid_kernel, dim3((unsigned)pyr_blocks), dim3(256), 0, s,
                               (const FlowCam *)(tab + pyr_at), (int)pyr.size());
            PANO_LAUNCH_CHECK("flow_pyramid_kernel");
        }
        if (stages & FLOW_SEARCH)
            for (int l = F.top; l >= 0; --l) {
                if (search[l].empty()) continue;
                hipLaunchKernelGGL(flow_search_kernel, dim3((unsigned)search_blocks[l]), dim3(64), 0, s,
                                   (const FlowPair *)(tab + search_at[l]), (int)search[l].size(), cams_dev, params->gain);
                PANO_LAUNCH_CHECK("flow_search_kernel");
            }
        if (stages & FLOW_SMOOTH) {
            hipLaunchKernelGGL(flow_smooth_kernel, dim3((unsigned)smooth_blocks), dim3(64), 0, s,
                               (const FlowPair *)(tab + smooth_at), (int)smooth.size());
            PANO_LAUNCH_CHECK("flow_smooth_kernel");
        }
        if (stages & FLOW_APPLY) {
            hipLaunchKernelGGL(flow_apply_kernel, dim3((unsigned)app_blocks), dim3(256), 0, s,
                               (const FlowCam *)(tab + app_at), (int)app.size(), cams_dev, n,
                               (const FlowPart *)(tab + parts_at), (int32_t *)(base + F.stats_at));
            PANO_LAUNCH_CHECK("flow_apply_kernel");
        }
    }
    // the stages a test asked for, out of the workspace: each region as it lies there
    if (pyramid_out && F.pyramid_bytes)
        PANO_HIP(hipMemcpyAsync(pyramid_out, base, F.pyramid_bytes, hipMemcpyDeviceToDevice, s));
    if (vectors_out && F.vectors_bytes)
        PANO_HIP(hipMemcpyAsync(vectors_out, base + F.vectors_at, F.vectors_bytes, hipMemcpyDeviceToDevice, s));
    if (fields_out && F.fields_bytes)
        PANO_HIP(hipMemcpyAsync(fields_out, base + F.fields_at, F.fields_bytes, hipMemcpyDeviceToDevice, s));
    if (stats_out)
        PANO_HIP(hipMemcpyAsync(stats_out, base + F.stats_at, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return PANO_OK;
}

extern "C" int pano_flow_pyramid(pano_ctx *ctx, const pano_patch *patches_host, int n,
                                 int H, int W, const pano_flow_params *params, void *work, int64_t work_bytes) {
    return flow_run(ctx, "pano_flow_pyramid", FLOW_PYRAMID, patches_host, n, H, W, params, work, work_bytes,
                    nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int pano_flow_search(pano_ctx *ctx, const pano_patch *patches_host, int n, int H,
                                int W, const pano_flow_params *params, void *work, int64_t work_bytes) {
    return flow_run(ctx, "pano_flow_search", FLOW_SEARCH, patches_host, n, H, W, params, work, work_bytes,
                    nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int pano_flow_smooth(pano_ctx *ctx, const pano_patch *patches_host, int n, int H,
                                int W, const pano_flow_params *params, void *work, int64_t work_bytes) {
    return flow_run(ctx, "pano_flow_smooth", FLOW_SMOOTH, patches_host, n, H, W, params, work, work_bytes,
                    nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int pano_flow_apply(pano_ctx *ctx, const pano_patch *patches_host, int n, int H,
                               int W, const pano_flow_params *params, void *work, int64_t work_bytes, float *const *out,
                               int32_t *stats) {
    return flow_run(ctx, "pano_flow_apply", FLOW_APPLY, patches_host, n, H, W, params, work, work_bytes, out,
                    nullptr, nullptr, nullptr, stats);
}

extern "C" int pano_flow_align(pano_ctx *ctx, const pano_patch *patches_host, int n, int H,
                               int W, const pano_flow_params *params, void *work, int64_t work_bytes, float *const *out,
                               uint16_t *pyramid, int16_t *vectors, int16_t *fields, int32_t *stats) {
    return flow_run(ctx, "pano_flow_align", FLOW_PYRAMID | FLOW_SEARCH | FLOW_SMOOTH | FLOW_APPLY, patches_host,
                    n, H, W, params, work, work_bytes, out, pyramid, vectors, fields, stats);
}
