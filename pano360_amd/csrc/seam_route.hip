// Seam routing in front of the stage-level multiband blend (-b seam).  The
// contract - runner-up, difference, open pixels, groups, the N-label priority flood and the class
// sweep that gives the heap's labels bit for bit - is in include/pano360.h;
// tests/seam_route_model.py restates all of it in NumPy, heap loop included.
//
// Flood.  In class (d, g) an open pixel that is still unlabelled, has D >= d and admits a camera
// c of group g (at most one: a pixel admits its a and its b, which are of different groups) can
// take exactly one label, c.  A 64 x 64 tile therefore loads two int16 per cell with a one-cell
// frame - the label, and that one candidate (-1: the cell is not part of this class) - which is
// all that D, a and b say about the cell while the class runs: 17 KiB a tile.  A pass walks every
// row in both directions and every column in both directions, a wave per direction and a lane
// per line, 64 cells in sequence: a cell whose candidate is the label of one of its four
// neighbours takes it, so a label crosses a whole line in one walk.  Passes repeat until one
// labels nothing; the walks look in all four directions, so one quiet pass is the fixed point.
//
// Races.  A lane reads neighbours' labels while other lanes write them, and a tile reads its
// frame while the neighbour writes its interior.  Every write to a cell stores the same value,
// its candidate, over -1, so a stale read only delays a label to the next pass or round; the
// closure is the same set whatever the timing.  No atomics in the flood, and the same input
// gives the same bytes.  (The two pixel counts of the statistics are integer sums.)
#include <vector>

#include "common.h"

#define ROUTE_TILE 64
#define ROUTE_PITCH (ROUTE_TILE + 2)
#define ROUTE_THREADS 256
#define ROUTE_OPEN (-1)
#define ROUTE_WALL (-2)

struct RouteState {                 // device memory, zeroed before a flood
    int32_t d, g, changed, done;
    int32_t class_rounds, n_front, rounds, max_rounds;
    int32_t n_open, n_moved;
    int32_t present[256];           // present[level]: an open pixel has it
};

__device__ __forceinline__ int route_quant(float v) { return (uint8_t)(int)(255.0f * v); }

// ---- runner-up, difference, open flag, pairs ------------------------------------------------
__global__ __launch_bounds__(256) void seam_route_prepare_kernel(
    const pano_patch *__restrict__ patches, int n, int H, int W,
    const int16_t *__restrict__ owner0, float ratio, int16_t *__restrict__ second,
    uint8_t *__restrict__ diff, int16_t *__restrict__ label, uint8_t *__restrict__ pairs,
    uint8_t *__restrict__ present) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t g = (size_t)y * W + x;
    const int a = owner0[g];
    float alpha_a = 0.0f, alpha_b = 0.0f;
    int b = -1;
    bool any = false, a_here = false;
    for (int i = 0; i < n; ++i) {
        const pano_patch p = patches[i];
        const int px = x - p.x0, py = y - p.y0;
        if ((unsigned)px >= (unsigned)p.w || (unsigned)py >= (unsigned)p.h) continue;
        const float al = p.planes[3 * (size_t)p.vh * p.vpitch + (size_t)py * p.vpitch + px];
        any |= p.mask[(size_t)py * p.w + px] == 0;
        if (i == a) {
            alpha_a = al;
            a_here = true;
        } else if (al > alpha_b) {      // strict: the first maximum keeps the place
            alpha_b = al;
            b = i;
        }
    }
    int D = 0;
    if (b >= 0 && a_here) {
        const pano_patch pa = patches[a], pb = patches[b];
        const size_t plane_a = (size_t)pa.vh * pa.vpitch, plane_b = (size_t)pb.vh * pb.vpitch;
        const size_t oa = (size_t)(y - pa.y0) * pa.vpitch + (x - pa.x0);
        const size_t ob = (size_t)(y - pb.y0) * pb.vpitch + (x - pb.x0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int dk = route_quant(pa.planes[c * plane_a + oa]) -
                           route_quant(pb.planes[c * plane_b + ob]);
            D = max(D, dk < 0 ? -dk : dk);
        }
    }
    int lab = ROUTE_WALL;
    if (any && a_here) {
        const float bar = ratio * alpha_a;                                   // unfused (Makefile)
        lab = a;
        if (b >= 0 && alpha_b >= bar) {
            lab = ROUTE_OPEN;
            pairs[(size_t)a * n + b] = 1;           // every writer stores the same byte
            present[D] = 1;
        }
    }
    second[g] = (int16_t)b;
    diff[g] = (uint8_t)D;
    label[g] = (int16_t)lab;
}

// ---- the rounds' bookkeeping ------------------------------------------------------------------
// the levels the open pixels have, and how many they are
__global__ __launch_bounds__(256) void seam_route_init_kernel(const int16_t *__restrict__ label,
                                                              const uint8_t *__restrict__ diff,
                                                              int n, RouteState *__restrict__ state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool open = i < n && label[i] == ROUTE_OPEN;
    if (open) state->present[diff[i]] = 1;          // every writer stores the same word
    const uint64_t m = __ballot(open);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&state->n_open, (int)__popcll(m));
}

// the highest level that occurs below `from` (inclusive), or -1
__device__ __forceinline__ int route_next_level(const RouteState *state, int from) {
    int d = from;
    while (d >= 0 && !state->present[d]) --d;
    return d;
}

__global__ void seam_route_begin_kernel(RouteState *state) {
    state->d = route_next_level(state, 255);
    state->g = 0;
    state->done = state->d < 0;
}

// after a round: the same class again if a tile changed, else the next class
__global__ void seam_route_advance_kernel(RouteState *state, int n_groups) {
    if (state->done) return;
    if (state->changed) {
        state->changed = 0;
        ++state->rounds;
        ++state->class_rounds;
        return;
    }
    if (state->class_rounds) {
        ++state->n_front;
        if (state->class_rounds > state->max_rounds) state->max_rounds = state->class_rounds;
        state->class_rounds = 0;
    }
    if (state->g + 1 < n_groups) {
        ++state->g;
        return;
    }
    const int d = route_next_level(state, state->d - 1);
    if (d < 0) {
        state->done = 1;
    } else {
        state->d = d;
        state->g = 0;
    }
}

// ---- one round: every tile floods the running class to its own fixed point ---------------------
__global__ __launch_bounds__(ROUTE_THREADS) void seam_route_flood_kernel(
    const int16_t *__restrict__ a, const int16_t *__restrict__ second,
    const uint8_t *__restrict__ diff, int16_t *label, const int32_t *__restrict__ group, int n,
    int H, int W, RouteState *state) {
    __shared__ int16_t lab[ROUTE_PITCH * ROUTE_PITCH];
    __shared__ int16_t cand[ROUTE_PITCH * ROUTE_PITCH];
    if (state->done) return;
    const int d = state->d, g = state->g;
    const int y0 = blockIdx.y * ROUTE_TILE, x0 = blockIdx.x * ROUTE_TILE;
    const int th = H - y0 < ROUTE_TILE ? H - y0 : ROUTE_TILE;
    const int tw = W - x0 < ROUTE_TILE ? W - x0 : ROUTE_TILE;
    bool mine = false;
    for (int i = threadIdx.x; i < ROUTE_PITCH * ROUTE_PITCH; i += ROUTE_THREADS) {
        const int ty = i / ROUTE_PITCH - 1, tx = i % ROUTE_PITCH - 1;
        const int y = y0 + ty, x = x0 + tx;
        int l = ROUTE_WALL, c = -1;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t p = (size_t)y * W + x;
            l = label[p];
            // the frame's cells are the neighbours' to label
            if (l == ROUTE_OPEN && ty >= 0 && ty < th && tx >= 0 && tx < tw && diff[p] >= d) {
                const int ca = a[p], cb = second[p];
                if ((unsigned)ca < (unsigned)n && group[ca] == g) c = ca;
                else if ((unsigned)cb < (unsigned)n && group[cb] == g) c = cb;
            }
        }
        lab[i] = (int16_t)l;
        cand[i] = (int16_t)c;
        mine |= c >= 0;
    }
    // most tiles hold no cell of the class (early: few levels are >= d; late: all is labelled)
    if (!__syncthreads_or(mine)) return;
    // wave 0: rows left to right, 1: rows right to left, 2: columns down, 3: columns up
    const int line = threadIdx.x & 63, dir = threadIdx.x >> 6;
    const bool rows = dir < 2;
    const int nlines = rows ? th : tw, len = rows ? tw : th;
    const int along = rows ? 1 : ROUTE_PITCH, across = rows ? ROUTE_PITCH : 1;
    const int first = ROUTE_PITCH + 1 + line * across + ((dir & 1) ? (len - 1) * along : 0);
    const int step = (dir & 1) ? -along : along;
    // other lanes and waves write labels while this one reads them: every access of a pass goes to
    // LDS as written (volatile), none is kept in a register or merged across the walk
    volatile int16_t *const live = lab;
    bool worked = false;
    for (;;) {
        bool any = false;
        if (line < nlines) {
            int idx = first;
            for (int k = 0; k < len; ++k, idx += step) {
                const int c = cand[idx];
                if (c < 0 || live[idx] != ROUTE_OPEN) continue;
                if (live[idx - 1] == c || live[idx + 1] == c || live[idx - ROUTE_PITCH] == c ||
                    live[idx + ROUTE_PITCH] == c) {
                    live[idx] = (int16_t)c;
                    any = true;
                }
            }
        }
        if (!__syncthreads_or(any)) break;
        worked = true;
    }
    if (!worked) return;
    for (int i = threadIdx.x; i < th * tw; i += ROUTE_THREADS) {
        const int y = i / tw, x = i % tw;
        const int idx = (y + 1) * ROUTE_PITCH + x + 1;
        if (cand[idx] >= 0 && lab[idx] >= 0) label[(size_t)(y0 + y) * W + x0 + x] = lab[idx];
    }
    if (threadIdx.x == 0) state->changed = 1;
}

// ---- the owner map ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seam_route_finish_kernel(const int16_t *a,
                                                                const int16_t *__restrict__ label,
                                                                int n, int16_t *owner,
                                                                RouteState *__restrict__ state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < n) {
        const int l = label[i], first = a[i];
        const int who = l >= 0 ? l : (l == ROUTE_OPEN ? first : -1);
        moved = l >= 0 && who != first;
        owner[i] = (int16_t)who;
    }
    const uint64_t m = __ballot(moved);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&state->n_moved, (int)__popcll(m));
}

// stats: the flood's four; `whole`: the two of pano_seam_route behind them
__global__ void seam_route_stats_kernel(const RouteState *state, int32_t *stats, int whole,
                                        int n_groups) {
    stats[0] = state->n_front;
    stats[1] = state->rounds;
    stats[2] = state->max_rounds;
    stats[3] = state->n_moved;
    if (whole) {
        stats[4] = state->n_open;
        stats[5] = n_groups;
    }
}

static int route_check_shape(int n, int H, int W, const char *who) {
    PANO_REQUIRE(n >= 1 && n <= 32767, "%s: %d cameras (int16 planes hold 1 .. 32767)", who, n);
    PANO_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= (1 << 29),
                 "%s: a %d x %d mosaic is outside H, W >= 1, H W <= 2^29", who, H, W);
    return PANO_OK;
}

static int route_prepare(hipStream_t s, const pano_patch *patches, int n, int H, int W,
                         const int16_t *owner0, float ratio, int16_t *second, uint8_t *diff,
                         int16_t *label, uint8_t *pairs, uint8_t *present) {
    PANO_HIP(hipMemsetAsync(pairs, 0, (size_t)n * n, s));
    PANO_HIP(hipMemsetAsync(present, 0, 256, s));
    hipLaunchKernelGGL(seam_route_prepare_kernel, dim3(ceil_div(W, 64), ceil_div(H, 4)),
                       dim3(64, 4), 0, s, patches, n, H, W, owner0, ratio, second, diff, label,
                       pairs, present);
    PANO_LAUNCH_CHECK("seam_route_prepare_kernel");
    return PANO_OK;
}

static int route_check_prepare(const pano_patch *patches, int n, int H, int W, float ratio,
                               const char *who) {
    PANO_REQUIRE(patches, "%s: null table", who);
    if (int rc = route_check_shape(n, H, W, who)) return rc;
    PANO_REQUIRE(n <= PANO_SEAM_ROUTE_MAX_CAMERAS, "%s: %d cameras (the pair matrix holds %d)",
                 who, n, PANO_SEAM_ROUTE_MAX_CAMERAS);
    PANO_REQUIRE(ratio > 0.0f && ratio <= 1.0f, "%s: ratio %g is outside (0, 1]", who,
                 (double)ratio);
    return PANO_OK;
}

extern "C" int pano_seam_route_prepare(pano_ctx *ctx, const pano_patch *patches, int n, int H,
                                       int W, const int16_t *owner0, float ratio,
                                       int16_t *second, uint8_t *diff, int16_t *label,
                                       uint8_t *pairs, uint8_t *present) {
    PANO_ENTER(ctx, "pano_seam_route_prepare");
    if (int rc = route_check_prepare(patches, n, H, W, ratio, "pano_seam_route_prepare")) return rc;
    PANO_REQUIRE(owner0 && second && diff && label && pairs && present,
                 "pano_seam_route_prepare: null pointer");
    return route_prepare((hipStream_t)stream, patches, n, H, W, owner0, ratio, second, diff, label,
                         pairs, present);
}

// The rounds, the owner map and the statistics (`whole`: six of them).  Waits for the stream.
static int route_flood(pano_ctx *ctx, hipStream_t s, const int16_t *a, const int16_t *second,
                       const uint8_t *diff, int16_t *label, const int32_t *group, int n,
                       int n_groups, int H, int W, int16_t *owner_out, int32_t *stats, bool whole,
                       const char *who) {
    PANO_REQUIRE(n_groups >= 1 && n_groups <= n, "%s: %d groups for %d cameras", who, n_groups, n);
    for (int c = 0; c < n; ++c)
        PANO_REQUIRE(group[c] >= 0 && group[c] < n_groups, "%s: group[%d] = %d of %d groups", who,
                     c, group[c], n_groups);
    const size_t group_off = align_up(sizeof(RouteState));
    if (int rc = pano_buf_reserve_sync(ctx, BUF_ROUTE_STATE, group_off + (size_t)n * sizeof(int32_t), s))
        return rc;
    if (int rc = pano_buf_reserve(ctx->buf[BUF_ROUTE_HOST], sizeof(int32_t), true)) return rc;
    RouteState *state = (RouteState *)ctx->buf[BUF_ROUTE_STATE].p;
    int32_t *group_dev = (int32_t *)((char *)ctx->buf[BUF_ROUTE_STATE].p + group_off);
    volatile int32_t *done = (volatile int32_t *)ctx->buf[BUF_ROUTE_HOST].p;
    const int cells = H * W;
    PANO_HIP(hipMemsetAsync(state, 0, sizeof(RouteState), s));
    // pageable source: the runtime stages it before returning
    PANO_HIP(hipMemcpyAsync(group_dev, group, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(seam_route_init_kernel, dim3(ceil_div(cells, 256)), dim3(256), 0, s, label,
                       diff, cells, state);
    hipLaunchKernelGGL(seam_route_begin_kernel, dim3(1), dim3(1), 0, s, state);
    PANO_LAUNCH_CHECK("seam_route_init_kernel");
    const dim3 grid(ceil_div(W, ROUTE_TILE), ceil_div(H, ROUTE_TILE));
    // every round labels a cell or ends a class: the loop is bounded by cells + 256 n_groups rounds
    const int64_t bound = (int64_t)cells + 256 * (int64_t)n_groups + PANO_SEAM_BATCH;
    *done = 0;
    for (int64_t queued = 0; queued <= bound;) {
        for (int k = 0; k < PANO_SEAM_BATCH; ++k) {
            hipLaunchKernelGGL(seam_route_flood_kernel, grid, dim3(ROUTE_THREADS), 0, s, a, second,
                               diff, label, group_dev, n, H, W, state);
            hipLaunchKernelGGL(seam_route_advance_kernel, dim3(1), dim3(1), 0, s, state, n_groups);
        }
        PANO_LAUNCH_CHECK("the seam route rounds");
        queued += PANO_SEAM_BATCH;
        PANO_HIP(hipMemcpyAsync((void *)done, &state->done, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PANO_HIP(hipStreamSynchronize(s));
        if (*done) break;
    }
    PANO_REQUIRE(*done, "%s: the rounds did not end (a bug)", who);
    hipLaunchKernelGGL(seam_route_finish_kernel, dim3(ceil_div(cells, 256)), dim3(256), 0, s, a,
                       label, cells, owner_out, state);
    if (stats)
        hipLaunchKernelGGL(seam_route_stats_kernel, dim3(1), dim3(1), 0, s, state, stats,
                           whole ? 1 : 0, n_groups);
    PANO_LAUNCH_CHECK("seam_route_finish_kernel");
    return PANO_OK;
}

extern "C" int pano_seam_route_flood(pano_ctx *ctx, const int16_t *a, const int16_t *second,
                                     const uint8_t *diff, int16_t *label, const int32_t *group,
                                     int n, int n_groups, int H, int W, int16_t *owner_out,
                                     int32_t *stats) {
    PANO_ENTER(ctx, "pano_seam_route_flood");
    PANO_REQUIRE(a && second && diff && label && group && owner_out,
                 "pano_seam_route_flood: null pointer");
    if (int rc = route_check_shape(n, H, W, "pano_seam_route_flood")) return rc;
    return route_flood(ctx, (hipStream_t)stream, a, second, diff, label, group, n, n_groups, H, W,
                       owner_out, stats, false, "pano_seam_route_flood");
}

// group[c]: the smallest non-negative integer no lower-indexed competitor of c uses; returns the
// number of groups.  pairs: [n][n], pairs[a][b] != 0 when a and b compete (either way round).
static int route_groups(const uint8_t *pairs, int n, std::vector<int32_t> &group) {
    group.assign(n, 0);
    std::vector<uint8_t> used;
    int n_groups = 1;
    for (int c = 0; c < n; ++c) {
        used.assign(c + 1, 0);
        for (int o = 0; o < c; ++o)
            if (pairs[(size_t)c * n + o] | pairs[(size_t)o * n + c]) used[group[o]] = 1;
        int k = 0;
        while (used[k]) ++k;
        group[c] = k;
        n_groups = k + 1 > n_groups ? k + 1 : n_groups;
    }
    return n_groups;
}

extern "C" int pano_seam_route(pano_ctx *ctx, const pano_patch *patches, int n, int H, int W,
                               float ratio, int16_t *owner, uint8_t *valid, int32_t *stats) {
    PANO_ENTER(ctx, "pano_seam_route");
    if (int rc = route_check_prepare(patches, n, H, W, ratio, "pano_seam_route")) return rc;
    PANO_REQUIRE(owner && valid, "pano_seam_route: null output");
    const hipStream_t s = (hipStream_t)stream;
    const size_t px = (size_t)H * W, nn = (size_t)n * n;
    const size_t label_off = align_up(px * sizeof(int16_t));
    const size_t diff_off = label_off + align_up(px * sizeof(int16_t));
    const size_t pairs_off = diff_off + align_up(px);
    const size_t present_off = pairs_off + align_up(nn);
    if (int rc = pano_buf_reserve_sync(ctx, BUF_ROUTE_PLANES, present_off + 256, s)) return rc;
    if (int rc = pano_buf_reserve(ctx->buf[BUF_ROUTE_PAIRS_HOST], nn, true)) return rc;
    char *base = (char *)ctx->buf[BUF_ROUTE_PLANES].p;
    int16_t *second = (int16_t *)base, *label = (int16_t *)(base + label_off);
    uint8_t *diff = (uint8_t *)(base + diff_off), *pairs = (uint8_t *)(base + pairs_off);
    uint8_t *present = (uint8_t *)(base + present_off);
    if (int rc = pano_ownership(ctx, patches, n, H, W, owner, valid)) return rc;
    if (int rc = route_prepare(s, patches, n, H, W, owner, ratio, second, diff, label, pairs, present))
        return rc;
    const uint8_t *pairs_host = (const uint8_t *)ctx->buf[BUF_ROUTE_PAIRS_HOST].p;
    PANO_HIP(hipMemcpyAsync((void *)pairs_host, pairs, nn, hipMemcpyDeviceToHost, s));
    PANO_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> group;
    const int n_groups = route_groups(pairs_host, n, group);
    // in place: the finish reads a pixel's first owner and writes its routed one in one thread
    return route_flood(ctx, s, owner, second, diff, label, group.data(), n, n_groups, H, W, owner,
                       stats, true, "pano_seam_route");
}
