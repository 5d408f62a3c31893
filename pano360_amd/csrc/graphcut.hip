// The overlap seam: blend.graph_cut of the reference (blend.py:56-100) and blend.alpha_blend
// (blend.py:48-53).  The contract - the levels, the presets, the class sweep that replaces the
// heap and why it gives the heap's labels bit for bit, the resize - is in include/pano360.h;
// tests/graph_cut_model.py restates all of it in NumPy, heap loop included.
//
// Flood.  A tile is a rectangle of cells in LDS with a one-cell frame: one byte of level
// (0 .. 255) and one byte of state per cell.  States: -1 / +1 labelled, 0 unlabelled,
// SEAM_LOW unlabelled with level -1 (257 levels do not fit the byte), SEAM_WALL outside the
// grid.  In class (d, c) a cell is OPEN when it is unlabelled and its level is >= d.  One pass
// (seam_line_pass) takes the lines of one direction, a wave per line, 64 cells per step: the
// ballots of "open", "labelled c" and "open with a c neighbour across the lines" are three
// 64-bit masks, the seeds are the open cells next to a c cell in any of the four directions,
// and one 64-bit addition per direction spreads the seeds over their maximal runs of open cells
// (seam_fill; wave-uniform integer work).  The resident path takes 256 cells of a line at once
// and joins the runs across its 64-cell chunks on the masks; a longer line is walked left to
// right and back with the last cell's state as carry.  Rows and columns alternate until a pass
// labels nothing: since the seeds look in all four directions, one quiet pass is the fixed point.
//
// Races.  A wave reads neighbours' states while other waves write them, and in the tiled path a
// tile reads its halo while the neighbour writes its interior.  A cell only ever goes from
// unlabelled to the one colour of the running class (a byte store), so a stale read only delays
// a label to the next pass or round; the closure is the same set whatever the timing.  No atomics
// anywhere, and the same input gives the same bits.
//
// Resident path: one 1024-thread workgroup declares all of the CU's 160 KiB, loads the grid,
// runs every class and stores the labels: one launch.  Tiled path: 64 x 64 tiles, one launch per
// round plus a one-thread kernel that ends the class when the round's "changed" word stayed
// clear and picks the next level that occurs; PANO_SEAM_BATCH rounds are queued between two
// reads of the "done" word, and the launches past the end return on their first load.
#include "common.h"

#define SEAM_LOW 2
#define SEAM_WALL 3
#define SEAM_RES_THREADS 1024
#define SEAM_RES_CELLS PANO_SEAM_RESIDENT_CELLS
#define SEAM_RES_GROUP 4             // chunks of 64 cells a wave takes of a line at once
#define SEAM_TILE 64
#define SEAM_TILE_PITCH (SEAM_TILE + 2)
#define SEAM_TILE_THREADS 256

static_assert(2 * SEAM_RES_CELLS + 512 <= 160 * 1024, "the resident grid must fit one CU's LDS");

struct SeamState {                  // tiled path: device memory, zeroed before a flood
    int32_t d, c, changed, done;
    int32_t class_rounds, n_front, rounds, max_rounds;
    int32_t present[260];           // present[level + 1]: the level occurs in the grid
};

// ---- levels -------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ bool seam_in_domain(T v) {
    return v >= (T)0 && v <= (T)255 && (T)(int)v == v;
}

// One thread per cell, a block per 256 cells of one cell row: the lanes of a wave read
// neighbouring runs of shrink x c values of the same image row.
template <typename T, bool WRAP>
__global__ __launch_bounds__(256) void seam_levels_kernel(const T *__restrict__ a,
                                                          const T *__restrict__ b, int w, int nc,
                                                          int shrink, int cols,
                                                          int16_t *__restrict__ level,
                                                          int32_t *__restrict__ bad) {
    const int cx = blockIdx.x * 256 + threadIdx.x, cy = blockIdx.y;
    if (cx >= cols) return;
    int lowest = 256;
    bool wrong = false;
    for (int sy = 0; sy < shrink; ++sy) {
        const size_t row = ((size_t)(cy * shrink + sy) * w + (size_t)cx * shrink) * nc;
        for (int sx = 0; sx < shrink; ++sx) {
            const T *pa = a + row + (size_t)sx * nc, *pb = b + row + (size_t)sx * nc;
            int diff = 0;
            for (int k = 0; k < nc; ++k) {
                int dk;
                if (WRAP) {
                    dk = (uint8_t)((int)pa[k] - (int)pb[k]);       // the uint8 subtraction wraps
                } else {
                    wrong |= !seam_in_domain(pa[k]) || !seam_in_domain(pb[k]);
                    dk = (int)pa[k] - (int)pb[k];
                    dk = dk < 0 ? -dk : dk;
                }
                diff = dk > diff ? dk : diff;
            }
            if (nc == 4 && (pa[3] == (T)0 || pb[3] == (T)0)) diff = -1;   // blend.py:62-63
            lowest = diff < lowest ? diff : lowest;
        }
    }
    // uint8: the key -diff wraps too, 0 first, then 255, 254, .. 1
    if (WRAP) lowest = lowest == 0 ? 255 : lowest - 1;
    if (wrong) {
        *bad = 1;
        lowest = 0;
    }
    level[(size_t)cy * cols + cx] = (int16_t)lowest;
}

extern "C" int pano_seam_levels(pano_ctx *ctx, const void *img1, const void *img2, int dtype,
                                int h, int w, int c, int shrink, int16_t *level, int32_t *bad) {
    PANO_ENTER(ctx, "pano_seam_levels");
    PANO_REQUIRE(img1 && img2 && level && bad, "pano_seam_levels: null pointer");
    PANO_REQUIRE(shrink >= 1 && c >= 1 && c <= 4 && h >= shrink && w >= shrink &&
                     (int64_t)h * w <= (1 << 29) && h / shrink <= 65535,
                 "pano_seam_levels: %d x %d x %d with shrink %d is outside 1 <= c <= 4, "
                 "h, w >= shrink >= 1, h w <= 2^29, h / shrink <= 65535", h, w, c, shrink);
    PANO_REQUIRE(dtype >= PANO_SEAM_U8 && dtype <= PANO_SEAM_F64, "pano_seam_levels: dtype %d",
                 dtype);
    PANO_REQUIRE(!(dtype == PANO_SEAM_U8 && c == 4),
                 "pano_seam_levels: uint8 images with an alpha channel (the reference cannot store "
                 "its -1 in a uint8 difference)");
    const hipStream_t s = (hipStream_t)stream;
    const int rows = h / shrink, cols = w / shrink;
    PANO_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
    const dim3 grid(ceil_div(cols, 256), rows), block(256);
#define SEAM_LEVELS(T, WRAP)                                                                   \
    hipLaunchKernelGGL((seam_levels_kernel<T, WRAP>), grid, block, 0, s, (const T *)img1,     \
                       (const T *)img2, w, c, shrink, cols, level, bad)
    switch (dtype) {
    case PANO_SEAM_U8: SEAM_LEVELS(uint8_t, true); break;
    case PANO_SEAM_I16: SEAM_LEVELS(int16_t, false); break;
    case PANO_SEAM_I32: SEAM_LEVELS(int32_t, false); break;
    case PANO_SEAM_F32: SEAM_LEVELS(float, false); break;
    default: SEAM_LEVELS(double, false); break;
    }
#undef SEAM_LEVELS
    PANO_LAUNCH_CHECK("seam_levels_kernel");
    return PANO_OK;
}

// ---- the flood of one class in one LDS tile -------------------------------------------------
// Seeds (a subset of `open`) spread towards the higher bits over the runs of `open` they lie in:
// adding a seed to its run sends a carry through the run's ones above it, so the ones that the
// sum cleared are the filled cells (a second seed higher in the run stays set: or it back in).
__device__ __forceinline__ uint64_t seam_fill_up(uint64_t seeds, uint64_t open) {
    return ((open ^ (open + seeds)) & open) | seeds;
}

// ... and towards both ends
__device__ __forceinline__ uint64_t seam_fill(uint64_t seeds, uint64_t open) {
    seeds &= open;
    return seam_fill_up(seeds, open) | __brevll(seam_fill_up(__brevll(seeds), __brevll(open)));
}

__device__ __forceinline__ int seam_clamp_level(int v) { return v < -1 ? -1 : (v > 255 ? 255 : v); }

// The state a cell takes before the flood (blend.py:71-80, the seeds popped): see the header.
__device__ __forceinline__ int seam_preset(int x, int cols, int border) {
    return x <= border ? -1 : (x >= cols - border ? 1 : 0);
}

// One pass along `nlines` lines of `len` cells.  Cell p of line l is at origin + l across +
// p along; every line has a frame cell at p = -1 and p = len, and frame lines at l = -1 and
// l = nlines.  A wave takes a line G chunks of 64 cells at a time: their loads go out together,
// and the runs that cross a chunk boundary inside the group are joined on the masks alone.
// Returns whether this wave labelled a cell (the same in all its lanes).
template <int G>
__device__ __forceinline__ bool seam_line_pass(const uint8_t *lev, int8_t *st, int origin,
                                               int nlines, int len, int along, int across, int d,
                                               int c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int floor_level = d < 0 ? 0 : d;
    const bool low_open = d < 0;
    const int ngroups = (len + 64 * G - 1) / (64 * G);
    const int ndirs = ngroups > 1 ? 2 : 1;
    bool any = false;
    for (int line = wave; line < nlines; line += nwaves) {
        const int base = origin + line * across;
        for (int dir = 0; dir < ndirs; ++dir) {
            bool carry = false;
            for (int gg = 0; gg < ngroups; ++gg) {
                const int g = dir ? ngroups - 1 - gg : gg;
                const int p0 = g * 64 * G, p1 = p0 + 64 * G;
                uint64_t open_m[G], c_m[G], fill[G];
                int idx[G];
                uint64_t any_open = 0;
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int p = p0 + 64 * j + lane;
                    idx[j] = base + p * along;
                    const bool inside = p < len;
                    const int s = p <= len ? (int)st[idx[j]] : SEAM_WALL;   // p == len: the frame
                    const int v = inside ? (int)lev[idx[j]] : 0;
                    const bool open = inside && ((s == 0 && v >= floor_level) ||
                                                 (s == SEAM_LOW && low_open));
                    open_m[j] = __ballot(open);
                    c_m[j] = __ballot(s == c);
                    any_open |= open_m[j];
                }
                // most chunks hold no open cell (early: few levels are >= d; late: all is labelled)
                if (any_open) {
                    bool before = st[base + (p0 - 1) * along] == c;
                    bool after = p1 <= len && st[base + p1 * along] == c;
                    if (gg > 0) {
                        if (dir == 0) before |= carry;
                        else after |= carry;
                    }
                    uint64_t any_fill = 0;
#pragma unroll
                    for (int j = 0; j < G; ++j) {
                        fill[j] = 0;
                        if (open_m[j] == 0) continue;
                        const bool side = ((open_m[j] >> lane) & 1) &&
                                          (st[idx[j] - across] == c || st[idx[j] + across] == c);
                        const uint64_t low = j == 0 ? (before ? 1ull : 0ull) : c_m[j - 1] >> 63;
                        const uint64_t high = j == G - 1 ? (after ? 1ull : 0ull) : c_m[j + 1] & 1;
                        const uint64_t seeds = (__ballot(side) | (c_m[j] << 1) | low |
                                                (c_m[j] >> 1) | (high << 63)) & open_m[j];
                        if (seeds) fill[j] = seam_fill(seeds, open_m[j]);
                        any_fill |= fill[j];
                    }
                    if (any_fill) {
                        // a run that a neighbouring chunk filled up to the boundary goes on here
#pragma unroll
                        for (int j = 1; j < G; ++j)
                            if ((fill[j - 1] >> 63) & open_m[j] & ~fill[j] & 1)
                                fill[j] |= seam_fill_up(1ull, open_m[j]);
#pragma unroll
                        for (int j = G - 2; j >= 0; --j)
                            if ((fill[j + 1] & 1) & ((open_m[j] & ~fill[j]) >> 63))
                                fill[j] |= __brevll(seam_fill_up(1ull, __brevll(open_m[j])));
#pragma unroll
                        for (int j = 0; j < G; ++j)
                            if ((fill[j] >> lane) & 1) st[idx[j]] = (int8_t)c;
                        any = true;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < G; ++j) fill[j] = 0;
                }
                carry = dir == 0 ? ((fill[G - 1] | c_m[G - 1]) >> 63) & 1
                                 : (fill[0] | c_m[0]) & 1;
            }
        }
    }
    return any;
}

// Class (d, c) to its fixed point in a tile of th x tw cells (pitch tw + 2 or more, frame
// included).  flags: three ints in LDS, all 0 before the block's first class; `phase` counts the
// block's passes across classes: pass n reports in flags[n % 3] and clears the slot of pass
// n + 1, which was last read two barriers ago.  Returns the passes that labelled a cell.
template <int G>
__device__ __forceinline__ int seam_flood_class(const uint8_t *lev, int8_t *st, int pitch, int th,
                                                int tw, int d, int c, volatile int *flags,
                                                int &phase) {
    const int origin = pitch + 1;
    int passes = 0;
    for (;;) {
        const int slot = phase % 3;
        if (threadIdx.x == 0) flags[(phase + 1) % 3] = 0;
        const bool any = (passes & 1) ? seam_line_pass<G>(lev, st, origin, tw, th, pitch, 1, d, c)
                                      : seam_line_pass<G>(lev, st, origin, th, tw, 1, pitch, d, c);
        if (any && (threadIdx.x & 63) == 0) flags[slot] = 1;
        __syncthreads();
        ++phase;
        if (!flags[slot]) break;
        ++passes;
    }
    return passes;
}

// ---- resident path ------------------------------------------------------------------------
__global__ __launch_bounds__(SEAM_RES_THREADS) void seam_resident_kernel(
    const int16_t *__restrict__ level, int rows, int cols, int border,
    int8_t *__restrict__ labels, int32_t *__restrict__ stats) {
    __shared__ uint8_t lev[SEAM_RES_CELLS];
    __shared__ int8_t st[SEAM_RES_CELLS];
    __shared__ uint8_t present[260];
    __shared__ int flags[3];
    const int pitch = cols + 2, cells = (rows + 2) * pitch;
    for (int i = threadIdx.x; i < 260; i += SEAM_RES_THREADS) present[i] = 0;
    if (threadIdx.x < 3) flags[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += SEAM_RES_THREADS) {
        const int y = i / pitch - 1, x = i % pitch - 1;
        int s = SEAM_WALL, v = 0;
        if (y >= 0 && y < rows && x >= 0 && x < cols) {
            v = seam_clamp_level(level[(size_t)y * cols + x]);
            present[v + 1] = 1;                       // every writer stores the same byte
            s = seam_preset(x, cols, border);
            if (s == 0 && v < 0) s = SEAM_LOW;
        }
        lev[i] = (uint8_t)(v < 0 ? 0 : v);
        st[i] = (int8_t)s;
    }
    __syncthreads();
    int phase = 0, n_front = 0, total = 0, most = 0;
    for (int d = 255; d >= -1; --d) {
        if (!present[d + 1]) continue;
        for (int c = -1; c <= 1; c += 2) {
            const int passes = seam_flood_class<SEAM_RES_GROUP>(lev, st, pitch, rows, cols, d, c, flags, phase);
            if (passes) {
                ++n_front;
                total += passes;
                most = passes > most ? passes : most;
            }
        }
    }
    for (int i = threadIdx.x; i < rows * cols; i += SEAM_RES_THREADS) {
        const int s = st[(i / cols + 1) * pitch + i % cols + 1];
        labels[i] = (int8_t)(s == SEAM_LOW ? 0 : s);
    }
    if (stats && threadIdx.x == 0) {
        stats[0] = n_front;
        stats[1] = total;
        stats[2] = most;
        stats[3] = 1;
    }
}

// ---- tiled path ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seam_init_kernel(const int16_t *__restrict__ level,
                                                        int cols, int n, int border,
                                                        int8_t *__restrict__ labels,
                                                        SeamState *__restrict__ state) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    state->present[seam_clamp_level(level[i]) + 1] = 1;                 // every writer stores the same word
    labels[i] = (int8_t)seam_preset(i % cols, cols, border);
}

// the highest level that occurs below `from` (inclusive), or -2
__device__ __forceinline__ int seam_next_level(const SeamState *state, int from) {
    int d = from;
    while (d >= -1 && !state->present[d + 1]) --d;
    return d;
}

__global__ void seam_begin_kernel(SeamState *state) {
    state->d = seam_next_level(state, 255);
    state->c = -1;
    state->done = state->d < -1;
}

// after a round: the same class again if a tile changed, else the next class
__global__ void seam_advance_kernel(SeamState *state) {
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
    if (state->c < 0) {
        state->c = 1;
        return;
    }
    const int d = seam_next_level(state, state->d - 1);
    if (d < -1) {
        state->done = 1;
    } else {
        state->d = d;
        state->c = -1;
    }
}

__global__ __launch_bounds__(SEAM_TILE_THREADS) void seam_tile_kernel(
    const int16_t *__restrict__ level, int rows, int cols, int8_t *labels, SeamState *state) {
    __shared__ uint8_t lev[SEAM_TILE_PITCH * SEAM_TILE_PITCH];
    __shared__ int8_t st[SEAM_TILE_PITCH * SEAM_TILE_PITCH];
    __shared__ int flags[3];
    if (state->done) return;
    const int d = state->d, c = state->c;
    const int y0 = blockIdx.y * SEAM_TILE, x0 = blockIdx.x * SEAM_TILE;
    const int th = rows - y0 < SEAM_TILE ? rows - y0 : SEAM_TILE;
    const int tw = cols - x0 < SEAM_TILE ? cols - x0 : SEAM_TILE;
    if (threadIdx.x < 3) flags[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < SEAM_TILE_PITCH * SEAM_TILE_PITCH; i += SEAM_TILE_THREADS) {
        const int y = y0 + i / SEAM_TILE_PITCH - 1, x = x0 + i % SEAM_TILE_PITCH - 1;
        int s = SEAM_WALL, v = 0;
        if (y >= 0 && y < rows && x >= 0 && x < cols) {
            v = seam_clamp_level(level[(size_t)y * cols + x]);
            s = labels[(size_t)y * cols + x];
            if (s == 0 && v < 0) s = SEAM_LOW;
        }
        lev[i] = (uint8_t)(v < 0 ? 0 : v);
        st[i] = (int8_t)s;
    }
    __syncthreads();
    int phase = 0;
    if (!seam_flood_class<1>(lev, st, SEAM_TILE_PITCH, th, tw, d, c, flags, phase)) return;
    for (int i = threadIdx.x; i < th * tw; i += SEAM_TILE_THREADS) {
        const int y = i / tw, x = i % tw;
        if (st[(y + 1) * SEAM_TILE_PITCH + x + 1] == c)
            labels[(size_t)(y0 + y) * cols + x0 + x] = (int8_t)c;
    }
    if (threadIdx.x == 0) state->changed = 1;
}

__global__ void seam_stats_kernel(const SeamState *state, int32_t *stats) {
    stats[0] = state->n_front;
    stats[1] = state->rounds;
    stats[2] = state->max_rounds;
    stats[3] = 2;
}

extern "C" int pano_seam_flood(pano_ctx *ctx, const int16_t *level, int rows, int cols,
                               int border, int path, int8_t *labels, int32_t *stats) {
    PANO_ENTER(ctx, "pano_seam_flood");
    PANO_REQUIRE(level && labels, "pano_seam_flood: null pointer");
    PANO_REQUIRE(rows >= 1 && border >= 2 && cols >= 2 * border + 1 &&
                     (int64_t)rows * cols <= (1 << 29),
                 "pano_seam_flood: a %d x %d grid with bands of %d columns is outside rows >= 1, "
                 "border >= 2, cols >= 2 border + 1, rows cols <= 2^29", rows, cols, border);
    PANO_REQUIRE(path >= 0 && path <= 2, "pano_seam_flood: path %d", path);
    const hipStream_t s = (hipStream_t)stream;
    const bool fits = (int64_t)(rows + 2) * (cols + 2) <= SEAM_RES_CELLS;
    PANO_REQUIRE(path != 1 || fits, "pano_seam_flood: a %d x %d grid does not fit the resident "
                 "path (%d cells, frame included)", rows, cols, SEAM_RES_CELLS);
    if (path == 1 || (path == 0 && fits)) {
        hipLaunchKernelGGL(seam_resident_kernel, dim3(1), dim3(SEAM_RES_THREADS), 0, s, level,
                           rows, cols, border, labels, stats);
        PANO_LAUNCH_CHECK("seam_resident_kernel");
        return PANO_OK;
    }
    if (int rc = pano_buf_reserve(ctx->buf[BUF_SEAM_DEV], sizeof(SeamState), false)) return rc;
    if (int rc = pano_buf_reserve(ctx->buf[BUF_SEAM_HOST], sizeof(int32_t), true)) return rc;
    SeamState *state = (SeamState *)ctx->buf[BUF_SEAM_DEV].p;
    volatile int32_t *done = (volatile int32_t *)ctx->buf[BUF_SEAM_HOST].p;
    const int n = rows * cols;
    PANO_HIP(hipMemsetAsync(state, 0, sizeof(SeamState), s));
    hipLaunchKernelGGL(seam_init_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, s, level, cols, n,
                       border, labels, state);
    hipLaunchKernelGGL(seam_begin_kernel, dim3(1), dim3(1), 0, s, state);
    PANO_LAUNCH_CHECK("seam_init_kernel");
    const dim3 grid(ceil_div(cols, SEAM_TILE), ceil_div(rows, SEAM_TILE));
    // every round labels a cell or ends a class: the loop is bounded by n + 2 * 257 rounds
    for (int64_t queued = 0; queued <= (int64_t)n + 2 * 257 + PANO_SEAM_BATCH;) {
        for (int k = 0; k < PANO_SEAM_BATCH; ++k) {
            hipLaunchKernelGGL(seam_tile_kernel, grid, dim3(SEAM_TILE_THREADS), 0, s, level, rows,
                               cols, labels, state);
            hipLaunchKernelGGL(seam_advance_kernel, dim3(1), dim3(1), 0, s, state);
        }
        PANO_LAUNCH_CHECK("the seam rounds");
        queued += PANO_SEAM_BATCH;
        PANO_HIP(hipMemcpyAsync((void *)done, &state->done, sizeof(int32_t),
                                hipMemcpyDeviceToHost, s));
        PANO_HIP(hipStreamSynchronize(s));
        if (*done) break;
    }
    PANO_REQUIRE(*done, "pano_seam_flood: the rounds did not end (a bug)");
    if (stats) {
        hipLaunchKernelGGL(seam_stats_kernel, dim3(1), dim3(1), 0, s, state, stats);
        PANO_LAUNCH_CHECK("seam_stats_kernel");
    }
    return PANO_OK;
}

// ---- mask -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seam_mask_kernel(const int8_t *__restrict__ labels,
                                                        int cols, const int4 *__restrict__ xtab,
                                                        const int4 *__restrict__ ytab,
                                                        uint8_t *__restrict__ mask, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int4 tx = xtab[x], ty = ytab[y];
    const float a0 = __int_as_float(tx.z), a1 = __int_as_float(tx.w);
    const float b0 = __int_as_float(ty.z), b1 = __int_as_float(ty.w);
    const int8_t *top = labels + (size_t)ty.x * cols, *bottom = labels + (size_t)ty.y * cols;
    const float s00 = top[tx.x] == -1 ? 1.0f : 0.0f, s01 = top[tx.y] == -1 ? 1.0f : 0.0f;
    const float s10 = bottom[tx.x] == -1 ? 1.0f : 0.0f, s11 = bottom[tx.y] == -1 ? 1.0f : 0.0f;
    const float r0 = s00 * a0 + s01 * a1, r1 = s10 * a0 + s11 * a1;       // unfused (Makefile)
    const float v = r0 * b0 + r1 * b1;
    mask[(size_t)y * w + x] = (uint8_t)(int)(v * 255.0f);                 // truncates, as astype
}

extern "C" int pano_seam_mask(pano_ctx *ctx, const int8_t *labels, int rows, int cols,
                              const int32_t *xtab, const int32_t *ytab, uint8_t *mask, int h,
                              int w) {
    PANO_ENTER(ctx, "pano_seam_mask");
    PANO_REQUIRE(labels && xtab && ytab && mask, "pano_seam_mask: null pointer");
    PANO_REQUIRE(rows >= 1 && cols >= 1 && h >= 1 && w >= 1 && h <= 65535,
                 "pano_seam_mask: %d x %d cells to %d x %d pixels", rows, cols, h, w);
    hipLaunchKernelGGL(seam_mask_kernel, dim3(ceil_div(w, 256), h), dim3(256), 0,
                       (hipStream_t)stream, labels, cols, (const int4 *)xtab, (const int4 *)ytab,
                       mask, w);
    PANO_LAUNCH_CHECK("seam_mask_kernel");
    return PANO_OK;
}

// ---- alpha blend ----------------------------------------------------------------------------
// T: the images' type, M: the mask's, K: NumPy's result type of the two
template <typename T, typename M, typename K>
__global__ __launch_bounds__(256) void alpha_blend_kernel(const T *__restrict__ a,
                                                          const T *__restrict__ b,
                                                          const M *__restrict__ mask, int64_t sy,
                                                          int64_t sx, int64_t sc, int w, int nc,
                                                          size_t n, uint8_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t px = i / nc;
    const int k = (int)(i % nc), x = (int)(px % w);
    const int64_t y = (int64_t)(px / w);
    const M m = mask[y * sy + x * sx + k * sc];
    const M rest = (M)1 - m;
    const K first = (K)a[i] * (K)m, second = (K)b[i] * (K)rest;           // unfused (Makefile)
    out[i] = (uint8_t)(int)(first + second);
}

extern "C" int pano_alpha_blend(pano_ctx *ctx, const void *img1, const void *img2, int dtype,
                                const void *mask, int mask_f64, int64_t mask_sy, int64_t mask_sx,
                                int64_t mask_sc, int h, int w, int c, uint8_t *out) {
    PANO_ENTER(ctx, "pano_alpha_blend");
    PANO_REQUIRE(img1 && img2 && mask && out, "pano_alpha_blend: null pointer");
    PANO_REQUIRE(h >= 1 && w >= 1 && c >= 1 && (int64_t)h * w * c <= ((int64_t)1 << 31),
                 "pano_alpha_blend: %d x %d x %d", h, w, c);
    PANO_REQUIRE(dtype >= PANO_SEAM_U8 && dtype <= PANO_SEAM_F64, "pano_alpha_blend: dtype %d",
                 dtype);
    PANO_REQUIRE(mask_sy >= 0 && mask_sx >= 0 && mask_sc >= 0, "pano_alpha_blend: mask strides");
    const size_t n = (size_t)h * w * c;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const hipStream_t s = (hipStream_t)stream;
#define ALPHA(T, M, K)                                                                         \
    hipLaunchKernelGGL((alpha_blend_kernel<T, M, K>), grid, block, 0, s, (const T *)img1,     \
                       (const T *)img2, (const M *)mask, mask_sy, mask_sx, mask_sc, w, c, n, out)
    if (mask_f64) {
        switch (dtype) {
        case PANO_SEAM_U8: ALPHA(uint8_t, double, double); break;
        case PANO_SEAM_I16: ALPHA(int16_t, double, double); break;
        case PANO_SEAM_I32: ALPHA(int32_t, double, double); break;
        case PANO_SEAM_F32: ALPHA(float, double, double); break;
        default: ALPHA(double, double, double); break;
        }
    } else {
        switch (dtype) {
        case PANO_SEAM_U8: ALPHA(uint8_t, float, float); break;
        case PANO_SEAM_I16: ALPHA(int16_t, float, float); break;
        case PANO_SEAM_I32: ALPHA(int32_t, float, double); break;
        case PANO_SEAM_F32: ALPHA(float, float, float); break;
        default: ALPHA(double, float, double); break;
        }
    }
#undef ALPHA
    PANO_LAUNCH_CHECK("alpha_blend_kernel");
    return PANO_OK;
}
