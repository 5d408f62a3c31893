// Deghosting of exposure brackets before they are fused (pano_deghost_u8, pano_deghost_work_bytes):
// reference-guided and rank based.  Two exposures of a static scene differ by a monotone map of
// brightness, so a pixel's rank within its own frame's histogram is nearly the same in both; where
// the ranks of an exposure and of the stack's reference exposure disagree, the exposure shows other
// scene content and takes the reference's pixel, carried to its own brightness through the
// histogram-matching map of the two frames.  Integers throughout: the contract is in
// include/pano360.h, a NumPy statement of it is tests/deghost_model.py.
//
// One tile table (batch.h) over all frames of all stacks of a call, a section of it per launch:
//   deghost_hist_kernel    a 128 x 128 tile of a frame -> its grey values, stored, and in LDS its
//                          counts of g, B, G and R, added to the frame's [4][256] histograms with
//                          integer atomicAdd
//   deghost_tables_kernel  a workgroup per frame scans the bins: the rank interval of every grey
//                          value and, against the reference's scanned bins, the three colour maps
//   deghost_raw_kernel     rank intervals apart by more than tol -> the raw mask, 32 pixels a word
//   deghost_clean_kernel   erosion and dilation of the packed words in LDS, the set bits counted
//   deghost_apply_kernel   frames with a dst and a count above 0 are copied, masked pixels from
//                          the mapped reference; the tiles of the others leave at once
// Integer sums do not depend on the order of the additions: the same input gives the same bytes.
#include "batch.h"
#include "geom.h"
#include "wave.h"

#define DG_TILE 128                 // the histogram kernel's tile
#define DG_FRAMES 256               // frames of one pass over the kernels (whole stacks)
#define DG_MAX_SLACK 15
#define DG_MAX_ERODE 3
#define DG_MAX_DILATE 15
#define DG_REACH (DG_MAX_ERODE + DG_MAX_DILATE)     // 18 < 32: one neighbouring word on each side
#define DG_CW 16                    // the clean-up's tile: words of a row,
#define DG_CH 64                    // and rows
#define DG_LW (DG_CW + 2)           // ... in LDS with a word on each side
#define DG_LH (DG_CH + 2 * DG_REACH)    // and erode + dilate rows above and below

struct DeghostDev {                 // a frame of a launch, in device memory
    const uint8_t *src, *ref_src;   // the frame and its stack's reference frame
    uint8_t *dst;
    int64_t src_pitch, ref_pitch, dst_pitch;
    uint8_t *grey;                  // [h][w rounded up to 4]
    const uint8_t *ref_grey;
    uint32_t *hist;                 // [4][256]: g, B, G, R
    const uint32_t *ref_hist;
    uint8_t *ranks;                 // [2][256]: lo, hi
    const uint8_t *ref_ranks;
    uint8_t *maps;                  // [3][256]
    uint32_t *raw, *mask;           // [h][wpr]
    int32_t *count;                 // the frame's entry of the stack's counts
    int w, h, slack, tol, erode, dilate, is_ref;
    TileSlot slot;
};

// ---- stage A: grey and histograms -----------------------------------------------------------
// One workgroup per 128 x 128 tile of a frame: a thread takes four neighbouring pixels of a row as
// three dwords, 16 passes of 8 rows.  Every input byte is read once; the grey values are stored
// for stage C (1 byte a pixel written and 2 read there, against 6 read to form them again).
__global__ __launch_bounds__(256) void deghost_hist_kernel(const DeghostDev *__restrict__ table, int n) {
    __shared__ uint32_t s_hist[4][256];
    int tile;
    const DeghostDev &D = batch_record(table, n, tile);
    const int tid = threadIdx.x, h = D.h, w = D.w, pitch = (w + 3) & ~3;
    const int x0 = (tile % D.slot.tiles_x) * DG_TILE, y0 = (tile / D.slot.tiles_x) * DG_TILE;
#pragma unroll
    for (int c = 0; c < 4; ++c) s_hist[c][tid] = 0;
    __syncthreads();
    const int x = x0 + (tid & 31) * 4, ry = tid >> 5;
    for (int p = 0; p < DG_TILE / 8; ++p) {
        const int y = y0 + p * 8 + ry;
        if (y >= h || x >= w) continue;
        uint32_t b[4][3], g4 = 0;
        rgb4_load((frame_ptr)D.src + (int64_t)y * D.src_pitch + 3 * x, x, w, b);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < w) {
                const uint32_t g = (29u * b[j][0] + 150u * b[j][1] + 77u * b[j][2] + 128u) >> 8;
                g4 |= g << (8 * j);
                atomicAdd(&s_hist[0][g], 1u);
                atomicAdd(&s_hist[1][b[j][0]], 1u);
                atomicAdd(&s_hist[2][b[j][1]], 1u);
                atomicAdd(&s_hist[3][b[j][2]], 1u);
            }
        // (x is a multiple of 4 below w: the dword ends inside the row's pitch)
        *(uint32_t *)(D.grey + (size_t)y * pitch + x) = g4;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t v = s_hist[c][tid];
        if (v) atomicAdd(&D.hist[c * 256 + tid], v);
    }
}

// ---- stage B: tables ------------------------------------------------------------------------
// One workgroup per frame, a thread per bin.  below[c][v] = #{. < v} of the frame's four
// histograms by exclusive scans, kept in LDS; thread v then forms the rank interval of grey v
// and, for a frame other than the reference, scans the reference's colour bins and searches the
// frame's scanned counts for the three map entries of value v.
__global__ __launch_bounds__(256) void deghost_tables_kernel(const DeghostDev *__restrict__ table) {
    __shared__ uint32_t s_below[4][257];
    __shared__ uint32_t s_waves[4];
    const DeghostDev &D = table[blockIdx.x];
    const int tid = threadIdx.x;
    const uint64_t N = (uint64_t)D.h * (uint64_t)D.w;
    for (int c = 0; c < 4; ++c) {
        uint32_t total;
        s_below[c][tid] = block_scan_exclusive<256>(D.hist[c * 256 + tid], s_waves, total);
        if (tid == 255) s_below[c][256] = total;
    }
    __syncthreads();
    const int a = max(tid - D.slack, 0), b = min(tid + D.slack + 1, 256);
    D.ranks[tid] = (uint8_t)((uint64_t)s_below[0][a] * 255u / N);
    D.ranks[256 + tid] = (uint8_t)((uint64_t)s_below[0][b] * 255u / N);
    if (D.is_ref) {                                     // (the whole workgroup)
        for (int c = 0; c < 3; ++c) D.maps[c * 256 + tid] = (uint8_t)tid;
        return;
    }
    for (int c = 0; c < 3; ++c) {
        const uint32_t hr = D.ref_hist[(1 + c) * 256 + tid];
        uint32_t total;
        const uint32_t target = block_scan_exclusive<256>(hr, s_waves, total) + (hr + 1u) / 2u;
        int lo = 0, hi = 255;                           // the smallest u with below[u + 1] >= target
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_below[1 + c][mid + 1] >= target)
                hi = mid;
            else
                lo = mid + 1;
        }
        D.maps[c * 256 + tid] = (uint8_t)lo;
    }
}

// ---- stage C: raw mask ----------------------------------------------------------------------
// One workgroup per 256 x 16 pixels of a frame other than the reference, a wave per row and four
// rows per wave: a lane takes four grey pixels of the frame and of the reference as a dword each,
// and eight lanes' four bits meet in a word through three exchanges (align.hip's packing).  The
// four 256-byte rank tables sit in LDS.  Bits from the row's end on are 0.
__global__ __launch_bounds__(256) void deghost_raw_kernel(const DeghostDev *__restrict__ table, int n) {
    __shared__ uint8_t s_rank[4][256];                  // lo_i, hi_i, lo_r, hi_r
    int tile;
    const DeghostDev &D = batch_record(table, n, tile);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_rank[0][tid] = D.ranks[tid], s_rank[1][tid] = D.ranks[256 + tid];
    s_rank[2][tid] = D.ref_ranks[tid], s_rank[3][tid] = D.ref_ranks[256 + tid];
    __syncthreads();
    const int h = D.h, w = D.w, pitch = (w + 3) & ~3, wpr = (w + 31) >> 5, tol = D.tol;
    const int x = (tile % D.slot.tiles_x) * 256 + 4 * lane;
    for (int i = 0; i < 4; ++i) {
        const int y = (tile / D.slot.tiles_x) * 16 + wave * 4 + i;
        if (y >= h) break;                              // (the whole wave)
        uint32_t gi4 = 0, gr4 = 0;
        if (x < w) {
            gi4 = *(const uint32_t *)(D.grey + (size_t)y * pitch + x);
            gr4 = *(const uint32_t *)(D.ref_grey + (size_t)y * pitch + x);
        }
        uint32_t bits = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < w) {
                const uint32_t gi = (gi4 >> (8 * j)) & 255u, gr = (gr4 >> (8 * j)) & 255u;
                const int lo_i = s_rank[0][gi], hi_i = s_rank[1][gi], lo_r = s_rank[2][gr], hi_r = s_rank[3][gr];
                bits |= (uint32_t)(lo_i > hi_r + tol || lo_r > hi_i + tol) << j;
            }
        bits <<= 4 * (lane & 7);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) bits |= __shfl_xor(bits, o, 64);
        if ((lane & 7) == 0 && (x >> 5) < wpr) D.raw[(size_t)y * wpr + (x >> 5)] = bits;
    }
}

// ---- stage D: clean-up ----------------------------------------------------------------------
// 32 bits from bit `off` (0 .. 63) of the 96 bits w0, w1, w2
__device__ __forceinline__ uint32_t deghost_bits_at(uint32_t w0, uint32_t w1, uint32_t w2, int off) {
    const uint64_t lo = (uint64_t)w0 | (uint64_t)w1 << 32, hi = (uint64_t)w1 | (uint64_t)w2 << 32;
    return off < 32 ? (uint32_t)(lo >> off) : (uint32_t)(hi >> (off - 32));
}

// One workgroup per 16 words x 64 rows of a frame other than the reference, on packed words only.
// The raw words of the tile, a word on each side and erode + dilate rows above and below go to
// LDS, what lies outside the image as set.  Then four passes between two LDS tiles: the erosion
// along the row (a word and its two neighbours, funnel shifts, AND), down the column (AND over
// rows), everything outside the image cleared, and the dilation likewise with OR.  A pass is
// evaluated only where the passes before it are whole: the rows lose `erode` at either end after
// the erosion, and of the side words only the bits next to the tile are right - erode <= 3 bits
// of them are not, and the dilation reads the 15 nearest the tile.
__global__ __launch_bounds__(256) void deghost_clean_kernel(const DeghostDev *__restrict__ table, int n) {
    __shared__ uint32_t s_a[DG_LH][DG_LW], s_b[DG_LH][DG_LW];
    __shared__ uint32_t s_cnt[4];
    int tile;
    const DeghostDev &D = batch_record(table, n, tile);
    const int tid = threadIdx.x, h = D.h, w = D.w, wpr = (w + 31) >> 5;
    const int er = D.erode, di = D.dilate, reach = er + di, rows = DG_CH + 2 * reach;
    const int xw0 = (tile % D.slot.tiles_x) * DG_CW - 1, y0 = (tile / D.slot.tiles_x) * DG_CH - reach;
    const uint32_t last = (w & 31) ? (1u << (w & 31)) - 1u : ~0u;      // the pixels of a row's last word
    for (int i = tid; i < rows * DG_LW; i += 256) {
        const int r = i / DG_LW, c = i % DG_LW, y = y0 + r, xw = xw0 + c;
        uint32_t v = ~0u;
        if (y >= 0 && y < h && xw >= 0 && xw < wpr) {
            v = D.raw[(size_t)y * wpr + xw];
            if (xw == wpr - 1) v |= ~last;
        }
        s_a[r][c] = v;
    }
    __syncthreads();
    for (int i = tid; i < rows * DG_LW; i += 256) {     // the erosion along the row: a -> b
        const int r = i / DG_LW, c = i % DG_LW;
        const uint32_t w0 = c > 0 ? s_a[r][c - 1] : ~0u, w1 = s_a[r][c], w2 = c < DG_LW - 1 ? s_a[r][c + 1] : ~0u;
        uint32_t v = w1;
        for (int s = 1; s <= er; ++s) v &= deghost_bits_at(w0, w1, w2, 32 + s) & deghost_bits_at(w0, w1, w2, 32 - s);
        s_b[r][c] = v;
    }
    __syncthreads();
    for (int i = tid; i < rows * DG_LW; i += 256) {     // ... down the column: b -> a, rows er .. rows - er - 1
        const int r = i / DG_LW, c = i % DG_LW, y = y0 + r, xw = xw0 + c;
        if (r < er || r >= rows - er) continue;
        uint32_t v = s_b[r][c];
        for (int s = 1; s <= er; ++s) v &= s_b[r - s][c] & s_b[r + s][c];
        if (!(y >= 0 && y < h && xw >= 0 && xw < wpr))
            v = 0;                                      // outside the image: clear for the dilation
        else if (xw == wpr - 1)
            v &= last;
        s_a[r][c] = v;
    }
    __syncthreads();
    for (int i = tid; i < rows * DG_LW; i += 256) {     // the dilation along the row: a -> b, the tile's words
        const int r = i / DG_LW, c = i % DG_LW;
        if (r < er || r >= rows - er || c < 1 || c > DG_CW) continue;
        const uint32_t w0 = s_a[r][c - 1], w1 = s_a[r][c], w2 = s_a[r][c + 1];
        uint32_t v = w1;
        for (int s = 1; s <= di; ++s) v |= deghost_bits_at(w0, w1, w2, 32 + s) | deghost_bits_at(w0, w1, w2, 32 - s);
        s_b[r][c] = v;
    }
    __syncthreads();
    uint32_t cnt = 0;
    for (int i = tid; i < DG_CH * DG_CW; i += 256) {    // ... down the column: b -> the mask
        const int r = reach + i / DG_CW, c = 1 + i % DG_CW, y = y0 + r, xw = xw0 + c;
        if (y >= h || xw >= wpr) continue;
        uint32_t v = s_b[r][c];
        for (int s = 1; s <= di; ++s) v |= s_b[r - s][c] | s_b[r + s][c];
        if (xw == wpr - 1) v &= last;
        D.mask[(size_t)y * wpr + xw] = v;
        cnt += (uint32_t)__popc(v);
    }
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        const uint32_t total = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (total) atomicAdd(D.count, (int32_t)total);
    }
}

// ---- stage E: apply -------------------------------------------------------------------------
// One workgroup per 64 x 16 tile, a thread four neighbouring pixels of a row: twelve bytes in,
// three dwords out, and the reference's twelve only where one of the four mask bits is set.  The
// three 256-byte maps sit in LDS.  A frame whose count is 0 is not copied: its tiles leave.
__global__ __launch_bounds__(256) void deghost_apply_kernel(const DeghostDev *__restrict__ table, int n) {
    __shared__ uint8_t s_map[3][256];
    int tile;
    const DeghostDev &D = batch_record(table, n, tile);
    if (*D.count == 0) return;                          // (the whole workgroup)
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) s_map[c][tid] = D.maps[c * 256 + tid];
    __syncthreads();
    const int w = D.w, h = D.h, wpr = (w + 31) >> 5;
    const int u0 = (tile % D.slot.tiles_x) * 64 + (tid & 15) * 4;
    const int v = (tile / D.slot.tiles_x) * 16 + (tid >> 4);
    if (u0 >= w || v >= h) return;
    // (u0 is a multiple of 4: the four bits lie in one word; those from w on are 0)
    const uint32_t four = (D.mask[(size_t)v * wpr + (u0 >> 5)] >> (u0 & 31)) & 15u;
    uint32_t b[4][3];
    rgb4_load((frame_ptr)D.src + (int64_t)v * D.src_pitch + 3 * u0, u0, w, b);
    if (four) {
        uint32_t r[4][3];
        rgb4_load((frame_ptr)D.ref_src + (int64_t)v * D.ref_pitch + 3 * u0, u0, w, r);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (four >> j & 1u) {
#pragma unroll
                for (int c = 0; c < 3; ++c) b[j][c] = s_map[c][r[j][c]];
            }
    }
    rgb4_store((rgb_out_ptr)D.dst + (int64_t)v * D.dst_pitch + 3 * u0, u0, w, b);
}

// ---- C ABI ----------------------------------------------------------------------------------
struct DeghostLayout {              // a stack in the workspace
    size_t hist, ranks, maps, frames;   // byte offsets: [k][4][256] uint32, [k][2][256], [k][3][256] bytes
    size_t grey_bytes, mask_bytes, frame_bytes;     // a frame's grey image, one of its two masks, all three
    size_t total;
};

static DeghostLayout deghost_layout(int h, int w, int k) {
    DeghostLayout A;
    A.hist = 0;
    A.ranks = A.hist + align_up((size_t)k * 4096);
    A.maps = A.ranks + align_up((size_t)k * 512);
    A.frames = A.maps + align_up((size_t)k * 768);
    A.grey_bytes = align_up((size_t)h * (size_t)((w + 3) & ~3));
    A.mask_bytes = align_up((size_t)4 * h * (size_t)((w + 31) >> 5));
    A.frame_bytes = A.grey_bytes + 2 * A.mask_bytes;
    A.total = A.frames + (size_t)k * A.frame_bytes;
    return A;
}

extern "C" size_t pano_deghost_work_bytes(int h, int w, int k) {
    return pano_stack_ok(h, w, k) ? deghost_layout(h, w, k).total : 0;
}

static int deghost_check(const pano_deghost_stack &S, int i, const void *work, size_t work_bytes) {
    if (int rc = pano_stack_frames_check("pano_deghost_u8", i, S.src, S.src_pitch, S.dst, S.dst_pitch, S.w, S.h, S.k,
                                         S.reference, work, work_bytes))
        return rc;
    PANO_REQUIRE(S.counts, "pano_deghost_u8: stack %d: null counts", i);
    return PANO_OK;
}

typedef BatchSection<DeghostDev> DeghostSection;    // the records of one launch

template <int TW, int TH>
static void deghost_add(DeghostSection &S, DeghostDev D) {
    batch_section_add<PANO_FUSE_MAX_SIDE, TW, TH, DG_FRAMES>(S, D, D.w, D.h);
}

#define DG_LAUNCH(kernel, S) BATCH_LAUNCH_SECTION(kernel, S, 256, dev, s)

// The stacks [first, first + count) of a call, at most DG_FRAMES frames: one table, five launches.
static int deghost_pass(pano_ctx *ctx, const pano_deghost_stack *stacks, const size_t *at, int first, int count,
                        const pano_deghost_params &P, char *work, hipStream_t s) {
    DeghostSection hist, raw, clean, apply;
    for (int i = first; i < first + count; ++i) {
        const pano_deghost_stack &S = stacks[i];
        const DeghostLayout A = deghost_layout(S.h, S.w, S.k);
        char *base = work + at[i];
        PANO_HIP(hipMemsetAsync(base + A.hist, 0, (size_t)S.k * 4096, s));     // what the kernels add into
        PANO_HIP(hipMemsetAsync(S.counts, 0, (size_t)S.k * 4, s));
        char *ref_frame = base + A.frames + (size_t)S.reference * A.frame_bytes;
        for (int e = 0; e < S.k; ++e) {
            char *frame = base + A.frames + (size_t)e * A.frame_bytes;
            DeghostDev D = {};
            D.src = S.src[e], D.src_pitch = S.src_pitch[e];
            D.ref_src = S.src[S.reference], D.ref_pitch = S.src_pitch[S.reference];
            D.dst = S.dst[e], D.dst_pitch = S.dst_pitch[e];
            D.grey = (uint8_t *)frame, D.ref_grey = (const uint8_t *)ref_frame;
            D.raw = (uint32_t *)(frame + A.grey_bytes), D.mask = (uint32_t *)(frame + A.grey_bytes + A.mask_bytes);
            D.hist = (uint32_t *)(base + A.hist) + (size_t)e * 1024;
            D.ref_hist = (const uint32_t *)(base + A.hist) + (size_t)S.reference * 1024;
            D.ranks = (uint8_t *)(base + A.ranks) + (size_t)e * 512;
            D.ref_ranks = (const uint8_t *)(base + A.ranks) + (size_t)S.reference * 512;
            D.maps = (uint8_t *)(base + A.maps) + (size_t)e * 768;
            D.count = S.counts + e;
            D.w = S.w, D.h = S.h, D.slack = P.slack, D.tol = P.tol, D.erode = P.erode, D.dilate = P.dilate;
            D.is_ref = e == S.reference;
            deghost_add<DG_TILE, DG_TILE>(hist, D);
            if (D.is_ref) continue;
            deghost_add<256, 16>(raw, D);
            deghost_add<32 * DG_CW, DG_CH>(clean, D);
            if (D.dst) deghost_add<64, 16>(apply, D);
        }
    }
    std::vector<DeghostDev> table;
    for (DeghostSection *S : {&hist, &raw, &clean, &apply}) {
        S->first = (int)table.size();
        table.insert(table.end(), S->recs.begin(), S->recs.end());
    }
    if (int rc = pano_buf_upload(ctx, BUF_DEGHOST_DEV, table.data(), table.size() * sizeof(DeghostDev), s)) return rc;
    const DeghostDev *dev = (const DeghostDev *)ctx->buf[BUF_DEGHOST_DEV].p;
    const int frames = (int)hist.recs.size();

    // (timing ids: the tables go with the raw masks)
    PANO_TIMED(PK_DEGHOST_HIST, s, DG_LAUNCH(deghost_hist_kernel, hist));
    if (ctx->timing_on) pano_timing_edge(ctx, PK_DEGHOST_RAW, s, true);
    hipLaunchKernelGGL(deghost_tables_kernel, dim3((unsigned)frames), dim3(256), 0, s, dev + hist.first);
    PANO_LAUNCH_CHECK("deghost_tables_kernel");
    DG_LAUNCH(deghost_raw_kernel, raw);
    if (ctx->timing_on) pano_timing_edge(ctx, PK_DEGHOST_RAW, s, false);
    PANO_TIMED(PK_DEGHOST_CLEAN, s, DG_LAUNCH(deghost_clean_kernel, clean));
    PANO_TIMED(PK_DEGHOST_APPLY, s, DG_LAUNCH(deghost_apply_kernel, apply));

    // the stages a test asked for, out of the workspace
    for (int i = first; i < first + count; ++i) {
        const pano_deghost_stack &S = stacks[i];
        if (!S.hists && !S.ranks && !S.maps && !S.raw && !S.mask) continue;
        const DeghostLayout A = deghost_layout(S.h, S.w, S.k);
        const char *base = work + at[i];
        if (S.hists) PANO_HIP(hipMemcpyAsync(S.hists, base + A.hist, (size_t)S.k * 4096, hipMemcpyDeviceToDevice, s));
        if (S.ranks) PANO_HIP(hipMemcpyAsync(S.ranks, base + A.ranks, (size_t)S.k * 512, hipMemcpyDeviceToDevice, s));
        if (S.maps) PANO_HIP(hipMemcpyAsync(S.maps, base + A.maps, (size_t)S.k * 768, hipMemcpyDeviceToDevice, s));
        const size_t words = (size_t)S.h * (size_t)((S.w + 31) >> 5);
        for (int e = 0; e < S.k; ++e) {
            const char *frame = base + A.frames + (size_t)e * A.frame_bytes + A.grey_bytes;
            uint32_t *const outs[2] = {S.raw, S.mask};
            for (int m = 0; m < 2; ++m) {
                if (!outs[m]) continue;
                if (e == S.reference)                   // (the reference has none: nothing wrote its part)
                    PANO_HIP(hipMemsetAsync(outs[m] + e * words, 0, 4 * words, s));
                else
                    PANO_HIP(hipMemcpyAsync(outs[m] + e * words, frame + m * A.mask_bytes, 4 * words,
                                            hipMemcpyDeviceToDevice, s));
            }
        }
    }
    return PANO_OK;
}

extern "C" int pano_deghost_u8(pano_ctx *ctx, const pano_deghost_stack *stacks, int n,
                               const pano_deghost_params *params, void *work, int64_t work_bytes) {
    PANO_ENTER(ctx, "pano_deghost_u8");
    PANO_REQUIRE(stacks && params && work, "pano_deghost_u8: null pointer");
    PANO_REQUIRE(n >= 1, "pano_deghost_u8: %d stacks", n);
    PANO_REQUIRE(work_bytes >= 0, "pano_deghost_u8: a workspace of %lld bytes", (long long)work_bytes);
    PANO_REQUIRE(params->slack >= 0 && params->slack <= DG_MAX_SLACK, "pano_deghost_u8: slack %d (0 .. %d)",
                 params->slack, DG_MAX_SLACK);
    PANO_REQUIRE(params->tol >= 0 && params->tol <= 255, "pano_deghost_u8: tol %d (0 .. 255)", params->tol);
    PANO_REQUIRE(params->erode >= 0 && params->erode <= DG_MAX_ERODE, "pano_deghost_u8: erode %d (0 .. %d)",
                 params->erode, DG_MAX_ERODE);
    PANO_REQUIRE(params->dilate >= 0 && params->dilate <= DG_MAX_DILATE, "pano_deghost_u8: dilate %d (0 .. %d)",
                 params->dilate, DG_MAX_DILATE);
    std::vector<size_t> at((size_t)n);                  // the stacks' places in the workspace
    size_t need = 0;
    for (int i = 0; i < n; ++i) {                       // (nothing is queued for a refused call)
        if (int rc = deghost_check(stacks[i], i, work, (size_t)work_bytes)) return rc;
        at[i] = need;
        need += deghost_layout(stacks[i].h, stacks[i].w, stacks[i].k).total;
    }
    PANO_REQUIRE(need <= (size_t)work_bytes, "pano_deghost_u8: the stacks need a workspace of %zu bytes, %lld given",
                 need, (long long)work_bytes);
    for (int first = 0; first < n;) {
        int count = 0, frames = 0;
        while (first + count < n && frames + stacks[first + count].k <= DG_FRAMES) frames += stacks[first + count++].k;
        if (int rc = deghost_pass(ctx, stacks, at.data(), first, count, *params, (char *)work, (hipStream_t)stream))
            return rc;
        first += count;
    }
    return PANO_OK;
}
