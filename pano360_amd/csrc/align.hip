// Alignment of hand-held exposure brackets at the ingest (pano_align_mtb, pano_align_work_bytes):
// Ward's median threshold bitmaps.  Every exposure becomes a bitmap "brighter than its own
// median", which hardly depends on the exposure, and an integer translation against the stack's
// reference exposure is found coarse to fine by counting differing bits.  Integers throughout: the
// contract is in include/pano360.h, a NumPy statement of it is tests/align_model.py.
//
// One tile table (batch.h) over all frames of all stacks of a call, a section of it per launch:
//   align_grey_kernel     a 128 x 128 tile of a frame -> its grey values and, in LDS, its part of
//                         every level above (the levels nest), stored; the tile's counts go to the
//                         frame's [L + 1][256] histograms with integer atomicAdd
//   align_median_kernel   a wave per frame and level scans the 256 bins
//   align_bitmap_kernel   tb = g > m and eb = |g - m| > exclude of every level, 32 pixels a word
//   align_search_kernel   one launch per level L .. 0: every workgroup derives the shift so far
//                         from the counters of the levels above, then counts its words' differing
//                         bits for the nine candidates and adds nine integers to this level's
//   align_shift_kernel    the counters -> int32 (dx, dy) per frame
//   align_apply_kernel    frames with a dst and a non-zero shift are copied shifted, the border
//                         replicated; the tiles of the others leave at once
// Integer sums do not depend on the order of the additions: the same input gives the same bytes.
#include "batch.h"
#include "geom.h"
#include "wave.h"

#define AL_MAX_BITS 7               // levels 0 .. 7
#define AL_TILE (1 << AL_MAX_BITS)  // the grey kernel's tile: one pixel of level 7
#define AL_LDS 21848                // 128^2 + 64^2 + ... + 1, rounded up to a dword
#define AL_FRAMES 256               // frames of one pass over the kernels (whole stacks)

struct AlignLevel {                 // level l of a frame in its workspace
    int h, w, pitch, wpr;           // rows, pixels, bytes between grey rows, bitmap words per row
    size_t grey, bits;              // byte offsets in the frame's grey pyramid and in its bitmaps
};

__host__ __device__ __forceinline__ size_t al_a256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// Level l of an h x w frame: h >> l by w >> l; a level's grey rows are a multiple of 4 bytes
// apart, its bitmaps are tb [h_l][wpr_l] then eb [h_l][wpr_l] uint32.
__host__ __device__ __forceinline__ void align_level(int h, int w, int l, AlignLevel &v) {
    v.grey = v.bits = 0;
    for (int j = 0;; ++j) {
        v.h = h >> j, v.w = w >> j;
        v.pitch = (v.w + 3) & ~3, v.wpr = (v.w + 31) >> 5;
        if (j == l) return;
        v.grey += al_a256((size_t)v.h * v.pitch);
        v.bits += al_a256((size_t)8 * v.h * v.wpr);
    }
}

struct AlignDev {                   // a frame (a level of a frame) of a launch, in device memory
    const uint8_t *src;
    uint8_t *dst;
    int64_t src_pitch, dst_pitch;
    uint8_t *grey;                  // the frame's pyramid
    uint32_t *bits;                 // its bitmaps
    const uint32_t *ref_bits;       // those of its stack's reference frame
    uint32_t *hist;                 // [L + 1][256]
    uint32_t *err;                  // [L + 1][9]
    int32_t *med;                   // [L + 1]
    int32_t *shift;                 // the frame's (dx, dy) in the stack's result
    int w, h, L, level, exclude, is_ref;
    TileSlot slot;
};

// ---- stages A and B: grey, pyramid, histograms ---------------------------------------------
// One workgroup per 128 x 128 tile of a frame.  Level 0: a thread takes four neighbouring pixels
// of a row, 16 passes of 8 rows.  The tile's 64 x 64, 32 x 32 ... pixels of the levels above are
// formed in LDS from the level below; pixels outside the frame are 0 there and are neither stored
// nor counted (a pixel inside level l + 1 reads only pixels inside level l).
__global__ __launch_bounds__(256) void align_grey_kernel(const AlignDev *__restrict__ table, int n) {
    __shared__ __attribute__((aligned(4))) uint8_t s_g[AL_LDS];
    __shared__ uint32_t s_hist[AL_MAX_BITS + 1][256];
    int tile;
    const AlignDev &D = batch_record(table, n, tile);
    const int tid = threadIdx.x, L = D.L, h = D.h, w = D.w;
    const int x0 = (tile % D.slot.tiles_x) * AL_TILE, y0 = (tile / D.slot.tiles_x) * AL_TILE;
    for (int l = 0; l <= L; ++l) s_hist[l][tid] = 0;
    __syncthreads();
    AlignLevel V;
    align_level(h, w, 0, V);
    const int qx = (tid & 31) * 4, ry = tid >> 5;
    for (int p = 0; p < AL_TILE / 8; ++p) {
        const int r = p * 8 + ry, y = y0 + r, x = x0 + qx;
        uint32_t g4 = 0;
        if (y < h && x < w) {
            uint32_t b[4][3];
            rgb4_load((frame_ptr)D.src + (int64_t)y * D.src_pitch + 3 * x, x, w, b);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < w) {
                    const uint32_t g = (29u * b[j][0] + 150u * b[j][1] + 77u * b[j][2] + 128u) >> 8;
                    g4 |= g << (8 * j);
                    atomicAdd(&s_hist[0][g], 1u);
                }
            // (x is a multiple of 4 below w: the dword ends inside the row's pitch)
            *(uint32_t *)(D.grey + (size_t)y * V.pitch + x) = g4;
        }
        *(uint32_t *)&s_g[r * AL_TILE + qx] = g4;
    }
    int off = 0;
    for (int l = 1; l <= L; ++l) {
        __syncthreads();
        const int ns = AL_TILE >> (l - 1), nd = AL_TILE >> l, noff = off + ns * ns;
        align_level(h, w, l, V);
        const int lx0 = x0 >> l, ly0 = y0 >> l;
        uint8_t *grey = D.grey + V.grey;
        for (int e = tid; e < nd * nd; e += 256) {
            const int r = e >> (AL_MAX_BITS - l), c = e & (nd - 1);
            const uint8_t *q = s_g + off + 2 * r * ns + 2 * c;
            const uint32_t v = ((uint32_t)q[0] + q[1] + q[ns] + q[ns + 1] + 2u) >> 2;
            s_g[noff + e] = (uint8_t)v;
            if (ly0 + r < V.h && lx0 + c < V.w) {
                grey[(size_t)(ly0 + r) * V.pitch + lx0 + c] = (uint8_t)v;
                atomicAdd(&s_hist[l][v], 1u);
            }
        }
        off = noff;
    }
    __syncthreads();
    for (int l = 0; l <= L; ++l) {
        const uint32_t v = s_hist[l][tid];
        if (v) atomicAdd(&D.hist[l * 256 + tid], v);
    }
}

// ---- stage C: medians ---------------------------------------------------------------------
// One workgroup per frame, wave l its level l: a lane sums four bins, the wave scans the sums,
// and the one lane in whose bins the count reaches (N + 1) / 2 finds the bin.
__global__ __launch_bounds__(64 * (AL_MAX_BITS + 1)) void align_median_kernel(const AlignDev *__restrict__ table) {
    const AlignDev &D = table[blockIdx.x];
    const int l = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (l > D.L) return;
    const uint32_t *bins = D.hist + l * 256 + 4 * lane;
    const uint32_t c[4] = {bins[0], bins[1], bins[2], bins[3]};
    const uint32_t t = (c[0] + c[1]) + (c[2] + c[3]);
    const uint32_t incl = wave_scan_inclusive(t);
    const uint32_t need = ((uint32_t)(D.h >> l) * (uint32_t)(D.w >> l) + 1u) / 2u;
    uint32_t acc = incl - t;
    if (acc < need && need <= incl)
        for (int j = 0; j < 4; ++j) {
            acc += c[j];
            if (acc >= need) {
                D.med[l] = 4 * lane + j;
                break;
            }
        }
}

// ---- stage D: bitmaps ---------------------------------------------------------------------
// One workgroup per 256 x 16 pixels of a level, a wave per row and four rows per wave: a lane
// takes four pixels as one dword, and eight lanes' four bits each meet in a word through three
// exchanges.  Bits from the row's end on are 0.
__global__ __launch_bounds__(256) void align_bitmap_kernel(const AlignDev *__restrict__ table, int n) {
    int tile;
    const AlignDev &D = batch_record(table, n, tile);
    AlignLevel V;
    align_level(D.h, D.w, D.level, V);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = D.med[D.level], ex = D.exclude;
    const int x = (tile % D.slot.tiles_x) * 256 + 4 * lane;
    const uint8_t *grey = D.grey + V.grey;
    uint32_t *tb = D.bits + V.bits / 4, *eb = tb + (size_t)V.h * V.wpr;
    for (int i = 0; i < 4; ++i) {
        const int y = (tile / D.slot.tiles_x) * 16 + wave * 4 + i;
        if (y >= V.h) break;                            // (the whole wave)
        const uint32_t g4 = x < V.w ? *(const uint32_t *)(grey + (size_t)y * V.pitch + x) : 0u;
        uint32_t t = 0, e = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < V.w) {
                const int g = (int)((g4 >> (8 * j)) & 255u);
                t |= (uint32_t)(g > m) << j;
                e |= (uint32_t)(abs(g - m) > ex) << j;
            }
        t <<= 4 * (lane & 7), e <<= 4 * (lane & 7);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            t |= __shfl_xor(t, o, 64);
            e |= __shfl_xor(e, o, 64);
        }
        if ((lane & 7) == 0 && (x >> 5) < V.wpr) {
            tb[(size_t)y * V.wpr + (x >> 5)] = t;
            eb[(size_t)y * V.wpr + (x >> 5)] = e;
        }
    }
}

// ---- stage E: search ----------------------------------------------------------------------
// candidate i of a level: (0, 0) first, then dy = -1, 0, 1 outer and dx = -1, 0, 1 inner
__host__ __device__ __forceinline__ void align_candidate(int i, int &dx, int &dy) {
    const int j = i == 0 ? 4 : (i <= 4 ? i - 1 : i);
    dx = j % 3 - 1, dy = j / 3 - 1;
}

// The shift found by the levels L .. l of a frame, at level l's resolution: s <- 2 s + d, d the
// first candidate with the smallest count.  Every caller computes the same.
__device__ __forceinline__ void align_shift_down_to(const AlignDev &D, int l, int &sx, int &sy) {
    sx = sy = 0;
    for (int lv = D.L; lv >= l; --lv) {
        const uint32_t *e = D.err + lv * 9;
        uint32_t least = e[0];
        int best = 0;
        for (int i = 1; i < 9; ++i)
            if (e[i] < least) least = e[i], best = i;
        int dx, dy;
        align_candidate(best, dx, dy);
        sx = 2 * sx + dx, sy = 2 * sy + dy;
    }
}

// 32 bits from bit `off` (0 .. 33) of the 96 bits w0, w1, w2
__device__ __forceinline__ uint32_t align_bits_at(uint32_t w0, uint32_t w1, uint32_t w2, int off) {
    const uint64_t lo = (uint64_t)w0 | (uint64_t)w1 << 32, hi = (uint64_t)w1 | (uint64_t)w2 << 32;
    return off < 32 ? (uint32_t)(lo >> off) : (uint32_t)(hi >> (off - 32));
}

// One workgroup per 16 words x 64 rows of the reference's bitmap at level D.level, a thread one
// word of four rows.  For a candidate c the frame's bits that face the reference's word xw of row
// y start at bit 32 xw - c.x of row y - c.y: three neighbouring words cover the three dx.  Words
// outside the frame read as 0, and so do the bits past a row's end: eb is 0 there, which is
// "outside the frame" of the contract.
__global__ __launch_bounds__(256) void align_search_kernel(const AlignDev *__restrict__ table, int n) {
    __shared__ uint32_t s_cnt[4][9];
    int tile;
    const AlignDev &D = batch_record(table, n, tile);
    const int l = D.level;
    AlignLevel V;
    align_level(D.h, D.w, l, V);
    int sx, sy;
    align_shift_down_to(D, l + 1, sx, sy);
    sx *= 2, sy *= 2;
    const int wpr = V.wpr;
    const uint32_t *rt = D.ref_bits + V.bits / 4, *re = rt + (size_t)V.h * wpr;
    const uint32_t *ft = D.bits + V.bits / 4, *fe = ft + (size_t)V.h * wpr;
    const int tid = threadIdx.x;
    const int xw = (tile % D.slot.tiles_x) * 16 + (tid & 15);
    uint32_t cnt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (xw < wpr) {
        const int b0 = 32 * xw - sx - 1, q0 = b0 >> 5, o0 = b0 & 31;
        for (int i = 0; i < 4; ++i) {
            const int y = (tile / D.slot.tiles_x) * 64 + (tid >> 4) + 16 * i;
            if (y >= V.h) break;
            const uint32_t a = rt[(size_t)y * wpr + xw], m = re[(size_t)y * wpr + xw];
            if (!m) continue;
#pragma unroll
            for (int r = 0; r < 3; ++r) {               // dy = r - 1
                const int yy = y - (sy + r - 1);
                if ((unsigned)yy >= (unsigned)V.h) continue;
                uint32_t wt[3], we[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const bool in = (unsigned)(q0 + j) < (unsigned)wpr;
                    wt[j] = in ? ft[(size_t)yy * wpr + q0 + j] : 0u;
                    we[j] = in ? fe[(size_t)yy * wpr + q0 + j] : 0u;
                }
#pragma unroll
                for (int t = 0; t < 3; ++t) {           // dx = 1 - t
                    const int j = 3 * r + (2 - t), idx = j == 4 ? 0 : (j < 4 ? j + 1 : j);
                    const uint32_t bt = align_bits_at(wt[0], wt[1], wt[2], o0 + t);
                    const uint32_t be = align_bits_at(we[0], we[1], we[2], o0 + t);
                    cnt[idx] += (uint32_t)__popc((a ^ bt) & m & be);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) cnt[k] = wave_sum(cnt[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) s_cnt[tid >> 6][k] = cnt[k];
    __syncthreads();
    if (tid < 9) {
        const uint32_t total = (s_cnt[0][tid] + s_cnt[1][tid]) + (s_cnt[2][tid] + s_cnt[3][tid]);
        if (total) atomicAdd(&D.err[l * 9 + tid], total);
    }
}

__global__ __launch_bounds__(64) void align_shift_kernel(const AlignDev *__restrict__ table, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const AlignDev &D = table[i];
    int sx = 0, sy = 0;
    if (!D.is_ref) align_shift_down_to(D, 0, sx, sy);
    D.shift[0] = sx, D.shift[1] = sy;
}

// ---- stage F: apply -----------------------------------------------------------------------
// One workgroup per 64 x 16 tile, a thread four neighbouring pixels of a row.  A frame whose
// shift is (0, 0) is not copied: its tiles leave.
__global__ __launch_bounds__(256) void align_apply_kernel(const AlignDev *__restrict__ table, int n) {
    int tile;
    const AlignDev &D = batch_record(table, n, tile);
    const int dx = D.shift[0], dy = D.shift[1];
    if (dx == 0 && dy == 0) return;
    const int w = D.w, h = D.h;
    const int u0 = (tile % D.slot.tiles_x) * 64 + ((int)threadIdx.x & 15) * 4;
    const int v = (tile / D.slot.tiles_x) * 16 + ((int)threadIdx.x >> 4);
    if (u0 >= w || v >= h) return;
    const frame_ptr row = (frame_ptr)D.src + (int64_t)min(max(v - dy, 0), h - 1) * D.src_pitch;
    uint32_t b[4][3];
    if (u0 - dx >= 0 && u0 + 3 - dx <= w - 1) {
        const frame_ptr a = row + 3 * (u0 - dx);
        rgb4_unpack(*(frame_ptr32)a, *(frame_ptr32)(a + 4), *(frame_ptr32)(a + 8), b);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const frame_ptr a = row + 3 * min(max(u0 + j - dx, 0), w - 1);
            b[j][0] = a[0], b[j][1] = a[1], b[j][2] = a[2];
        }
    }
    rgb4_store((rgb_out_ptr)D.dst + (int64_t)v * D.dst_pitch + 3 * u0, u0, w, b);
}

// ---- C ABI --------------------------------------------------------------------------------
static inline int align_levels(int h, int w, int max_bits) {   // min(max_bits, max(0, bit_length(min(h, w)) - 5))
    int side = h < w ? h : w, bits = 0;
    while (side) ++bits, side >>= 1;
    const int L = bits > 5 ? bits - 5 : 0;
    return L < max_bits ? L : max_bits;
}

struct AlignLayout {                // a stack in the workspace, laid out for the levels 0 .. Lm
    int Lm;                         // align_levels(h, w, AL_MAX_BITS)
    size_t hist, err, med, frames;  // byte offsets: [k][Lm + 1][256], [k][Lm + 1][9], [k][Lm + 1]
    size_t grey_bytes, frame_bytes; // a frame's pyramid, and that with its bitmaps
    size_t total;
};

static AlignLayout align_layout(int h, int w, int k) {
    AlignLayout A;
    A.Lm = align_levels(h, w, AL_MAX_BITS);
    const size_t per = (size_t)k * (A.Lm + 1);
    A.hist = 0;
    A.err = A.hist + al_a256(per * 256 * 4);
    A.med = A.err + al_a256(per * 9 * 4);
    A.frames = A.med + al_a256(per * 4);
    AlignLevel V;
    align_level(h, w, A.Lm, V);
    A.grey_bytes = V.grey + al_a256((size_t)V.h * V.pitch);
    A.frame_bytes = A.grey_bytes + V.bits + al_a256((size_t)8 * V.h * V.wpr);
    A.total = A.frames + (size_t)k * A.frame_bytes;
    return A;
}

extern "C" size_t pano_align_work_bytes(int h, int w, int k) {
    return pano_stack_ok(h, w, k) ? align_layout(h, w, k).total : 0;
}

static int align_check(const pano_align_stack &S, int i, const void *work, size_t work_bytes) {
    if (int rc = pano_stack_frames_check("pano_align_mtb", i, S.src, S.src_pitch, S.dst, S.dst_pitch, S.w, S.h, S.k,
                                         S.reference, work, work_bytes))
        return rc;
    PANO_REQUIRE(S.shifts, "pano_align_mtb: stack %d: null shifts", i);
    return PANO_OK;
}

typedef BatchSection<AlignDev> AlignSection;        // the records of one launch

template <int TW, int TH, int CHUNK>
static void align_add(AlignSection &S, AlignDev D, int w, int h) {
    batch_section_add<PANO_FUSE_MAX_SIDE, TW, TH, CHUNK>(S, D, w, h);
}

#define AL_LAUNCH(kernel, S, threads) BATCH_LAUNCH_SECTION(kernel, S, threads, dev, s)

// The stacks [first, first + count) of a call, at most AL_FRAMES frames: one table, every launch.
static int align_pass(pano_ctx *ctx, const pano_align_stack *stacks, const size_t *at, int first, int count,
                      const pano_align_params &P, char *work, hipStream_t s) {
    AlignSection grey, bitmap, apply, search[AL_MAX_BITS + 1];
    int top = 0;
    for (int i = first; i < first + count; ++i) {
        const pano_align_stack &S = stacks[i];
        const AlignLayout A = align_layout(S.h, S.w, S.k);
        char *base = work + at[i];
        PANO_HIP(hipMemsetAsync(base, 0, A.med, s));    // the histograms and the counters
        const int L = align_levels(S.h, S.w, P.max_bits);
        top = L > top ? L : top;
        for (int e = 0; e < S.k; ++e) {
            AlignDev D = {};
            D.src = S.src[e], D.src_pitch = S.src_pitch[e];
            D.dst = S.dst[e], D.dst_pitch = S.dst_pitch[e];
            D.grey = (uint8_t *)(base + A.frames + (size_t)e * A.frame_bytes);
            D.bits = (uint32_t *)(D.grey + A.grey_bytes);
            D.ref_bits = (const uint32_t *)(base + A.frames + (size_t)S.reference * A.frame_bytes + A.grey_bytes);
            D.hist = (uint32_t *)(base + A.hist) + (size_t)e * (A.Lm + 1) * 256;
            D.err = (uint32_t *)(base + A.err) + (size_t)e * (A.Lm + 1) * 9;
            D.med = (int32_t *)(base + A.med) + (size_t)e * (A.Lm + 1);
            D.shift = S.shifts + 2 * e;
            D.w = S.w, D.h = S.h, D.L = L, D.exclude = P.exclude, D.is_ref = e == S.reference;
            align_add<AL_TILE, AL_TILE, AL_FRAMES>(grey, D, S.w, S.h);
            for (int l = 0; l <= L; ++l) {
                D.level = l;
                align_add<256, 16, AL_FRAMES *(AL_MAX_BITS + 1)>(bitmap, D, S.w >> l, S.h >> l);
                if (!D.is_ref) align_add<512, 64, AL_FRAMES>(search[l], D, S.w >> l, S.h >> l);
            }
            D.level = 0;
            if (!D.is_ref && D.dst) align_add<64, 16, AL_FRAMES>(apply, D, S.w, S.h);
        }
    }
    std::vector<AlignDev> table;
    AlignSection *sections[AL_MAX_BITS + 4] = {&grey, &bitmap, &apply};
    for (int l = 0; l <= AL_MAX_BITS; ++l) sections[3 + l] = &search[l];
    for (AlignSection *S : sections) {
        S->first = (int)table.size();
        table.insert(table.end(), S->recs.begin(), S->recs.end());
    }
    if (int rc = pano_buf_upload(ctx, BUF_ALIGN_DEV, table.data(), table.size() * sizeof(AlignDev), s)) return rc;
    const AlignDev *dev = (const AlignDev *)ctx->buf[BUF_ALIGN_DEV].p;
    const int frames = (int)grey.recs.size();

    // (timing ids: the medians go with the bitmaps, the final shifts with the search)
    PANO_TIMED(PK_ALIGN_GREY, s, AL_LAUNCH(align_grey_kernel, grey, 256));
    if (ctx->timing_on) pano_timing_edge(ctx, PK_ALIGN_BITMAP, s, true);
    hipLaunchKernelGGL(align_median_kernel, dim3((unsigned)frames), dim3(64 * (AL_MAX_BITS + 1)), 0, s, dev);
    PANO_LAUNCH_CHECK("align_median_kernel");
    AL_LAUNCH(align_bitmap_kernel, bitmap, 256);
    if (ctx->timing_on) pano_timing_edge(ctx, PK_ALIGN_BITMAP, s, false);
    if (ctx->timing_on) pano_timing_edge(ctx, PK_ALIGN_SEARCH, s, true);
    for (int l = top; l >= 0; --l) AL_LAUNCH(align_search_kernel, search[l], 256);
    hipLaunchKernelGGL(align_shift_kernel, dim3((unsigned)ceil_div(frames, 64)), dim3(64), 0, s, dev, frames);
    PANO_LAUNCH_CHECK("align_shift_kernel");
    if (ctx->timing_on) pano_timing_edge(ctx, PK_ALIGN_SEARCH, s, false);
    PANO_TIMED(PK_ALIGN_APPLY, s, AL_LAUNCH(align_apply_kernel, apply, 256));

    // the stages a test asked for, out of the workspace: dense, the levels 0 .. L one after another
    for (int i = first; i < first + count; ++i) {
        const pano_align_stack &S = stacks[i];
        if (!S.grey && !S.medians && !S.bitmaps && !S.errs) continue;
        const AlignLayout A = align_layout(S.h, S.w, S.k);
        const char *base = work + at[i];
        const int L = align_levels(S.h, S.w, P.max_bits);
        const size_t row = (size_t)(A.Lm + 1) * 4, dense = (size_t)(L + 1) * 4;
        if (S.medians)
            PANO_HIP(hipMemcpy2DAsync(S.medians, dense, base + A.med, row, dense, S.k, hipMemcpyDeviceToDevice, s));
        if (S.errs)
            PANO_HIP(hipMemcpy2DAsync(S.errs, 9 * dense, base + A.err, 9 * row, 9 * dense, S.k,
                                      hipMemcpyDeviceToDevice, s));
        size_t g_at = 0, b_at = 0;                      // (in bytes, in words)
        for (int e = 0; e < S.k; ++e) {
            const char *frame = base + A.frames + (size_t)e * A.frame_bytes;
            for (int l = 0; l <= L; ++l) {
                AlignLevel V;
                align_level(S.h, S.w, l, V);
                if (S.grey)
                    PANO_HIP(hipMemcpy2DAsync(S.grey + g_at, V.w, frame + V.grey, V.pitch, V.w, V.h,
                                              hipMemcpyDeviceToDevice, s));
                if (S.bitmaps)
                    PANO_HIP(hipMemcpyAsync(S.bitmaps + b_at, frame + A.grey_bytes + V.bits, (size_t)8 * V.h * V.wpr,
                                            hipMemcpyDeviceToDevice, s));
                g_at += (size_t)V.h * V.w, b_at += (size_t)2 * V.h * V.wpr;
            }
        }
    }
    return PANO_OK;
}

extern "C" int pano_align_mtb(pano_ctx *ctx, const pano_align_stack *stacks, int n, const pano_align_params *params,
                              void *work, int64_t work_bytes) {
    PANO_ENTER(ctx, "pano_align_mtb");
    PANO_REQUIRE(stacks && params && work, "pano_align_mtb: null pointer");
    PANO_REQUIRE(n >= 1, "pano_align_mtb: %d stacks", n);
    PANO_REQUIRE(work_bytes >= 0, "pano_align_mtb: a workspace of %lld bytes", (long long)work_bytes);
    PANO_REQUIRE(params->max_bits >= 0 && params->max_bits <= AL_MAX_BITS, "pano_align_mtb: max_bits %d (0 .. %d)",
                 params->max_bits, AL_MAX_BITS);
    PANO_REQUIRE(params->exclude >= 0 && params->exclude <= 127, "pano_align_mtb: exclude %d (0 .. 127)",
                 params->exclude);
    std::vector<size_t> at((size_t)n);                  // the stacks' places in the workspace
    size_t need = 0;
    for (int i = 0; i < n; ++i) {                       // (nothing is queued for a refused call)
        if (int rc = align_check(stacks[i], i, work, (size_t)work_bytes)) return rc;
        at[i] = need;
        need += align_layout(stacks[i].h, stacks[i].w, stacks[i].k).total;
    }
    PANO_REQUIRE(need <= (size_t)work_bytes, "pano_align_mtb: the stacks need a workspace of %zu bytes, %lld given",
                 need, (long long)work_bytes);
    for (int first = 0; first < n;) {
        int count = 0, frames = 0;
        while (first + count < n && frames + stacks[first + count].k <= AL_FRAMES) frames += stacks[first + count++].k;
        if (int rc = align_pass(ctx, stacks, at.data(), first, count, *params, (char *)work, (hipStream_t)stream))
            return rc;
        first += count;
    }
    return PANO_OK;
}
