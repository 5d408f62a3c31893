// PNG output (pano_png_filter, pano_deflate, pano_deflate_lengths): the scanline filters with
// the minimum-sum-of-absolute-values choice per row, and a deflate coder that finds runs of equal
// bytes (matches at distance 1 only) and codes every DEFLATE_CHUNK input bytes as one dynamic
// Huffman block with optimal length-limited codes (package-merge).  The contract (what the file
// guarantees, the scratch layout, the waits) is in include/pano360.h; the host side (the zlib
// wrapper, the chunks of the PNG container) is pano360_amd/png.py and a NumPy restatement of the
// filter rule and of the run tokeniser is tests/png_model.py.
#include "common.h"
#include "wave.h"

#define FILT_BLOCK 256
#define FILT_MAX_GROUPS (1 << 20)   // grid cap of the filter kernel (it loops beyond it)

#define DEFLATE_CHUNK PANO_DEFLATE_CHUNK
#define DEF_BLOCK 1024              // threads of a chunk's workgroup
#define DEF_SPAN (DEFLATE_CHUNK / DEF_BLOCK)   // input bytes per thread: 64, one mask word
#define DEF_SPAN_WORDS (DEF_SPAN / 4)
#define DEF_STRIDE_WORDS (DEF_SPAN_WORDS + 1)  // LDS words per span: odd, so lanes hit distinct banks
#define DEF_POOL_WORDS (DEF_BLOCK * DEF_STRIDE_WORDS)
#define DEF_MAX_GROUPS 4096         // grid cap of the chunk kernels (they loop beyond it)
#define DEF_LIT 286                 // literal/length symbols
#define DEF_DIST 30                 // distance symbols
#define DEF_DIST_AT 288             // where the distance alphabet starts in the joint arrays
#define DEF_SYMS 320                // joint array size
#define DEF_HDR_WORDS 160           // >= (17 + 19 * 3 + 316 * 14 bits + 31) / 32 + 1
#define DEF_MAX_MATCH 258
#define DEF_ADLER 65521u

static_assert(DEF_SPAN == 64, "one 64-bit mask of run starts per thread");

// ---- 1. the scanline filters ------------------------------------------------------------------------
struct PngImage {
    const uint8_t *img;             // pixel (x, y) at img[y * pitch + 3 x], RGB or BGR
    int64_t pitch;
    int h, w, bgr;
};

__device__ __forceinline__ int png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}

// the five filtered values of one byte: x the byte, a left, b up, c upper left
__device__ __forceinline__ void png_filters(int x, int a, int b, int c, uint8_t f[5]) {
    f[0] = (uint8_t)x;
    f[1] = (uint8_t)(x - a);
    f[2] = (uint8_t)(x - b);
    f[3] = (uint8_t)(x - ((a + b) >> 1));
    f[4] = (uint8_t)(x - png_paeth(a, b, c));
}

// One workgroup per row: the five sums of |filtered byte as int8| over the row, the choice (the
// first minimum in the order 0 .. 4), then the chosen filter written.  Every candidate comes
// from the unfiltered neighbours, so rows are independent.
__global__ __launch_bounds__(FILT_BLOCK) void png_filter_kernel(PngImage P,
                                                                uint8_t *__restrict__ out) {
    __shared__ unsigned long long sums[FILT_BLOCK / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = P.bgr ? 2 : 0, c2 = 2 - c0;
    const int64_t row_bytes = 1 + 3 * (int64_t)P.w;
    for (int64_t y = blockIdx.x; y < P.h; y += gridDim.x) {
        const uint8_t *cur = P.img + y * P.pitch;
        const uint8_t *up = y ? cur - P.pitch : nullptr;
        auto load = [&](int64_t x, int px[4][3]) {   // px[0] the pixel, [1] left, [2] up, [3] upper left
            const int64_t o = 3 * x;
            const int order[3] = {c0, 1, c2};
            for (int k = 0; k < 3; ++k) {
                const int64_t i = o + order[k];
                px[0][k] = cur[i];
                px[1][k] = x ? cur[i - 3] : 0;
                px[2][k] = up ? up[i] : 0;
                px[3][k] = up && x ? up[i - 3] : 0;
            }
        };
        unsigned long long s[5] = {0, 0, 0, 0, 0};
        for (int64_t x = tid; x < P.w; x += FILT_BLOCK) {
            int px[4][3];
            load(x, px);
            for (int k = 0; k < 3; ++k) {
                uint8_t f[5];
                png_filters(px[0][k], px[1][k], px[2][k], px[3][k], f);
                for (int m = 0; m < 5; ++m) s[m] += (unsigned)abs((int)(int8_t)f[m]);
            }
        }
        for (int m = 0; m < 5; ++m) {
            s[m] = wave_sum(s[m]);
            if (lane == 0) sums[wave][m] = s[m];
        }
        __syncthreads();
        int best = 0;
        unsigned long long best_sum = 0;
        for (int m = 0; m < 5; ++m) {
            unsigned long long t = 0;
            for (int v = 0; v < FILT_BLOCK / 64; ++v) t += sums[v][m];
            if (m == 0 || t < best_sum) {
                best = m;
                best_sum = t;
            }
        }
        uint8_t *dst = out + y * row_bytes;
        if (tid == 0) dst[0] = (uint8_t)best;
        for (int64_t x = tid; x < P.w; x += FILT_BLOCK) {
            int px[4][3];
            load(x, px);
            for (int k = 0; k < 3; ++k) {
                uint8_t f[5];
                png_filters(px[0][k], px[1][k], px[2][k], px[3][k], f);
                dst[1 + 3 * x + k] = f[best];
            }
        }
        __syncthreads();
    }
}

// ---- 2. length-limited Huffman code lengths: package-merge, one workgroup ---------------------------
// The used symbols are sorted by (frequency, index) by counting.  Level 1 of the package-merge is
// the sorted leaves; level l + 1 merges the leaves with the packages of level l (pairs of its
// items, in order), leaves first among equal weights.  Both lists are sorted, so an item's place
// is its index plus a binary search in the other list: one parallel step per level.  Only the
// leaves' places are kept.  The first 2n - 2 items of the top level are the solution; walking
// down, the first t items of a level hold c leaves (a binary search in that level's places) and
// t - c packages, which are the first 2 (t - c) items of the level below.  A symbol's length is
// the number of levels whose chosen prefix holds its leaf.  The result is an optimal code under
// the limit: Kraft sum exactly 1 for two or more used symbols; one used symbol gets length 1.
struct PmScratch {
    unsigned long long leaf[288];
    unsigned long long W[2][576];
    unsigned long long PW[288];
    uint16_t pos[15][288];
    uint16_t sym[288];
    int n;
};
static_assert(sizeof(PmScratch) <= DEF_POOL_WORDS * 4, "the scratch lives in the chunk's pool");

// freq, lens: LDS, n_sym <= 288, 1 <= max_bits <= 15, n_sym <= 2^max_bits; every thread of a
// workgroup of at least 2 n_sym threads calls it; lens is valid after it returns
__device__ void pm_lengths(const uint32_t *freq, int n_sym, int max_bits, uint8_t *lens,
                           PmScratch &S) {
    const int tid = threadIdx.x;
    if (tid == 0) S.n = 0;
    __syncthreads();
    if (tid < n_sym) {
        const uint32_t f = freq[tid];
        lens[tid] = 0;
        if (f) {
            int rank = 0;
            for (int j = 0; j < n_sym; ++j) {
                const uint32_t fj = freq[j];
                rank += fj && (fj < f || (fj == f && j < tid));
            }
            S.leaf[rank] = f;
            S.sym[rank] = (uint16_t)tid;
            atomicAdd(&S.n, 1);
        }
    }
    __syncthreads();
    const int n = S.n;
    __syncthreads();                                // (every path leaves S reusable)
    if (n == 0) return;
    if (n == 1) {
        if (tid == 0) lens[S.sym[0]] = 1;
        __syncthreads();
        return;
    }
    if (tid < n) {
        S.W[0][tid] = S.leaf[tid];
        S.pos[0][tid] = (uint16_t)tid;
    }
    int m = n, cur = 0;
    for (int l = 1; l < max_bits; ++l) {
        __syncthreads();
        const int np = m >> 1;
        if (tid < np) S.PW[tid] = S.W[cur][2 * tid] + S.W[cur][2 * tid + 1];
        __syncthreads();
        if (tid < n) {
            const unsigned long long w = S.leaf[tid];
            int lo = 0, hi = np;                    // packages lighter than the leaf
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (S.PW[mid] < w) lo = mid + 1;
                else hi = mid;
            }
            S.W[cur ^ 1][tid + lo] = w;
            S.pos[l][tid] = (uint16_t)(tid + lo);
        } else if (tid < n + np) {
            const int j = tid - n;
            const unsigned long long w = S.PW[j];
            int lo = 0, hi = n;                     // leaves no heavier than the package
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (S.leaf[mid] <= w) lo = mid + 1;
                else hi = mid;
            }
            S.W[cur ^ 1][j + lo] = w;
        }
        m = n + np;
        cur ^= 1;
    }
    __syncthreads();
    if (tid < n) {
        int t = 2 * n - 2, len = 0;
        for (int l = max_bits - 1; l >= 0 && t > 0; --l) {
            int lo = 0, hi = n;                     // leaves among the first t items of the level
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (S.pos[l][mid] < t) lo = mid + 1;
                else hi = mid;
            }
            len += tid < lo;
            t = 2 * (t - lo);
        }
        lens[S.sym[tid]] = (uint8_t)len;
    }
    __syncthreads();
}

__global__ __launch_bounds__(DEF_BLOCK) void deflate_lengths_kernel(
    const uint32_t *__restrict__ freq, int n_sym, int max_bits, uint8_t *__restrict__ lengths) {
    __shared__ PmScratch S;
    __shared__ uint32_t f[288];
    __shared__ uint8_t lens[288];
    if ((int)threadIdx.x < n_sym) f[threadIdx.x] = freq[threadIdx.x];
    __syncthreads();
    pm_lengths(f, n_sym, max_bits, lens, S);
    if ((int)threadIdx.x < n_sym) lengths[threadIdx.x] = lens[threadIdx.x];
}

// ---- 3. the chunk in LDS and its runs ------------------------------------------------------------
// What kernel 4 leaves per chunk for kernel 6
struct DefRecord {
    uint8_t lens[DEF_SYMS];         // code lengths: literal/length at 0, distance at DEF_DIST_AT
    uint32_t hdr_bits;
    uint32_t pad[15];
    uint32_t hdr[DEF_HDR_WORDS];    // the block header, LSB first
};
static_assert(sizeof(DefRecord) == 1024, "one KiB per chunk");

// A thread's view of its DEF_SPAN bytes of the chunk
struct DefSpan {
    const uint8_t *bytes;           // LDS: the span's bytes
    unsigned long long starts;      // bit j: byte j of the span starts a run (differs from the byte before it)
    int span0, end;                 // the span's bytes [span0, end) of the chunk (end <= chunk length)
    int incoming;                   // chunk index of the last run start before the span, -1: none
    int next;                       // chunk index of the first run start after the span, or the chunk length
};

// The chunk's bytes into the pool (span t at word t * DEF_STRIDE_WORDS, zeros past the end), and
// every thread's span.  `wt` is 2 * (DEF_BLOCK / 64) ints of LDS.  Ends with the pool readable.
__device__ DefSpan def_load(const uint8_t *__restrict__ data, int64_t n, int64_t chunk,
                            uint32_t *pool, int *wt, uint32_t w[DEF_SPAN_WORDS]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t c0 = chunk * DEFLATE_CHUNK;
    const int clen = (int)(n - c0 < DEFLATE_CHUNK ? n - c0 : DEFLATE_CHUNK);
    const uint8_t *src = data + c0;
    const bool aligned = ((uintptr_t)data & 3) == 0;
    for (int g = tid; g < DEFLATE_CHUNK / 4; g += DEF_BLOCK) {
        uint32_t v = 0;
        if (aligned && 4 * g + 4 <= clen) {
            v = *(const uint32_t *)(src + 4 * g);
        } else {
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < clen) v |= (uint32_t)src[4 * g + k] << (8 * k);
        }
        pool[(g / DEF_SPAN_WORDS) * DEF_STRIDE_WORDS + g % DEF_SPAN_WORDS] = v;
    }
    __syncthreads();
    DefSpan sp;
    sp.bytes = (const uint8_t *)(pool + tid * DEF_STRIDE_WORDS);
    sp.span0 = tid * DEF_SPAN;
    sp.end = sp.span0 + DEF_SPAN < clen ? sp.span0 + DEF_SPAN : clen;
    for (int k = 0; k < DEF_SPAN_WORDS; ++k) w[k] = pool[tid * DEF_STRIDE_WORDS + k];
    // the byte before the span; byte 0 of the buffer starts a run whatever it is
    uint32_t prev = 0;
    bool force = false;
    if (tid > 0) prev = pool[(tid - 1) * DEF_STRIDE_WORDS + DEF_SPAN_WORDS - 1] >> 24;
    else if (c0 > 0) prev = src[-1];
    else force = true;
    unsigned long long starts = 0;
    for (int k = 0; k < DEF_SPAN_WORDS; ++k) {
        const uint32_t x = w[k] ^ (w[k] << 8 | prev);
        for (int b = 0; b < 4; ++b)
            if ((x >> (8 * b)) & 0xFF) starts |= 1ull << (4 * k + b);
        prev = w[k] >> 24;
    }
    if (force) starts |= 1;
    const int valid = sp.end - sp.span0;
    starts = valid <= 0 ? 0 : valid >= 64 ? starts : starts & ((1ull << valid) - 1);
    sp.starts = starts;
    // the last start before the span (a max scan) and the first one after it (a min scan from the right)
    const int last = starts ? sp.span0 + 63 - __clzll(starts) : -1;
    const int first = starts ? sp.span0 + __ffsll((long long)starts) - 1 : clen;
    int up = last, down = first;
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(up, o, 64), b = __shfl_down(down, o, 64);
        if (lane >= o) up = max(up, a);
        if (lane + o < 64) down = min(down, b);
    }
    if (lane == 63) wt[wave] = up;
    if (lane == 0) wt[DEF_BLOCK / 64 + wave] = down;
    const int up_before = __shfl_up(up, 1, 64), down_after = __shfl_down(down, 1, 64);
    __syncthreads();
    int incoming = lane ? up_before : -1, next = lane < 63 ? down_after : clen;
    for (int v = 0; v < DEF_BLOCK / 64; ++v) {
        if (v < wave) incoming = max(incoming, wt[v]);
        if (v > wave) next = min(next, wt[DEF_BLOCK / 64 + v]);
    }
    sp.incoming = incoming;
    sp.next = next;
    return sp;
}

// The tokens that start in the span, in order: lit(byte) and match(length), every match at
// distance 1.  A run's first byte is a literal; the rest of it, cut at the chunk's borders (a
// run that began before the chunk has no first byte here: its matches reach the byte before the
// chunk), is matches of DEF_MAX_MATCH and one of the remainder, or 1 - 2 literals if that is
// below 3.
template <class Lit, class Match>
__device__ __forceinline__ void def_walk(const DefSpan &sp, Lit &&lit, Match &&match) {
    int i = sp.span0, run_start = sp.incoming;
    while (i < sp.end) {
        const int rel = i - sp.span0;
        if ((sp.starts >> rel) & 1) {
            lit(sp.bytes[rel]);
            run_start = i++;
            continue;
        }
        const int base = run_start + 1;             // first byte of the run's rest in this chunk
        const unsigned long long later = rel < 63 ? sp.starts >> (rel + 1) : 0;
        const int e = later ? i + __ffsll((long long)later) : sp.next;   // the run's end in the chunk
        const int seg_end = e < sp.end ? e : sp.end;
        const uint8_t v = sp.bytes[rel];
        int p = i;
        while (p < seg_end) {
            const int r = (p - base) % DEF_MAX_MATCH;
            const int left = e - (p - r), tlen = left < DEF_MAX_MATCH ? left : DEF_MAX_MATCH;
            if (tlen >= 3) {
                if (r == 0) match(tlen);
                p += tlen - r;
            } else {
                lit(v);
                ++p;
            }
        }
        i = seg_end;
    }
}

// length 3 .. 258 -> its symbol, the number of extra bits and their value (RFC 1951, 3.2.5)
__device__ __forceinline__ void def_length_code(int len, int &sym, int &nextra, int &extra) {
    const int v = len - 3;
    if (v < 8) {
        sym = 257 + v;
        nextra = extra = 0;
    } else if (v == 255) {
        sym = 285;
        nextra = extra = 0;
    } else {
        const int eb = 29 - __clz(v);               // floor(log2 v) - 2
        const int rest = v - (4 << eb);
        sym = 261 + 4 * eb + (rest >> eb);
        nextra = eb;
        extra = rest & ((1 << eb) - 1);
    }
}
__device__ __forceinline__ int def_extra_bits(int sym) {
    return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2;
}

// the chunk's pool: dynamic LDS (with the rest a workgroup passes the 64 KiB a kernel gets unasked)
extern __shared__ __align__(16) uint32_t def_pool[];

// ---- 4. per chunk: histograms, code lengths, the block header, the bit count, Adler partials --------
__constant__ uint8_t kDefClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DefHeaderState {
    uint8_t rle_sym[DEF_SYMS], rle_extra[DEF_SYMS];
    uint32_t cl_freq[19];
    uint8_t cl_lens[19];
    uint32_t cl_code[19];
    int n_rle, hlit, hdist;
};

__device__ __forceinline__ void def_hdr_put(uint32_t *hdr, int &pos, uint32_t v, int nbits) {
    if (!nbits) return;
    hdr[pos >> 5] |= v << (pos & 31);
    if ((pos & 31) + nbits > 32) hdr[(pos >> 5) + 1] |= v >> (32 - (pos & 31));
    pos += nbits;
}

// the canonical code of symbol s (lengths lens[0 .. n)), bit-reversed for the LSB-first stream
__device__ __forceinline__ uint32_t def_code(const uint8_t *lens, int n, int s) {
    const int len = lens[s];
    if (!len) return 0;
    uint32_t code = 0;
    for (int j = 0; j < n; ++j) {
        const int lj = lens[j];
        if (lj && lj < len) code += 1u << (len - lj);
        else if (lj == len && j < s) ++code;
    }
    return __brev(code) >> (32 - len);
}

// one thread: the code lengths of both alphabets as symbols of the code-length alphabet
__device__ void def_header_rle(const uint8_t *lens, DefHeaderState &H) {
    int hlit = DEF_LIT, hdist = DEF_DIST;
    while (hlit > 257 && !lens[hlit - 1]) --hlit;
    while (hdist > 1 && !lens[DEF_DIST_AT + hdist - 1]) --hdist;
    H.hlit = hlit;
    H.hdist = hdist;
    for (int k = 0; k < 19; ++k) H.cl_freq[k] = 0;
    const int total = hlit + hdist;
    auto at = [&](int i) { return (int)lens[i < hlit ? i : DEF_DIST_AT + i - hlit]; };
    int k = 0;
    auto emit = [&](int sym, int extra) {
        H.rle_sym[k] = (uint8_t)sym;
        H.rle_extra[k] = (uint8_t)extra;
        ++H.cl_freq[sym];
        ++k;
    };
    for (int i = 0; i < total;) {
        const int v = at(i);
        int run = 1;
        while (i + run < total && at(i + run) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int t = run < 138 ? run : 138;
                emit(18, t - 11);
                run -= t;
            }
            if (run >= 3) {
                emit(17, run - 3);
                run = 0;
            }
            for (; run > 0; --run) emit(0, 0);
        } else {
            emit(v, 0);
            --run;
            while (run >= 3) {
                const int t = run < 6 ? run : 6;
                emit(16, t - 3);
                run -= t;
            }
            for (; run > 0; --run) emit(v, 0);
        }
    }
    H.n_rle = k;
}

// one thread: BFINAL, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code, the coded lengths
__device__ int def_header_bits(DefHeaderState &H, bool final_block, uint32_t *hdr) {
    int pos = 0;
    def_hdr_put(hdr, pos, final_block ? 1 : 0, 1);
    def_hdr_put(hdr, pos, 2, 2);
    int hclen = 19;
    while (hclen > 4 && !H.cl_lens[kDefClOrder[hclen - 1]]) --hclen;
    def_hdr_put(hdr, pos, H.hlit - 257, 5);
    def_hdr_put(hdr, pos, H.hdist - 1, 5);
    def_hdr_put(hdr, pos, hclen - 4, 4);
    for (int k = 0; k < hclen; ++k) def_hdr_put(hdr, pos, H.cl_lens[kDefClOrder[k]], 3);
    for (int s = 0; s < 19; ++s) H.cl_code[s] = def_code(H.cl_lens, 19, s);
    for (int k = 0; k < H.n_rle; ++k) {
        const int s = H.rle_sym[k];
        def_hdr_put(hdr, pos, H.cl_code[s], H.cl_lens[s]);
        if (s >= 16) def_hdr_put(hdr, pos, H.rle_extra[k], s == 16 ? 2 : s == 17 ? 3 : 7);
    }
    return pos;
}

__global__ __launch_bounds__(DEF_BLOCK) void deflate_code_kernel(
    const uint8_t *__restrict__ data, int64_t n, int64_t nchunks, DefRecord *__restrict__ recs,
    uint32_t *__restrict__ bits, uint32_t *__restrict__ adler) {
    uint32_t *pool = def_pool;
    __shared__ int wt[2 * (DEF_BLOCK / 64)];
    __shared__ uint32_t hist[DEF_SYMS];
    __shared__ uint8_t lens[DEF_SYMS];
    __shared__ uint32_t hdr[DEF_HDR_WORDS];
    __shared__ DefHeaderState H;
    __shared__ uint32_t sum_a, total_bits;
    __shared__ unsigned long long sum_b;
    __shared__ int hdr_bits;
    const int tid = threadIdx.x;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (tid < DEF_SYMS) {
            hist[tid] = 0;
            lens[tid] = 0;
        }
        if (tid < DEF_HDR_WORDS) hdr[tid] = 0;
        if (tid == 0) {
            sum_a = 0;
            total_bits = 0;
            sum_b = 0;
        }
        uint32_t w[DEF_SPAN_WORDS];
        const DefSpan sp = def_load(data, n, chunk, pool, wt, w);   // (its barriers order the zeroing)
        def_walk(
            sp, [&](uint8_t v) { atomicAdd(&hist[v], 1u); },
            [&](int len) {
                int sym, nextra, extra;
                def_length_code(len, sym, nextra, extra);
                atomicAdd(&hist[sym], 1u);
                atomicAdd(&hist[DEF_DIST_AT], 1u);
            });
        // Adler-32 partials of the chunk: a = sum d[i], b = sum (length - i) d[i]
        const int64_t c0 = chunk * DEFLATE_CHUNK;
        const int clen = (int)(n - c0 < DEFLATE_CHUNK ? n - c0 : DEFLATE_CHUNK);
        if (sp.span0 < sp.end) {
            uint32_t a = 0;
            unsigned long long b = 0;
#pragma unroll
            for (int k = 0; k < DEF_SPAN; ++k) {    // (zeros past the chunk's end)
                const uint32_t d = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
                a += d;
                b += (unsigned long long)(clen - sp.span0 - k) * d;
            }
            atomicAdd(&sum_a, a);
            atomicAdd(&sum_b, b);
        }
        if (tid == 0) atomicAdd(&hist[256], 1u);    // the end-of-block symbol
        __syncthreads();
        PmScratch &S = *(PmScratch *)pool;          // the chunk's bytes are not needed any more
        pm_lengths(hist, DEF_LIT, 15, lens, S);
        pm_lengths(hist + DEF_DIST_AT, DEF_DIST, 15, lens + DEF_DIST_AT, S);
        if (tid == 0) def_header_rle(lens, H);
        __syncthreads();
        pm_lengths(H.cl_freq, 19, 7, H.cl_lens, S);
        if (tid == 0) hdr_bits = def_header_bits(H, chunk == nchunks - 1, hdr);
        if (tid < DEF_LIT) atomicAdd(&total_bits, hist[tid] * (lens[tid] + def_extra_bits(tid)));
        if (tid == DEF_DIST_AT) atomicAdd(&total_bits, hist[tid] * lens[tid]);
        __syncthreads();
        DefRecord &R = recs[chunk];
        if (tid < DEF_SYMS) R.lens[tid] = lens[tid];
        if (tid < DEF_HDR_WORDS) R.hdr[tid] = hdr[tid];
        if (tid == 0) {
            R.hdr_bits = (uint32_t)hdr_bits;
            bits[chunk] = total_bits + (uint32_t)hdr_bits;
            adler[2 * chunk] = sum_a % DEF_ADLER;
            adler[2 * chunk + 1] = (uint32_t)(sum_b % DEF_ADLER);
        }
        __syncthreads();
    }
}

// ---- 5. exclusive scan of the chunks' bit counts into int64 offsets; offs[n] = the total -------------
// (wave.h: scan_exclusive_kernel)

// ---- 6. emission ------------------------------------------------------------------------------------
// A thread's bits go into the zeroed stream LSB first: the words wholly inside its bit range are
// stored, its first and last word, which it may share with its neighbours, are ORed atomically
// (integer, disjoint bits: the order does not matter).
struct DefBitOut {
    uint32_t *out;
    int64_t word, limit;            // (a word at or past `limit` is never written)
    unsigned long long acc;
    int nacc;
    bool shared_first;
    __device__ void begin(uint32_t *o, int64_t words, int64_t bit) {
        out = o;
        limit = words;
        word = bit >> 5;
        acc = 0;
        nacc = (int)(bit & 31);
        shared_first = nacc != 0;
    }
    __device__ __forceinline__ void put(uint32_t v, int nbits) {   // nbits <= 16
        acc |= (unsigned long long)v << nacc;
        nacc += nbits;
        if (nacc >= 32) {
            if (word >= limit) {
            } else if (shared_first) {
                atomicOr(&out[word], (uint32_t)acc);
            } else {
                out[word] = (uint32_t)acc;
            }
            shared_first = false;
            ++word;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ void end() {
        if (nacc && (uint32_t)acc && word < limit) atomicOr(&out[word], (uint32_t)acc);
    }
};

__global__ __launch_bounds__(DEF_BLOCK) void deflate_emit_kernel(
    const uint8_t *__restrict__ data, int64_t n, int64_t nchunks, const DefRecord *__restrict__ recs,
    const int64_t *__restrict__ offs, uint32_t *__restrict__ out, int64_t out_words) {
    uint32_t *pool = def_pool;
    __shared__ int wt[2 * (DEF_BLOCK / 64)];
    __shared__ uint8_t lens[DEF_SYMS];
    __shared__ uint32_t code[DEF_SYMS];             // (length << 16) | the reversed code
    __shared__ uint32_t hdr[DEF_HDR_WORDS];
    __shared__ int wave_bits[DEF_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const DefRecord &R = recs[chunk];
        if (tid < DEF_SYMS) lens[tid] = R.lens[tid];
        if (tid < DEF_HDR_WORDS) hdr[tid] = R.hdr[tid];
        uint32_t w[DEF_SPAN_WORDS];
        const DefSpan sp = def_load(data, n, chunk, pool, wt, w);   // (its barriers publish lens, hdr)
        if (tid < DEF_LIT) code[tid] = (uint32_t)lens[tid] << 16 | def_code(lens, DEF_LIT, tid);
        else if (tid >= DEF_DIST_AT && tid < DEF_DIST_AT + DEF_DIST)
            code[tid] = (uint32_t)lens[tid] << 16 |
                        def_code(lens + DEF_DIST_AT, DEF_DIST, tid - DEF_DIST_AT);
        const int dist_len = lens[DEF_DIST_AT];
        // the bits of the span's tokens; the last thread also writes the end-of-block symbol
        int count = 0;
        def_walk(
            sp, [&](uint8_t v) { count += lens[v]; },
            [&](int len) {
                int sym, nextra, extra;
                def_length_code(len, sym, nextra, extra);
                count += lens[sym] + nextra + dist_len;
            });
        if (tid == DEF_BLOCK - 1) count += lens[256];
        const int x = wave_scan_inclusive(count);
        if (lane == 63) wave_bits[wave] = x;
        __syncthreads();                            // (also publishes code[])
        int before = 0;
        for (int k = 0; k < wave; ++k) before += wave_bits[k];
        const int64_t chunk_bit = offs[chunk];
        const int hdr_bits = (int)R.hdr_bits;
        DefBitOut B;
        B.begin(out, out_words, chunk_bit + hdr_bits + before + x - count);
        const uint32_t dist_code = code[DEF_DIST_AT];
        def_walk(
            sp, [&](uint8_t v) { B.put(code[v] & 0xFFFF, (int)(code[v] >> 16)); },
            [&](int len) {
                int sym, nextra, extra;
                def_length_code(len, sym, nextra, extra);
                B.put(code[sym] & 0xFFFF, (int)(code[sym] >> 16));
                B.put((uint32_t)extra, nextra);
                B.put(dist_code & 0xFFFF, (int)(dist_code >> 16));
            });
        if (tid == DEF_BLOCK - 1) B.put(code[256] & 0xFFFF, (int)(code[256] >> 16));
        B.end();
        // the header, shifted to the chunk's bit offset
        const int sh = (int)(chunk_bit & 31), nwords = (sh + hdr_bits + 31) >> 5;
        if (tid < nwords) {
            const uint32_t lo = tid < DEF_HDR_WORDS ? hdr[tid] : 0;
            const uint32_t hi = tid > 0 && tid - 1 < DEF_HDR_WORDS ? hdr[tid - 1] : 0;
            const uint32_t v = sh ? lo << sh | hi >> (32 - sh) : lo;
            uint32_t *dst = out + (chunk_bit >> 5) + tid;
            const bool inside = (tid > 0 || sh == 0) && 32 * (tid + 1) <= sh + hdr_bits;
            if ((chunk_bit >> 5) + tid >= out_words) {
            } else if (inside) {
                *dst = v;
            } else {
                atomicOr(dst, v);
            }
        }
        __syncthreads();
    }
}

// ---- the entry points ------------------------------------------------------------------------------
extern "C" int pano_png_filter(pano_ctx *ctx, const uint8_t *img, int h, int w, int64_t pitch,
                               int flags, uint8_t *filtered) {
    PANO_ENTER(ctx, "pano_png_filter");
    PANO_REQUIRE(img && filtered, "pano_png_filter: null pointer");
    PANO_REQUIRE(h >= 1 && w >= 1, "pano_png_filter: %d x %d", w, h);
    PANO_REQUIRE(pitch >= 3 * (int64_t)w && (flags & ~PANO_PNG_BGR) == 0,
                 "pano_png_filter: pitch %lld for %d pixels, flags %d", (long long)pitch, w, flags);
    PngImage P;
    P.img = img;
    P.pitch = pitch;
    P.h = h;
    P.w = w;
    P.bgr = flags & PANO_PNG_BGR;
    const hipStream_t s = (hipStream_t)stream;
    PANO_TIMED(PK_PNG_FILTER, s,
               hipLaunchKernelGGL(png_filter_kernel, capped_grid(h, FILT_MAX_GROUPS),
                                  dim3(FILT_BLOCK), 0, s, P, filtered));
    PANO_LAUNCH_CHECK("png_filter_kernel");
    return PANO_OK;
}

extern "C" int pano_deflate_lengths(pano_ctx *ctx, const uint32_t *freq, int n_sym, int max_bits,
                                    uint8_t *lengths) {
    PANO_ENTER(ctx, "pano_deflate_lengths");
    PANO_REQUIRE(freq && lengths, "pano_deflate_lengths: null pointer");
    PANO_REQUIRE(n_sym >= 1 && n_sym <= 288 && max_bits >= 1 && max_bits <= 15 &&
                     n_sym <= (1 << max_bits),
                 "pano_deflate_lengths: %d symbols in %d bits (1..288 symbols, 1..15 bits, "
                 "symbols <= 2^bits)", n_sym, max_bits);
    const hipStream_t s = (hipStream_t)stream;
    PANO_TIMED(PK_DEFLATE_LENGTHS, s,
               hipLaunchKernelGGL(deflate_lengths_kernel, dim3(1), dim3(DEF_BLOCK), 0, s, freq, n_sym,
                                  max_bits, lengths));
    PANO_LAUNCH_CHECK("deflate_lengths_kernel");
    return PANO_OK;
}

// the chunk kernels' dynamic LDS passes the 64 KiB a kernel gets unasked (per device, idempotent)
int pano_deflate_opt_in(void) {
    PANO_HIP(hipFuncSetAttribute((const void *)deflate_code_kernel,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, DEF_POOL_WORDS * 4));
    PANO_HIP(hipFuncSetAttribute((const void *)deflate_emit_kernel,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, DEF_POOL_WORDS * 4));
    return PANO_OK;
}

// the scratch of pano_deflate: the chunks' records, bit counts, bit offsets, Adler partials
struct DefWork {
    int64_t nchunks, recs, bits, offs, adler, bytes;
};
static DefWork def_work(int64_t n) {
    DefWork w;
    w.nchunks = n > 0 ? ceil_div(n, DEFLATE_CHUNK) : 1;
    w.recs = 0;
    w.bits = (int64_t)sizeof(DefRecord) * w.nchunks;
    w.offs = w.bits + align_up(4 * w.nchunks);
    w.adler = w.offs + align_up(8 * (w.nchunks + 1));
    w.bytes = w.adler + align_up(8 * w.nchunks);
    return w;
}

extern "C" size_t pano_deflate_work_bytes(int64_t n) {
    if (n < 0 || n >= PANO_DEFLATE_MAX_BYTES) return 0;
    return (size_t)def_work(n).bytes;
}

extern "C" int pano_deflate(pano_ctx *ctx, const uint8_t *data, int64_t n, void *work,
                            int64_t work_bytes, const uint8_t **stream_out, int64_t *stream_bytes,
                            uint32_t *adler_out) {
    PANO_ENTER(ctx, "pano_deflate");
    PANO_REQUIRE(work && stream_out && stream_bytes && adler_out && (data || n == 0),
                 "pano_deflate: null pointer");
    *stream_out = nullptr;
    *stream_bytes = 0;
    *adler_out = 1;
    PANO_REQUIRE(n >= 0 && n < PANO_DEFLATE_MAX_BYTES, "pano_deflate: %lld bytes (0 .. 2^34 - 1)",
                 (long long)n);
    const DefWork L = def_work(n);
    PANO_REQUIRE(work_bytes >= L.bytes, "pano_deflate: work of %lld bytes, %lld needed",
                 (long long)work_bytes, (long long)L.bytes);
    const hipStream_t s = (hipStream_t)stream;
    uint8_t *w8 = (uint8_t *)work;
    DefRecord *recs = (DefRecord *)(w8 + L.recs);
    uint32_t *bits = (uint32_t *)(w8 + L.bits), *adler = (uint32_t *)(w8 + L.adler);
    int64_t *offs = (int64_t *)(w8 + L.offs);
    const int64_t nc = L.nchunks;
    const dim3 groups = capped_grid(nc, DEF_MAX_GROUPS);

    // 4. the chunks' codes and bit counts, 5. their scan; wait for the total and the Adler partials
    PANO_TIMED(PK_DEFLATE_CODE, s,
               hipLaunchKernelGGL(deflate_code_kernel, groups, dim3(DEF_BLOCK), DEF_POOL_WORDS * 4, s, data, n, nc,
                                  recs, bits, adler));
    PANO_LAUNCH_CHECK("deflate_code_kernel");
    PANO_TIMED(PK_DEFLATE_SCAN, s,
               hipLaunchKernelGGL((scan_exclusive_kernel<DEF_BLOCK, uint32_t>), dim3(1), dim3(DEF_BLOCK),
                                  0, s, (const uint32_t *)bits, nc, offs));
    PANO_LAUNCH_CHECK("scan_exclusive_kernel");
    int64_t total_bits = 0;
    std::vector<uint32_t> partial(2 * (size_t)nc);
    PANO_HIP(hipMemcpyAsync(&total_bits, offs + nc, 8, hipMemcpyDeviceToHost, s));
    PANO_HIP(hipMemcpyAsync(partial.data(), adler, 8 * (size_t)nc, hipMemcpyDeviceToHost, s));
    PANO_HIP(hipStreamSynchronize(s));
    PANO_REQUIRE(total_bits > 0 && total_bits < ((int64_t)1 << 40), "pano_deflate: %lld bits",
                 (long long)total_bits);
    uint64_t a = 1, b = 0;
    for (int64_t c = 0; c < nc; ++c) {
        const int64_t len = n - c * DEFLATE_CHUNK < DEFLATE_CHUNK ? n - c * DEFLATE_CHUNK : DEFLATE_CHUNK;
        b = (b + (uint64_t)len % DEF_ADLER * a + partial[2 * c + 1]) % DEF_ADLER;
        a = (a + partial[2 * c]) % DEF_ADLER;
    }
    *adler_out = (uint32_t)(b << 16 | a);

    // 6. emission into the zeroed stream, and the download
    const int64_t nbytes = ceil_div(total_bits, 8), raw_bytes = align_up(4 * (ceil_div(total_bits, 32) + 1));
    // (the context's buffers grow with a quarter to spare; the stream is idle, nothing reads them)
    if (int rc = pano_buf_reserve(ctx->buf[BUF_PNG_DEV], raw_bytes, false, raw_bytes / 4)) return rc;
    if (int rc = pano_buf_reserve(ctx->buf[BUF_PNG_HOST], nbytes, true, nbytes / 4)) return rc;
    uint32_t *const dev = (uint32_t *)ctx->buf[BUF_PNG_DEV].p;
    uint8_t *const host = (uint8_t *)ctx->buf[BUF_PNG_HOST].p;
    PANO_HIP(hipMemsetAsync(dev, 0, raw_bytes, s));
    PANO_TIMED(PK_DEFLATE_EMIT, s,
               hipLaunchKernelGGL(deflate_emit_kernel, groups, dim3(DEF_BLOCK), DEF_POOL_WORDS * 4, s, data, n, nc,
                                  (const DefRecord *)recs, (const int64_t *)offs,
                                  dev, raw_bytes / 4));
    PANO_LAUNCH_CHECK("deflate_emit_kernel");
    PANO_HIP(hipMemcpyAsync(host, dev, nbytes, hipMemcpyDeviceToHost, s));
    PANO_HIP(hipStreamSynchronize(s));
    *stream_out = host;
    *stream_bytes = nbytes;
    return PANO_OK;
}
