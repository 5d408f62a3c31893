// Baseline JPEG decode of a batch (pano_jpeg_decode): destuffing, self-synchronising parallel
// Huffman decode, DC prediction, the ISLOW IDCT and the pixel pass.  The contract (the batch
// layout, the stages, what is bit-exact with what) is in include/pano360.h; the host side is
// pano360_amd/jpeg.py and a NumPy restatement of every stage is tests/jpeg_model.py.
//
// Every kernel runs over a flat index across the whole batch (chunks, intervals, subsequence
// slots, blocks, pixels) and finds its image by a binary search of the image rows' first index
// of that kind.  The rows are checked against the buffer sizes on the host before anything is
// queued.
#include "common.h"
#include "wave.h"

#define JF PANO_JPEG_FIELDS
#define JPEG_TAB_BYTES (8 * PANO_JPEG_HUFF_BYTES + 4 * 64 * 2)
#define JPEG_BLOCK 256
#define SCAN_BLOCK 1024
#define JPEG_CHANGED 0x80000000u

__constant__ uint8_t kZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegBatch {
    const uint8_t *packed;          // desc at offset 0
    uint8_t *work;
    uint8_t *out;
    int n;                          // images
};

__device__ __forceinline__ const int64_t *jrow(const JpegBatch &b, int i) {
    return (const int64_t *)b.packed + (size_t)i * JF;
}
__device__ __forceinline__ const int64_t *jbatch(const JpegBatch &b) { return jrow(b, b.n); }

// the last image whose row field f is <= v (the rows ascend in f)
__device__ __forceinline__ int jpeg_find(const JpegBatch &b, int f, int64_t v) {
    int lo = 0, hi = b.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jrow(b, mid)[f] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the last index i of the ascending a[0 .. n) with a[i] <= v
__device__ __forceinline__ int jpeg_find32(const int32_t *__restrict__ a, int n, int64_t v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <typename T>
__device__ __forceinline__ T *jw(const JpegBatch &b, int64_t off) { return (T *)(b.work + off); }

__device__ __forceinline__ bool is_rst(int v) { return v >= 0xD0 && v <= 0xD7; }

// ---- 1. destuffing ---------------------------------------------------------------------------
// One thread per chunk of PANO_JPEG_CHUNK raw bytes.  A byte is dropped when it is the 00 of
// FF 00, an RSTn after FF, or an FF not followed by 00 (a marker's prefix or a fill byte; past
// the segment's end the next byte counts as a marker).  COUNT: bytes kept and markers met per
// chunk.  WRITE (after the scans): the kept bytes, each interval's first byte, the length.
template <bool WRITE>
__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_destuff_kernel(JpegBatch B) {
    const int64_t *bt = jbatch(B);
    const int64_t c = (int64_t)blockIdx.x * JPEG_BLOCK + threadIdx.x;
    if (c >= bt[PANO_JB_CHUNKS]) return;
    const int i = jpeg_find(B, PANO_JD_CHUNK0, c);
    const int64_t *r = jrow(B, i);
    const uint8_t *raw = B.packed + r[PANO_JD_DATA_OFF];
    const int64_t len = r[PANO_JD_DATA_LEN], lc = c - r[PANO_JD_CHUNK0];
    const int64_t a = lc * PANO_JPEG_CHUNK, e = a + PANO_JPEG_CHUNK < len ? a + PANO_JPEG_CHUNK : len;
    int32_t *kept = jw<int32_t>(B, bt[PANO_JB_W_KEPT]), *rst = jw<int32_t>(B, bt[PANO_JB_W_RST]);
    int32_t pos = 0, nrst = 0;
    uint8_t *dst = nullptr;
    int32_t *istart = nullptr;
    const int nint = (int)r[PANO_JD_NINT];
    if (WRITE) {
        const int32_t *kx = jw<int32_t>(B, bt[PANO_JB_W_KEPTX]);
        const int32_t *rx = jw<int32_t>(B, bt[PANO_JB_W_RSTX]);
        const int64_t c0 = r[PANO_JD_CHUNK0];
        pos = kx[c] - kx[c0];
        nrst = rx[c] - rx[c0];
        dst = B.work + r[PANO_JD_DST_OFF];
        istart = jw<int32_t>(B, bt[PANO_JB_W_ISTART]) + r[PANO_JD_INT0];
        if (lc == 0) istart[0] = 0;
    }
    int prev = a > 0 ? raw[a - 1] : 0;
    int cur = a < len ? raw[a] : 0;
    for (int64_t p = a; p < e; ++p) {
        const int next = p + 1 < len ? raw[p + 1] : 0xFF;
        const bool marker = prev == 0xFF && is_rst(cur);
        const bool drop = (prev == 0xFF && cur == 0) || marker || (cur == 0xFF && next != 0);
        if (!drop) {
            if (WRITE) dst[pos] = (uint8_t)cur;
            ++pos;
        }
        if (marker) {
            ++nrst;
            if (WRITE && nrst < nint) istart[nrst] = pos;
        }
        prev = cur;
        cur = next;
    }
    if (!WRITE) {
        kept[c] = pos;
        rst[c] = nrst;
    } else if (e == len) {
        jw<int32_t>(B, bt[PANO_JB_W_DSTLEN])[i] = pos;
    }
}

// ---- exclusive scan of n values in[k * stride] & mask, one workgroup, fixed order -----------
__global__ __launch_bounds__(SCAN_BLOCK) void jpeg_scan_kernel(const int32_t *__restrict__ in,
                                                               int stride, uint32_t mask, int n,
                                                               int32_t *__restrict__ out) {
    __shared__ int32_t waves[SCAN_BLOCK / 64];
    const int t = threadIdx.x;
    const int per = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const int a = min(t * per, n), e = min(a + per, n);
    int32_t sum = 0;
    for (int k = a; k < e; ++k) sum += (int32_t)((uint32_t)in[(size_t)k * stride] & mask);
    int32_t total;
    int32_t run = block_scan_exclusive<SCAN_BLOCK>(sum, waves, total);
    for (int k = a; k < e; ++k) {
        const int32_t v = (int32_t)((uint32_t)in[(size_t)k * stride] & mask);
        out[k] = run;
        run += v;
    }
}

// byte bounds [s, e) of interval g in its image's destuffed bytes (a missing or out-of-order
// marker gives an empty or clipped interval, never bounds outside the data)
__device__ __forceinline__ void jpeg_interval(const JpegBatch &B, const int64_t *bt, int img,
                                              int64_t g, int32_t &s, int32_t &e) {
    const int32_t len = jw<int32_t>(B, bt[PANO_JB_W_DSTLEN])[img];
    const int32_t st = jw<int32_t>(B, bt[PANO_JB_W_ISTART])[g];
    s = st < 0 || st > len ? len : st;
    e = jw<int32_t>(B, bt[PANO_JB_W_IEND])[g];
}

// per interval: its end and its number of subsequences
__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_intervals_kernel(JpegBatch B) {
    const int64_t *bt = jbatch(B);
    const int64_t g = (int64_t)blockIdx.x * JPEG_BLOCK + threadIdx.x;
    if (g >= bt[PANO_JB_INTS]) return;
    const int i = jpeg_find(B, PANO_JD_INT0, g);
    const int64_t *r = jrow(B, i);
    const int32_t len = jw<int32_t>(B, bt[PANO_JB_W_DSTLEN])[i];
    const int32_t *istart = jw<int32_t>(B, bt[PANO_JB_W_ISTART]);
    int32_t s = istart[g];
    s = s < 0 || s > len ? len : s;
    int32_t e = len;
    if (g + 1 - r[PANO_JD_INT0] < r[PANO_JD_NINT]) {
        const int32_t t = istart[g + 1];
        e = t < 0 || t > len ? len : t;
    }
    if (e < s) e = s;
    jw<int32_t>(B, bt[PANO_JB_W_IEND])[g] = e;
    const int64_t bits = 8 * (int64_t)(e - s);
    const int64_t nsub = (bits + PANO_JPEG_SUBSEQ - 1) / PANO_JPEG_SUBSEQ;
    jw<int32_t>(B, bt[PANO_JB_W_INSUB])[g] = nsub > 1 ? (int32_t)nsub : 1;
}

// ---- 2. Huffman --------------------------------------------------------------------------------
// MSB-first bit reader over one interval's bytes [0, end); bytes past the end read as zero.
struct JBits {
    const uint8_t *p;
    int32_t end, byte;
    uint64_t buf;                   // n valid bits, MSB-aligned
    int n;
    __device__ void fill() {
        while (n <= 56) {
            const uint32_t v = byte < end ? p[byte] : 0u;
            buf |= (uint64_t)v << (56 - n);
            n += 8;
            ++byte;
        }
    }
    __device__ void start(const uint8_t *data, int32_t len, int64_t bit) {
        p = data;
        end = len;
        byte = (int32_t)(bit >> 3);
        buf = 0;
        n = 0;
        fill();
        skip((int)(bit & 7));
    }
    __device__ __forceinline__ uint32_t peek(int k) const { return (uint32_t)(buf >> (64 - k)); }
    __device__ __forceinline__ void skip(int k) {
        buf <<= k;
        n -= k;
    }
    __device__ __forceinline__ int64_t pos() const { return 8 * (int64_t)byte - n; }
};

// one symbol of table T (layout: include/pano360.h); an invalid code reads as symbol 0, 1 bit
__device__ __forceinline__ int jpeg_symbol(JBits &br, const uint8_t *__restrict__ T) {
    const uint32_t w = br.peek(16);
    const uint16_t f = ((const uint16_t *)T)[w >> 7];
    if (f) {
        br.skip(f >> 8);
        return f & 255;
    }
    const int32_t *maxcode = (const int32_t *)(T + 1024);
    const int32_t *valoff = (const int32_t *)(T + 1096);
    for (int l = 10; l <= 16; ++l) {
        const int32_t code = (int32_t)(w >> (16 - l));
        if (code <= maxcode[l]) {
            br.skip(l);
            return T[1168 + ((valoff[l] + code) & 255)];
        }
    }
    br.skip(1);
    return 0;
}

__device__ __forceinline__ int jpeg_receive(JBits &br, int s) {
    if (s == 0) return 0;
    const int v = (int)br.peek(s);
    br.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

struct JState {
    int64_t pos;                    // bit within the image's destuffed bytes
    int u, k;                       // block within the MCU, next coefficient (0: the DC)
    int count;                      // blocks completed since the start
};

// Decode from `st` while the position is before `stop` (bits of the image), one symbol and its
// extra bits per step.  WRITE: the coefficients of block blk0 + count (while < nblk) go to coef.
template <bool WRITE>
__device__ void jpeg_run(const JpegBatch &B, const int64_t *r, int32_t s, int32_t e,
                         int64_t stop, JState &st, int16_t *__restrict__ coef, int64_t blk0,
                         int64_t nblk) {
    const uint8_t *tabs = B.packed + r[PANO_JD_TAB_OFF];
    const int bpm = (int)r[PANO_JD_BPM];
    const uint32_t comp_u = (uint32_t)r[PANO_JD_COMP_U], tabsel = (uint32_t)r[PANO_JD_TABSEL];
    JBits br;
    const int64_t base = 8 * (int64_t)s;
    br.start(B.work + r[PANO_JD_DST_OFF] + s, e - s, st.pos - base);
    int u = st.u, k = st.k, count = st.count;
    while (br.pos() + base < stop) {
        br.fill();
        const int c = (comp_u >> (2 * u)) & 3;
        const uint32_t sel = tabsel >> (8 * c);
        int16_t *blk = nullptr;
        if (WRITE && blk0 + count < nblk) blk = coef + 64 * (blk0 + count);
        if (k == 0) {
            const int sym = jpeg_symbol(br, tabs + (sel & 3) * PANO_JPEG_HUFF_BYTES);
            const int v = jpeg_receive(br, sym & 15);
            if (WRITE && blk) blk[0] = (int16_t)v;
            k = 1;
        } else {
            const int rs = jpeg_symbol(br, tabs + (4 + ((sel >> 2) & 3)) * PANO_JPEG_HUFF_BYTES);
            const int rr = rs >> 4, ss = rs & 15;
            if (ss) {
                k += rr;
                const int v = jpeg_receive(br, ss);
                if (WRITE && blk && k < 64) blk[kZigzag[k]] = (int16_t)v;
                ++k;
            } else if (rr == 15) {
                k += 16;
            } else {
                k = 64;
            }
        }
        if (k >= 64) {
            k = 0;
            u = u + 1 == bpm ? 0 : u + 1;
            ++count;
        }
    }
    st.pos = br.pos() + base;
    st.u = u;
    st.k = k;
    st.count = count;
}

// subsequence slot t -> (image, interval g, index j in the interval); false: an unused slot
__device__ __forceinline__ bool jpeg_slot(const JpegBatch &B, const int64_t *bt, int64_t t,
                                          int &img, int &g, int &j) {
    const int nint = (int)bt[PANO_JB_INTS];
    const int32_t *isubx = jw<int32_t>(B, bt[PANO_JB_W_ISUBX]);
    g = jpeg_find32(isubx, nint, t);
    j = (int)(t - isubx[g]);
    if (j >= jw<int32_t>(B, bt[PANO_JB_W_INSUB])[g]) return false;
    img = jpeg_find(B, PANO_JD_INT0, g);
    return true;
}

// Round 0: every subsequence from its first bit (the first of an interval in the true state,
// the others guessing block 0, coefficient 0).  Round >= 1: a subsequence whose predecessor's
// exit changed in the previous round decodes again from that exit; *flag = 1 when an exit
// differs from the one it had.  States are int4 (pos, u, k, count | JPEG_CHANGED).
__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_huff_sync_kernel(JpegBatch B, int round,
                                                                    const int4 *__restrict__ prev,
                                                                    int4 *__restrict__ next,
                                                                    int32_t *__restrict__ flag) {
    const int64_t *bt = jbatch(B);
    const int64_t t = (int64_t)blockIdx.x * JPEG_BLOCK + threadIdx.x;
    if (t >= bt[PANO_JB_SUBS]) return;
    int img, g, j;
    if (!jpeg_slot(B, bt, t, img, g, j)) {
        next[t] = make_int4(0, 0, 0, 0);
        return;
    }
    const int64_t *r = jrow(B, img);
    int32_t s, e;
    jpeg_interval(B, bt, img, g, s, e);
    const int64_t first = 8 * (int64_t)s, last = 8 * (int64_t)e;
    const int64_t end = first + (int64_t)(j + 1) * PANO_JPEG_SUBSEQ;
    const int64_t stop = end < last ? end : last;
    JState st;
    if (round == 0) {
        st.pos = first + (int64_t)j * PANO_JPEG_SUBSEQ;
        st.u = st.k = st.count = 0;
    } else {
        const int4 mine = prev[t];
        const int4 in = j > 0 ? prev[t - 1] : make_int4(0, 0, 0, 0);
        if (j == 0 || !((uint32_t)in.w & JPEG_CHANGED)) {
            next[t] = make_int4(mine.x, mine.y, mine.z, (int)((uint32_t)mine.w & ~JPEG_CHANGED));
            return;
        }
        st.pos = (int64_t)(uint32_t)in.x;
        st.u = in.y;
        st.k = in.z;
        st.count = 0;
        jpeg_run<false>(B, r, s, e, stop, st, nullptr, 0, 0);
        const bool changed = (int32_t)st.pos != mine.x || st.u != mine.y || st.k != mine.z;
        if (changed) *flag = 1;
        next[t] = make_int4((int32_t)st.pos, st.u, st.k,
                            (int)((uint32_t)st.count | (changed ? JPEG_CHANGED : 0u)));
        return;
    }
    jpeg_run<false>(B, r, s, e, stop, st, nullptr, 0, 0);
    next[t] = make_int4((int32_t)st.pos, st.u, st.k, (int)((uint32_t)st.count | JPEG_CHANGED));
}

// the coefficients: each subsequence from its synchronised entry, its blocks placed by the scan
// of the completed-block counts (cntx) within the interval
__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_huff_write_kernel(JpegBatch B,
                                                                     const int4 *__restrict__ fin) {
    const int64_t *bt = jbatch(B);
    const int64_t t = (int64_t)blockIdx.x * JPEG_BLOCK + threadIdx.x;
    if (t >= bt[PANO_JB_SUBS]) return;
    int img, g, j;
    if (!jpeg_slot(B, bt, t, img, g, j)) return;
    const int64_t *r = jrow(B, img);
    int32_t s, e;
    jpeg_interval(B, bt, img, g, s, e);
    const int64_t first = 8 * (int64_t)s, last = 8 * (int64_t)e;
    const int64_t end = first + (int64_t)(j + 1) * PANO_JPEG_SUBSEQ;
    const int64_t stop = end < last ? end : last;
    JState st;
    if (j == 0) {
        st.pos = first;
        st.u = st.k = 0;
    } else {
        const int4 in = fin[t - 1];
        st.pos = (int64_t)(uint32_t)in.x;
        st.u = in.y;
        st.k = in.z;
    }
    st.count = 0;
    const int32_t *cntx = jw<int32_t>(B, bt[PANO_JB_W_CNTX]);
    const int64_t ri = r[PANO_JD_RI], nmcu = r[PANO_JD_MCUX] * r[PANO_JD_MCUY];
    const int64_t gl = g - r[PANO_JD_INT0];
    const int64_t m0 = ri ? gl * ri : 0;
    const int64_t m1 = ri ? (m0 + ri < nmcu ? m0 + ri : nmcu) : nmcu;
    const int64_t bpm = r[PANO_JD_BPM];
    int16_t *coef = jw<int16_t>(B, bt[PANO_JB_W_COEF]) + 64 * (r[PANO_JD_BLK0] + m0 * bpm);
    const int64_t blk0 = cntx[t] - cntx[t - j];
    jpeg_run<true>(B, r, s, e, stop, st, coef, blk0, (m1 - m0) * bpm);
}

// ---- 3. DC prediction: one workgroup per (interval, component), MCUs in tiles -----------------
__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_dc_kernel(JpegBatch B) {
    __shared__ int32_t part[JPEG_BLOCK];
    __shared__ int32_t carry;
    const int64_t *bt = jbatch(B);
    const int64_t g = blockIdx.x;
    const int c = blockIdx.y, tid = threadIdx.x;
    const int img = jpeg_find(B, PANO_JD_INT0, g);
    const int64_t *r = jrow(B, img);
    if (c >= r[PANO_JD_NC]) return;
    const int bpm = (int)r[PANO_JD_BPM];
    const uint32_t comp_u = (uint32_t)r[PANO_JD_COMP_U];
    int u0 = -1, nb = 0;
    for (int u = 0; u < bpm; ++u)
        if ((int)((comp_u >> (2 * u)) & 3) == c) {
            if (u0 < 0) u0 = u;
            ++nb;
        }
    if (u0 < 0) return;
    const int64_t ri = r[PANO_JD_RI], nmcu = r[PANO_JD_MCUX] * r[PANO_JD_MCUY];
    const int64_t gl = g - r[PANO_JD_INT0];
    const int64_t m0 = ri ? gl * ri : 0;
    const int64_t m1 = ri ? (m0 + ri < nmcu ? m0 + ri : nmcu) : nmcu;
    int16_t *coef = jw<int16_t>(B, bt[PANO_JB_W_COEF]) + 64 * r[PANO_JD_BLK0];
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = m0; base < m1; base += JPEG_BLOCK) {
        const int64_t m = base + tid;
        int32_t sum = 0;
        if (m < m1)
            for (int q = 0; q < nb; ++q) sum += coef[64 * (m * bpm + u0 + q)];
        part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < JPEG_BLOCK; off <<= 1) {
            const int32_t v = tid >= off ? part[tid - off] : 0;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        int32_t run = carry + part[tid] - sum;
        if (m < m1)
            for (int q = 0; q < nb; ++q) {
                int16_t *d = coef + 64 * (m * bpm + u0 + q);
                run += *d;
                *d = (int16_t)run;
            }
        __syncthreads();
        if (tid == JPEG_BLOCK - 1) carry += part[tid];
        __syncthreads();
    }
}

// ---- 4. dequantise + ISLOW IDCT, 8 lanes per block ------------------------------------------
#define FIX_0_298631336 2446
#define FIX_0_390180644 3196
#define FIX_0_541196100 4433
#define FIX_0_765366865 6270
#define FIX_0_899976223 7373
#define FIX_1_175875602 9633
#define FIX_1_501321110 12299
#define FIX_1_847759065 15137
#define FIX_1_961570560 16069
#define FIX_2_053119869 16819
#define FIX_2_562915447 20995
#define FIX_3_072711026 25172

// one 8-point pass (T.81 A.3.3 in the ISLOW factorisation), results descaled by `shift`
__device__ __forceinline__ void jpeg_idct8(const int32_t (&x)[8], int shift, int32_t (&o)[8]) {
    int32_t z2 = x[2], z3 = x[6];
    int32_t z1 = (z2 + z3) * FIX_0_541196100;
    const int32_t tmp2 = z1 + z3 * -FIX_1_847759065;
    const int32_t tmp3 = z1 + z2 * FIX_0_765366865;
    const int32_t tmp0 = (x[0] + x[4]) * (1 << 13), tmp1 = (x[0] - x[4]) * (1 << 13);
    const int32_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    int32_t a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    z2 = a1 + a2;
    z3 = a0 + a2;
    int32_t z4 = a1 + a3;
    const int32_t z5 = (z3 + z4) * FIX_1_175875602;
    a0 *= FIX_0_298631336;
    a1 *= FIX_2_053119869;
    a2 *= FIX_3_072711026;
    a3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223;
    z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5;
    z4 = z4 * -FIX_0_390180644 + z5;
    a0 += z1 + z3;
    a1 += z2 + z4;
    a2 += z2 + z3;
    a3 += z1 + z4;
    const int32_t rnd = 1 << (shift - 1);
    o[0] = (t10 + a3 + rnd) >> shift;
    o[7] = (t10 - a3 + rnd) >> shift;
    o[1] = (t11 + a2 + rnd) >> shift;
    o[6] = (t11 - a2 + rnd) >> shift;
    o[2] = (t12 + a1 + rnd) >> shift;
    o[5] = (t12 - a1 + rnd) >> shift;
    o[3] = (t13 + a0 + rnd) >> shift;
    o[4] = (t13 - a0 + rnd) >> shift;
}

// libjpeg's post-IDCT range-limit table: entry (v & 1023), i.e. clamp(wrap10(v) + 128, 0, 255)
__device__ __forceinline__ uint8_t jpeg_limit(int32_t v) {
    int32_t w = v & 1023;
    if (w >= 512) w -= 1024;
    w += 128;
    return (uint8_t)(w < 0 ? 0 : (w > 255 ? 255 : w));
}

__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_idct_kernel(JpegBatch B) {
    __shared__ int32_t ws[JPEG_BLOCK / 8][8][9];
    const int64_t *bt = jbatch(B);
    const int64_t gid = (int64_t)blockIdx.x * JPEG_BLOCK + threadIdx.x;
    const int64_t b = gid >> 3;
    const int lane = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const bool live = b < bt[PANO_JB_BLOCKS];
    int img = 0, c = 0;
    int64_t bx = 0, by = 0;
    const int64_t *r = jrow(B, 0);
    if (live) {
        img = jpeg_find(B, PANO_JD_BLK0, b);
        r = jrow(B, img);
        const int64_t lb = b - r[PANO_JD_BLK0], bpm = r[PANO_JD_BPM], mx = r[PANO_JD_MCUX];
        const int64_t m = lb / bpm;
        const int u = (int)(lb - m * bpm);
        const uint32_t comp_u = (uint32_t)r[PANO_JD_COMP_U];
        c = (comp_u >> (2 * u)) & 3;
        int u0 = 0;
        while ((int)((comp_u >> (2 * u0)) & 3) != c) ++u0;
        const uint32_t samp = (uint32_t)(r[PANO_JD_SAMP] >> (8 * c));
        const int hc = samp & 15, vc = (samp >> 4) & 15, w = u - u0;
        bx = (m % mx) * hc + w % hc;
        by = (m / mx) * vc + w / hc;
        const int tq = (int)((r[PANO_JD_TABSEL] >> (8 * c + 4)) & 3);
        const uint16_t *q = (const uint16_t *)(B.packed + r[PANO_JD_TAB_OFF] +
                                               8 * PANO_JPEG_HUFF_BYTES) + 64 * tq;
        const int16_t *blk = jw<int16_t>(B, bt[PANO_JB_W_COEF]) + 64 * b;
        int32_t x[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = (int32_t)blk[8 * k + lane] * (int32_t)q[8 * k + lane];
        jpeg_idct8(x, 11, o);                             // column `lane`
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[slot][k][lane] = o[k];
    }
    __syncthreads();
    if (!live) return;
    int32_t x[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = ws[slot][lane][k];
    jpeg_idct8(x, 18, o);                                 // row `lane`
    uint8_t *dst = B.work + r[PANO_JD_PLANE0 + c] + (8 * by + lane) * r[PANO_JD_PITCH0 + c] + 8 * bx;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo |= (uint32_t)jpeg_limit(o[k]) << (8 * k);
        hi |= (uint32_t)jpeg_limit(o[4 + k]) << (8 * k);
    }
    *(uint2 *)dst = make_uint2(lo, hi);
}

// ---- 5. pixels ----------------------------------------------------------------------------------
__device__ __forceinline__ int jclamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the upsampled chroma sample at (x, y) of plane p (cw x ch real samples, pitch), factors
// (fh, fv) in {1, 2}: libjpeg's fancy upsampling with its narrow-plane case
__device__ __forceinline__ int jpeg_chroma(const uint8_t *__restrict__ p, int64_t pitch, int cw,
                                           int ch, int fh, int fv, int x, int y) {
    if (fh == 1 && fv == 1) return p[y * pitch + x];
    if (cw <= 2) return p[jclamp(y / fv, ch) * pitch + jclamp(x / fh, cw)];
    const int cx = x >> 1, odd = x & 1, ox = jclamp(odd ? cx + 1 : cx - 1, cw);
    if (fv == 1) {
        const uint8_t *row = p + y * pitch;
        return (3 * row[cx] + row[ox] + (odd ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1, oy = jclamp((y & 1) ? cy + 1 : cy - 1, ch);
    const uint8_t *r0 = p + cy * pitch, *r1 = p + oy * pitch;
    const int here = 3 * r0[cx] + r1[cx], there = 3 * r0[ox] + r1[ox];
    return (3 * here + there + (odd ? 7 : 8)) >> 4;
}

__device__ __forceinline__ uint8_t jsat(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

__global__ __launch_bounds__(JPEG_BLOCK) void jpeg_pixels_kernel(JpegBatch B) {
    const int64_t *bt = jbatch(B);
    const int64_t p = (int64_t)blockIdx.x * JPEG_BLOCK + threadIdx.x;
    if (p >= bt[PANO_JB_PIXELS]) return;
    const int img = jpeg_find(B, PANO_JD_PIX0, p);
    const int64_t *r = jrow(B, img);
    const int W = (int)r[PANO_JD_W], H = (int)r[PANO_JD_H], o = (int)r[PANO_JD_ORIENT];
    const int OW = o >= 5 ? H : W;
    const int64_t lp = p - r[PANO_JD_PIX0];
    const int ox = (int)(lp % OW), oy = (int)(lp / OW);
    int x = ox, y = oy;                                   // ImageOps.exif_transpose
    switch (o) {
    case 2: x = W - 1 - ox; break;
    case 3: x = W - 1 - ox; y = H - 1 - oy; break;
    case 4: y = H - 1 - oy; break;
    case 5: x = oy; y = ox; break;
    case 6: x = oy; y = H - 1 - ox; break;
    case 7: x = W - 1 - oy; y = H - 1 - ox; break;
    case 8: x = W - 1 - oy; y = ox; break;
    default: break;
    }
    const int Y = B.work[r[PANO_JD_PLANE0] + y * r[PANO_JD_PITCH0] + x];
    uint8_t bgr[3] = {(uint8_t)Y, (uint8_t)Y, (uint8_t)Y};
    if (r[PANO_JD_NC] == 3) {
        const int hm = (int)r[PANO_JD_HMAX], vm = (int)r[PANO_JD_VMAX];
        int cc[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint32_t samp = (uint32_t)(r[PANO_JD_SAMP] >> (8 * (k + 1)));
            const int hc = samp & 15, vc = (samp >> 4) & 15;
            const int cw = (W * hc + hm - 1) / hm, ch = (H * vc + vm - 1) / vm;
            cc[k] = jpeg_chroma(B.work + r[PANO_JD_PLANE1 + k], r[PANO_JD_PITCH1 + k], cw, ch,
                                hm / hc, vm / vc, x, y);
        }
        const int cb = cc[0] - 128, cr = cc[1] - 128, half = 1 << 15;
        bgr[0] = jsat(Y + ((116130 * cb + half) >> 16));
        bgr[1] = jsat(Y + ((-22554 * cb + half - 46802 * cr) >> 16));
        bgr[2] = jsat(Y + ((91881 * cr + half) >> 16));
    }
    uint8_t *d = B.out + r[PANO_JD_OUT_OFF] + 3 * lp;
    d[0] = bgr[0];
    d[1] = bgr[1];
    d[2] = bgr[2];
}

// ---- the entry point -------------------------------------------------------------------------------

// the rows against the buffers: every offset and size the kernels use, before anything is queued
static int jpeg_check(const int64_t *desc, int n, int64_t packed_bytes, int64_t work_bytes,
                      int64_t out_bytes) {
    const int64_t *bt = desc + (int64_t)n * JF;
    PANO_REQUIRE(bt[PANO_JB_N] == n, "pano_jpeg_decode: batch row says %lld images, not %d",
                 (long long)bt[PANO_JB_N], n);
    PANO_REQUIRE(bt[PANO_JB_PACKED_BYTES] <= packed_bytes && packed_bytes < ((int64_t)1 << 31) &&
                     (int64_t)(n + 1) * JF * 8 <= packed_bytes,
                 "pano_jpeg_decode: packed buffer of %lld bytes", (long long)packed_bytes);
    PANO_REQUIRE(bt[PANO_JB_WORK_BYTES] <= work_bytes && bt[PANO_JB_OUT_BYTES] <= out_bytes,
                 "pano_jpeg_decode: work or out buffer too small");
    int64_t chunks = 0, ints = 0, subs = 0, blocks = 0, pixels = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t *r = desc + (int64_t)i * JF;
        const int64_t w = r[PANO_JD_W], h = r[PANO_JD_H], nc = r[PANO_JD_NC], len = r[PANO_JD_DATA_LEN];
        PANO_REQUIRE(w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && (nc == 1 || nc == 3) &&
                         r[PANO_JD_ORIENT] >= 1 && r[PANO_JD_ORIENT] <= 8,
                     "pano_jpeg_decode: image %d: %lld x %lld, %lld components", i, (long long)w,
                     (long long)h, (long long)nc);
        const int64_t hm = r[PANO_JD_HMAX], vm = r[PANO_JD_VMAX];
        PANO_REQUIRE(hm >= 1 && hm <= 2 && vm >= 1 && vm <= 2 &&
                         r[PANO_JD_MCUX] == ceil_div(w, 8 * hm) && r[PANO_JD_MCUY] == ceil_div(h, 8 * vm),
                     "pano_jpeg_decode: image %d: MCU grid", i);
        const int64_t nmcu = r[PANO_JD_MCUX] * r[PANO_JD_MCUY], ri = r[PANO_JD_RI];
        PANO_REQUIRE(ri >= 0 && r[PANO_JD_NINT] == (ri ? ceil_div(nmcu, ri) : 1),
                     "pano_jpeg_decode: image %d: restart intervals", i);
        const int64_t bpm = r[PANO_JD_BPM];
        PANO_REQUIRE(bpm >= 1 && bpm <= 16, "pano_jpeg_decode: image %d: %lld blocks per MCU", i,
                     (long long)bpm);
        int per[3] = {0, 0, 0};
        for (int u = 0; u < bpm; ++u) {
            const int c = (int)((r[PANO_JD_COMP_U] >> (2 * u)) & 3);
            PANO_REQUIRE(c < nc, "pano_jpeg_decode: image %d: block component", i);
            ++per[c];
        }
        for (int c = 0; c < nc; ++c) {
            const int hc = (int)((r[PANO_JD_SAMP] >> (8 * c)) & 15);
            const int vc = (int)((r[PANO_JD_SAMP] >> (8 * c + 4)) & 15);
            PANO_REQUIRE(hc >= 1 && vc >= 1 && hm % hc == 0 && vm % vc == 0 && per[c] == hc * vc &&
                             (nc == 3 || (hc == 1 && vc == 1)),
                         "pano_jpeg_decode: image %d: sampling of component %d", i, c);
            const int64_t pitch = r[PANO_JD_PITCH0 + c];
            PANO_REQUIRE(pitch == 8 * r[PANO_JD_MCUX] * hc && r[PANO_JD_PLANE0 + c] >= 0 &&
                             r[PANO_JD_PLANE0 + c] + pitch * 8 * r[PANO_JD_MCUY] * vc <= work_bytes,
                         "pano_jpeg_decode: image %d: plane %d", i, c);
        }
        PANO_REQUIRE(len >= 0 && len < ((int64_t)1 << 28) && r[PANO_JD_DATA_OFF] >= 0 &&
                         r[PANO_JD_DATA_OFF] + len <= packed_bytes && r[PANO_JD_TAB_OFF] >= 0 &&
                         r[PANO_JD_TAB_OFF] + JPEG_TAB_BYTES <= packed_bytes &&
                         r[PANO_JD_DST_OFF] >= 0 && r[PANO_JD_DST_OFF] + len <= work_bytes &&
                         r[PANO_JD_OUT_OFF] >= 0 && r[PANO_JD_OUT_OFF] + 3 * w * h <= out_bytes,
                     "pano_jpeg_decode: image %d: offsets", i);
        PANO_REQUIRE(r[PANO_JD_CHUNK0] == chunks && r[PANO_JD_INT0] == ints &&
                         r[PANO_JD_SUB0] == subs && r[PANO_JD_BLK0] == blocks &&
                         r[PANO_JD_PIX0] == pixels,
                     "pano_jpeg_decode: image %d: first indices", i);
        chunks += len > 0 ? ceil_div(len, PANO_JPEG_CHUNK) : 1;
        ints += r[PANO_JD_NINT];
        subs += len * 8 / PANO_JPEG_SUBSEQ + r[PANO_JD_NINT] + 1;
        blocks += nmcu * bpm;
        pixels += w * h;
    }
    PANO_REQUIRE(bt[PANO_JB_CHUNKS] == chunks && bt[PANO_JB_INTS] == ints &&
                     bt[PANO_JB_SUBS] == subs && bt[PANO_JB_BLOCKS] == blocks &&
                     bt[PANO_JB_PIXELS] == pixels && subs < ((int64_t)1 << 30) &&
                     blocks < ((int64_t)1 << 30) && pixels < ((int64_t)1 << 34),
                 "pano_jpeg_decode: batch totals");
    const int64_t arrays[][2] = {
        {PANO_JB_W_KEPT, 4 * chunks},  {PANO_JB_W_RST, 4 * chunks},   {PANO_JB_W_KEPTX, 4 * chunks},
        {PANO_JB_W_RSTX, 4 * chunks},  {PANO_JB_W_DSTLEN, 4 * (int64_t)n},
        {PANO_JB_W_ISTART, 4 * ints},  {PANO_JB_W_IEND, 4 * ints},    {PANO_JB_W_INSUB, 4 * ints},
        {PANO_JB_W_ISUBX, 4 * ints},   {PANO_JB_W_STATE0, 16 * subs}, {PANO_JB_W_STATE1, 16 * subs},
        {PANO_JB_W_CNTX, 4 * subs},    {PANO_JB_W_FLAG, 4},           {PANO_JB_W_COEF, 128 * blocks}};
    for (const auto &a : arrays)
        PANO_REQUIRE(bt[a[0]] >= 0 && bt[a[0]] % 16 == 0 && bt[a[0]] + a[1] <= work_bytes,
                     "pano_jpeg_decode: work array %lld", (long long)a[0]);
    return PANO_OK;
}

static int jpeg_scan(pano_ctx *ctx, hipStream_t s, const int32_t *in, int stride, uint32_t mask,
                     int64_t n, int32_t *out) {
    PANO_TIMED(PK_JPEG_SCAN, s,
               hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(SCAN_BLOCK), 0, s, in, stride,
                                  mask, (int)n, out));
    PANO_LAUNCH_CHECK("jpeg_scan_kernel");
    return PANO_OK;
}

static inline dim3 jgrid(int64_t threads) { return dim3((unsigned)ceil_div(threads, JPEG_BLOCK)); }

extern "C" int pano_jpeg_decode(pano_ctx *ctx, const int64_t *desc, int n, const uint8_t *packed,
                                int64_t packed_bytes, void *work, int64_t work_bytes,
                                uint8_t *out, int64_t out_bytes) {
    PANO_ENTER(ctx, "pano_jpeg_decode");
    PANO_REQUIRE(n >= 1 && n <= (1 << 20), "pano_jpeg_decode: %d images", n);
    PANO_REQUIRE(desc && packed && work && out, "pano_jpeg_decode: null pointer");
    if (int rc = jpeg_check(desc, n, packed_bytes, work_bytes, out_bytes)) return rc;
    const int64_t *bt = desc + (int64_t)n * JF;
    const hipStream_t s = (hipStream_t)stream;
    uint8_t *w8 = (uint8_t *)work;
    JpegBatch B{packed, w8, out, n};
    const int64_t chunks = bt[PANO_JB_CHUNKS], ints = bt[PANO_JB_INTS], subs = bt[PANO_JB_SUBS];
    auto at = [&](int f) { return (int32_t *)(w8 + bt[f]); };

    // 1. destuffing
    PANO_HIP(hipMemsetAsync(at(PANO_JB_W_ISTART), 0xFF, 4 * ints, s));
    PANO_TIMED(PK_JPEG_DESTUFF, s,
               hipLaunchKernelGGL(jpeg_destuff_kernel<false>, jgrid(chunks), dim3(JPEG_BLOCK), 0,
                                  s, B));
    PANO_LAUNCH_CHECK("jpeg_destuff_kernel");
    if (int rc = jpeg_scan(ctx, s, at(PANO_JB_W_KEPT), 1, ~0u, chunks, at(PANO_JB_W_KEPTX))) return rc;
    if (int rc = jpeg_scan(ctx, s, at(PANO_JB_W_RST), 1, ~0u, chunks, at(PANO_JB_W_RSTX))) return rc;
    PANO_TIMED(PK_JPEG_DESTUFF, s,
               hipLaunchKernelGGL(jpeg_destuff_kernel<true>, jgrid(chunks), dim3(JPEG_BLOCK), 0,
                                  s, B));
    PANO_LAUNCH_CHECK("jpeg_destuff_kernel");
    PANO_TIMED(PK_JPEG_INTERVALS, s,
               hipLaunchKernelGGL(jpeg_intervals_kernel, jgrid(ints), dim3(JPEG_BLOCK), 0, s, B));
    PANO_LAUNCH_CHECK("jpeg_intervals_kernel");
    if (int rc = jpeg_scan(ctx, s, at(PANO_JB_W_INSUB), 1, ~0u, ints, at(PANO_JB_W_ISUBX))) return rc;

    // 2. Huffman: round 0, then rounds until no exit changes
    int4 *st[2] = {(int4 *)(w8 + bt[PANO_JB_W_STATE0]), (int4 *)(w8 + bt[PANO_JB_W_STATE1])};
    int32_t *flag = at(PANO_JB_W_FLAG);
    PANO_TIMED(PK_JPEG_HUFF_SYNC, s,
               hipLaunchKernelGGL(jpeg_huff_sync_kernel, jgrid(subs), dim3(JPEG_BLOCK), 0, s, B,
                                  0, (const int4 *)st[1], st[0], flag));
    PANO_LAUNCH_CHECK("jpeg_huff_sync_kernel");
    int cur = 0;
    int64_t max_rounds = 1;
    for (int i = 0; i < n; ++i) {
        const int64_t *r = desc + (int64_t)i * JF;
        const int64_t bound = r[PANO_JD_DATA_LEN] * 8 / PANO_JPEG_SUBSEQ + 2;
        if (bound > max_rounds) max_rounds = bound;
    }
    for (int64_t round = 1; round <= max_rounds; ++round) {
        int32_t host_flag = 0;
        PANO_HIP(hipMemsetAsync(flag, 0, 4, s));
        PANO_TIMED(PK_JPEG_HUFF_SYNC, s,
                   hipLaunchKernelGGL(jpeg_huff_sync_kernel, jgrid(subs), dim3(JPEG_BLOCK), 0, s,
                                      B, (int)round, (const int4 *)st[cur], st[cur ^ 1], flag));
        PANO_LAUNCH_CHECK("jpeg_huff_sync_kernel");
        cur ^= 1;
        PANO_HIP(hipMemcpyAsync(&host_flag, flag, 4, hipMemcpyDeviceToHost, s));
        PANO_HIP(hipStreamSynchronize(s));
        if (!host_flag) break;
    }
    int32_t *cntx = at(PANO_JB_W_CNTX);
    if (int rc = jpeg_scan(ctx, s, (const int32_t *)st[cur] + 3, 4, ~JPEG_CHANGED, subs, cntx))
        return rc;
    PANO_HIP(hipMemsetAsync(w8 + bt[PANO_JB_W_COEF], 0, 128 * bt[PANO_JB_BLOCKS], s));
    PANO_TIMED(PK_JPEG_HUFF_WRITE, s,
               hipLaunchKernelGGL(jpeg_huff_write_kernel, jgrid(subs), dim3(JPEG_BLOCK), 0, s, B,
                                  (const int4 *)st[cur]));
    PANO_LAUNCH_CHECK("jpeg_huff_write_kernel");

    // 3. DC prediction, 4. IDCT, 5. pixels
    PANO_TIMED(PK_JPEG_DC, s,
               hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)ints, 3), dim3(JPEG_BLOCK), 0, s,
                                  B));
    PANO_LAUNCH_CHECK("jpeg_dc_kernel");
    PANO_TIMED(PK_JPEG_IDCT, s,
               hipLaunchKernelGGL(jpeg_idct_kernel, jgrid(8 * bt[PANO_JB_BLOCKS]),
                                  dim3(JPEG_BLOCK), 0, s, B));
    PANO_LAUNCH_CHECK("jpeg_idct_kernel");
    PANO_TIMED(PK_JPEG_PIXELS, s,
               hipLaunchKernelGGL(jpeg_pixels_kernel, jgrid(bt[PANO_JB_PIXELS]), dim3(JPEG_BLOCK),
                                  0, s, B));
    PANO_LAUNCH_CHECK("jpeg_pixels_kernel");
    return PANO_OK;
}
