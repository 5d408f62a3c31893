// Baseline JPEG encode of one image (pano_jpeg_encode) or of a batch of images of any sizes
// (pano_jpeg_encode_batch): colour conversion, downsampling, the ISLOW FDCT and quantisation per
// block, per-block Huffman bit counts, an int64 scan of them, the bit emission and the byte
// stuffing.  The batch runs the same stages over all images' blocks at once: every stage is one
// kernel template and one driver (enc_run) runs both calls; what differs is in the two policies
// at "which image" below.  The contract (what is bit-exact with what, the scratch layout, the waits) is
// in include/pano360.h; the host side (quantisation tables, the header) is
// pano360_amd/jpeg.py and a NumPy restatement of every stage is tests/jpeg_encode_model.py.
//
// Blocks are numbered in scan order: MCU by MCU, and inside an MCU the luma blocks row by row,
// then Cb, then Cr.  The coefficients are kept as int16 [64] per block in zigzag order.
#include "common.h"
#include "wave.h"

#define ENC_BLOCK 256
#define ENC_TILE 32                 // blocks per workgroup of the block kernel (8 threads each)
#define ENC_WAVES (ENC_BLOCK / 64)  // blocks per workgroup of the count and emit kernels
#define ENC_WORDS 64                // LDS words per block of the emit kernel (>= 1691 bits + 31)
#define ENC_SCAN 1024               // threads of a scan workgroup
#define ENC_SCAN_ITEMS 4            // values per scan thread
#define ENC_SCAN_TILE (ENC_SCAN * ENC_SCAN_ITEMS)
#define ENC_CHUNK 64                // stream bytes per stuffing thread
#define ENC_MAX_GROUPS (1 << 20)    // grid cap of the block-wise kernels (they loop beyond it)

// ---- the Annex K Huffman tables, as (length << 16) | code per symbol -----------------------------
struct EncHuff {
    uint32_t e[4][256];             // DC luma, AC luma, DC chroma, AC chroma
};
constexpr uint8_t kEncBits[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                     {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
                                     {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                     {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kEncValsDC[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kEncValsACL[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61,
    0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52,
    0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25,
    0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64,
    0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3,
    0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8,
    0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
constexpr uint8_t kEncValsACC[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61,
    0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33,
    0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18,
    0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63,
    0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA,
    0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7,
    0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// canonical code assignment (T.81 C.1, C.2)
constexpr EncHuff enc_huff_tables() {
    EncHuff t{};
    for (int tab = 0; tab < 4; ++tab) {
        const uint8_t *vals = tab == 0 || tab == 2 ? kEncValsDC : tab == 1 ? kEncValsACL : kEncValsACC;
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kEncBits[tab][len - 1]; ++i) t.e[tab][vals[k++]] = (uint32_t)len << 16 | code++;
            code <<= 1;
        }
    }
    return t;
}
__constant__ EncHuff kEncHuff = enc_huff_tables();

__constant__ uint8_t kEncZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- the image and its block grid ----------------------------------------------------------------
struct EncGeom {
    const uint8_t *img;             // pixel (x, y) at img[y * pitch + 3 x], RGB or BGR
    int64_t pitch;
    int w, h, bgr;
    int hm, vm;                     // luma sampling (the chroma is 1x1)
    int mx, my, bpm;                // MCUs across / down, blocks per MCU
    int wib[2], hib[2];             // blocks across / down of the luma and of a chroma component
    int nblocks;
};
struct EncImage : EncGeom {
    uint8_t q[2][64];               // quantisers, natural order
};

// Where block b of the scan lies: component, and the block whose samples it codes (a dummy block
// of jccoefct.c codes no samples: its AC is zero and its DC that of the block before it, which
// is the nearest real block to the left, or for a bottom dummy the last block of the MCU row
// above it).  *dummy tells which.
struct EncPlace {
    int comp, bx, by;
    bool dummy;
};
__device__ __forceinline__ EncPlace enc_place(const EncGeom &E, int b) {
    const int mcu = b / E.bpm, k = b - mcu * E.bpm, ny = E.hm * E.vm;
    const int ux = mcu % E.mx, uy = mcu / E.mx;
    EncPlace p;
    if (k < ny) {
        p.comp = 0;
        p.bx = ux * E.hm + k % E.hm;
        p.by = uy * E.vm + k / E.hm;
    } else {
        p.comp = k - ny + 1;
        p.bx = ux;
        p.by = uy;
    }
    const int ci = p.comp ? 1 : 0, wib = E.wib[ci], hib = E.hib[ci];
    p.dummy = p.bx >= wib || p.by >= hib;
    if (p.by >= hib) {
        p.bx = min(ux * E.hm + E.hm - 1, wib - 1);
        p.by = hib - 1;
    } else if (p.bx >= wib) {
        p.bx = wib - 1;
    }
    return p;
}

__device__ __forceinline__ void enc_rgb(const EncGeom &E, int x, int y, int &r, int &g, int &b) {
    const uint8_t *p = E.img + (int64_t)y * E.pitch + 3 * (int64_t)x;
    const int c0 = p[0], c1 = p[1], c2 = p[2];
    r = E.bgr ? c2 : c0;
    g = c1;
    b = E.bgr ? c0 : c2;
}

// jccolor.c's rgb_ycc_convert (SCALEBITS 16; ONE_HALF - 1 on Cb and Cr)
__device__ __forceinline__ int enc_ycc(const EncGeom &E, int comp, int x, int y) {
    int r, g, b;
    enc_rgb(E, x, y, r, g, b);
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// The sample of component `comp` at (sx, sy) as libjpeg's preprocessing makes it: the last
// column and row replicated; chroma downsampled h2v1 (bias 0, 1, ...) or h2v2 (bias 1, 2, ...)
// over the replicated pixels; below the last downsampled h2v2 row, that row again.
__device__ __forceinline__ int enc_sample(const EncGeom &E, int comp, int sx, int sy) {
    const int W1 = E.w - 1, H1 = E.h - 1;
    if (comp == 0 || E.hm == 1) return enc_ycc(E, comp, min(sx, W1), min(sy, H1));
    const int x0 = min(2 * sx, W1), x1 = min(2 * sx + 1, W1);
    if (E.vm == 1) {
        const int y = min(sy, H1);
        return (enc_ycc(E, comp, x0, y) + enc_ycc(E, comp, x1, y) + (sx & 1)) >> 1;
    }
    const int r = min(sy, (E.h + 1) / 2 - 1);
    const int y0 = min(2 * r, H1), y1 = min(2 * r + 1, H1);
    return (enc_ycc(E, comp, x0, y0) + enc_ycc(E, comp, x1, y0) + enc_ycc(E, comp, x0, y1) +
            enc_ycc(E, comp, x1, y1) + 1 + (sx & 1)) >> 2;
}

// ---- ISLOW FDCT (jfdctint.c: CONST_BITS 13, PASS1_BITS 2), one 8-point pass ------------------------
// FIRST: outputs 0 and 4 shifted left by PASS1_BITS, the rest descaled by CONST_BITS - PASS1_BITS;
// else outputs 0 and 4 descaled by PASS1_BITS, the rest by CONST_BITS + PASS1_BITS.
template <bool FIRST>
__device__ __forceinline__ void enc_fdct8(const int *d, int *o) {
    constexpr int SH = FIRST ? 11 : 15;
    auto ds = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    o[0] = FIRST ? (tmp10 + tmp11) * 4 : ds(tmp10 + tmp11, 2);
    o[4] = FIRST ? (tmp10 - tmp11) * 4 : ds(tmp10 - tmp11, 2);
    const int z1 = (tmp12 + tmp13) * 4433;
    o[2] = ds(z1 + tmp13 * 6270, SH);
    o[6] = ds(z1 - tmp12 * 15137, SH);
    const int y1 = tmp4 + tmp7, y2 = tmp5 + tmp6, y3 = tmp4 + tmp6, y4 = tmp5 + tmp7;
    const int z5 = (y3 + y4) * 9633;
    const int a4 = tmp4 * 2446, a5 = tmp5 * 16819, a6 = tmp6 * 25172, a7 = tmp7 * 12299;
    const int m1 = y1 * -7373, m2 = y2 * -20995, m3 = y3 * -16069 + z5, m4 = y4 * -3196 + z5;
    o[7] = ds(a4 + m1 + m3, SH);
    o[5] = ds(a5 + m2 + m4, SH);
    o[3] = ds(a6 + m2 + m3, SH);
    o[1] = ds(a7 + m1 + m4, SH);
}

// ---- 1. blocks: samples, FDCT, quantisation, zigzag ------------------------------------------------
// ENC_TILE blocks per workgroup, 8 threads per block: thread r makes the samples of row r and its
// row pass, then column r's pass through LDS, then quantises zigzag positions 8r .. 8r + 7 and
// stores them as one 16-byte word.  enc_block is one such step of the whole workgroup: block b of
// image E (live: there is one) goes to dst[0 .. 64); q are the quantisers.
__device__ __forceinline__ void enc_block(const EncGeom &E, const uint8_t (*q)[64], int b, bool live,
                                          int (*tile)[8][9], int16_t *__restrict__ dst) {
    const int j = threadIdx.x >> 3, r = threadIdx.x & 7;
    EncPlace p{0, 0, 0, false};
    if (live) {
        p = enc_place(E, b);
        int d[8], o[8];
        for (int c = 0; c < 8; ++c) d[c] = enc_sample(E, p.comp, 8 * p.bx + c, 8 * p.by + r) - 128;
        enc_fdct8<true>(d, o);
        for (int c = 0; c < 8; ++c) tile[j][r][c] = o[c];
    }
    __syncthreads();
    if (live) {
        int d[8], o[8];
        for (int k = 0; k < 8; ++k) d[k] = tile[j][k][r];
        enc_fdct8<false>(d, o);
        for (int k = 0; k < 8; ++k) tile[j][k][r] = o[k];
    }
    __syncthreads();
    if (live) {
        const uint8_t *qc = q[p.comp ? 1 : 0];
        int16_t v[8];
        for (int i = 0; i < 8; ++i) {
            const int k = 8 * r + i, n = kEncZigzag[k];
            const int x = tile[j][n >> 3][n & 7], dq = 8 * qc[n];
            const int a = ((x < 0 ? -x : x) + (dq >> 1)) / dq;
            v[i] = (int16_t)(p.dummy && k ? 0 : x < 0 ? -a : a);
        }
        uint4 packed;
        packed.x = (uint16_t)v[0] | (uint32_t)(uint16_t)v[1] << 16;
        packed.y = (uint16_t)v[2] | (uint32_t)(uint16_t)v[3] << 16;
        packed.z = (uint16_t)v[4] | (uint32_t)(uint16_t)v[5] << 16;
        packed.w = (uint16_t)v[6] | (uint32_t)(uint16_t)v[7] << 16;
        *(uint4 *)(dst + 8 * r) = packed;
    }
    __syncthreads();
}

// Every stage's kernel is a template over W, "which image", a kernel argument passed by value:
// EncOne for pano_jpeg_encode, EncBatch for pano_jpeg_encode_batch (both at "which image" below).
// S holds what all images share (sampling, channel order, quantisers; nblocks: the blocks of all
// images, numbered one after the other) and where.at(S, g, live) is the image of block g.
struct EncAt {
    EncGeom E;
    int i, first, end;              // the image, its first block, one past its last
};

template <class W>
__global__ __launch_bounds__(ENC_BLOCK) void jpeg_enc_blocks_kernel(EncImage S, W where,
                                                                    int16_t *__restrict__ coef) {
    __shared__ int tile[ENC_TILE][8][9];
    for (int64_t base = (int64_t)blockIdx.x * ENC_TILE; base < S.nblocks;
         base += (int64_t)gridDim.x * ENC_TILE) {
        const int g = (int)base + (threadIdx.x >> 3);
        const bool live = g < S.nblocks;
        const EncAt a = where.at(S, g, live);
        enc_block(a.E, S.q, g - a.first, live, tile, coef + 64 * (int64_t)g);
    }
}

// ---- per-lane codes of one block (one wave, lane k = zigzag position k) -----------------------------
// Lane 0: the DC difference's category code and bits.  Lane k > 0 with a nonzero coefficient: a
// ZRL per 16 zeros before it, the run/size code and the bits.  Lane 63 with a zero: the EOB.
// At most 3 * 11 + 16 + 10 = 59 bits per lane.
struct EncCode {
    uint64_t bits;
    int n;
};
__device__ __forceinline__ void enc_put(EncCode &c, uint32_t e) {
    const int len = (int)(e >> 16);
    c.bits = c.bits << len | (e & 0xFFFF);
    c.n += len;
}
__device__ __forceinline__ void enc_put_value(EncCode &c, int v, int nb) {
    if (!nb) return;
    const uint32_t bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1);
    c.bits = c.bits << nb | bits;
    c.n += nb;
}
__device__ __forceinline__ int enc_nbits(int v) { return v ? 32 - __clz(v < 0 ? -v : v) : 0; }

// the DC of the block before b of the same component in scan order (0 for its first block)
__device__ __forceinline__ int enc_pred_dc(const EncGeom &E, const int16_t *coef, int b) {
    const int mcu = b / E.bpm, k = b - mcu * E.bpm, ny = E.hm * E.vm;
    int prev;
    if (k > 0 && k < ny) prev = b - 1;
    else if (mcu == 0) return 0;
    else prev = b - E.bpm + (k < ny ? ny - 1 : 0);
    return coef[64 * (int64_t)prev];
}

__device__ __forceinline__ EncCode enc_lane_code(const EncGeom &E, const int16_t *coef, int b,
                                                 int lane) {
    const int mcu = b / E.bpm, k = b - mcu * E.bpm;
    const int t = k < E.hm * E.vm ? 0 : 2;
    const int v = coef[64 * (int64_t)b + lane];
    const uint64_t mask = __ballot(v != 0) & ~1ull;
    EncCode c{0, 0};
    if (lane == 0) {
        const int diff = v - enc_pred_dc(E, coef, b), nb = enc_nbits(diff);
        enc_put(c, kEncHuff.e[t][nb]);
        enc_put_value(c, diff, nb);
    } else if (v != 0) {
        const uint64_t before = mask & ((1ull << lane) - 1);
        const int prev = before ? 63 - __clzll(before) : 0;
        int run = lane - prev - 1;
        for (; run > 15; run -= 16) enc_put(c, kEncHuff.e[t + 1][0xF0]);
        const int nb = enc_nbits(v);
        enc_put(c, kEncHuff.e[t + 1][run << 4 | nb]);
        enc_put_value(c, v, nb);
    } else if (lane == 63) {
        enc_put(c, kEncHuff.e[t + 1][0x00]);
    }
    return c;
}

// ---- 2. bit counts: one wave per block ------------------------------------------------------------
template <class W>
__global__ __launch_bounds__(ENC_BLOCK) void jpeg_enc_count_kernel(EncImage S, W where,
                                                                   const int16_t *__restrict__ coef,
                                                                   uint32_t *__restrict__ counts) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t g = (int64_t)blockIdx.x * ENC_WAVES + wave; g < S.nblocks;
         g += (int64_t)gridDim.x * ENC_WAVES) {
        const EncAt a = where.at(S, (int)g, true);
        const int bits = wave_sum(
            enc_lane_code(a.E, coef + 64 * (int64_t)a.first, (int)g - a.first, lane).n);
        if (lane == 0) counts[g] = (uint32_t)bits;
    }
}

// ---- 3. exclusive scan of uint32 values into int64 offsets ------------------------------------------
// local: each workgroup scans a tile of ENC_SCAN_TILE values (its offsets relative to the tile) and
// writes the tile's sum to part[tile]; parts: one workgroup (wave.h: scan_exclusive_kernel) scans
// part[0 .. nparts) in place and writes the total to part[nparts].  The offset of value i is
// out[i] + part[i / ENC_SCAN_TILE].
__global__ __launch_bounds__(ENC_SCAN) void jpeg_enc_scan_local_kernel(
    const uint32_t *__restrict__ in, int64_t n, int64_t *__restrict__ out, int64_t *__restrict__ part) {
    __shared__ int64_t waves[ENC_SCAN / 64];
    const int64_t i0 = (int64_t)blockIdx.x * ENC_SCAN_TILE + (int64_t)threadIdx.x * ENC_SCAN_ITEMS;
    uint32_t v[ENC_SCAN_ITEMS];
    int64_t sum = 0;
    for (int k = 0; k < ENC_SCAN_ITEMS; ++k) {
        v[k] = i0 + k < n ? in[i0 + k] : 0;
        sum += v[k];
    }
    int64_t total;
    int64_t run = block_scan_exclusive<ENC_SCAN>(sum, waves, total);
    for (int k = 0; k < ENC_SCAN_ITEMS; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += v[k];
    }
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__device__ __forceinline__ int64_t enc_offset(const int64_t *off, const int64_t *part, int64_t i) {
    return off[i] + part[i / ENC_SCAN_TILE];
}

// ---- 4. emission: one wave per block ---------------------------------------------------------------
// The wave ORs its lanes' codes into LDS words (bit 0 of the stream = the most significant bit),
// then stores them byte-swapped: words wholly inside the block with plain stores, its first and
// last word with atomicOr (they may be shared with the neighbouring blocks; the buffer was zeroed
// and the bits are disjoint, so the order does not matter).  The last block also writes the 1-bits
// that pad the stream to a whole byte.
__device__ __forceinline__ void enc_or_bits(uint32_t *lw, int p, uint64_t bits, int n) {
    while (n > 0) {
        const int room = 32 - (p & 31), take = n < room ? n : room;
        const uint32_t chunk = (uint32_t)(bits >> (n - take)) & (take == 32 ? ~0u : (1u << take) - 1);
        atomicOr(&lw[p >> 5], chunk << (room - take));
        p += take;
        n -= take;
    }
}

// enc_emit_block is one such step of the whole workgroup: the wave's block b of image E (live:
// there is one; coef: the image's first block) has `nbits` bits and starts at bit b0 of raw; the
// image's last block pads.  lw: the wave's ENC_WORDS words of LDS.
__device__ __forceinline__ void enc_emit_block(const EncGeom &E, const int16_t *__restrict__ coef,
                                               int b, bool live, int64_t b0, int nbits, bool last,
                                               uint32_t *lw, uint32_t *__restrict__ raw) {
    const int lane = threadIdx.x & 63;
    lw[lane] = 0;
    __syncthreads();
    if (live) {
        const EncCode c = enc_lane_code(E, coef, b, lane);
        const int x = wave_scan_inclusive(c.n);
        const int p = (int)(b0 & 31) + x - c.n;
        enc_or_bits(lw, p, c.bits, c.n);
        if (last) {
            const int pad = (int)(-(b0 + nbits) & 7);
            if (lane == 63 && pad) enc_or_bits(lw, (int)(b0 & 31) + nbits, (1u << pad) - 1, pad);
            nbits += pad;
        }
    }
    __syncthreads();
    if (live) {
        const int nwords = (int)(((b0 & 31) + nbits + 31) >> 5);
        uint32_t *dst = raw + (b0 >> 5);
        for (int i = lane; i < nwords; i += 64) {
            const uint32_t v = __builtin_bswap32(lw[i]);
            if (i == 0 || i == nwords - 1) atomicOr(&dst[i], v);
            else dst[i] = v;
        }
    }
    __syncthreads();
}

// where.bit0(a, off, part, g): the bit of raw at which block g, of image a, starts
template <class W>
__global__ __launch_bounds__(ENC_BLOCK) void jpeg_enc_emit_kernel(
    EncImage S, W where, const int16_t *__restrict__ coef, const uint32_t *__restrict__ counts,
    const int64_t *__restrict__ off, const int64_t *__restrict__ part, uint32_t *__restrict__ raw) {
    __shared__ uint32_t words[ENC_WAVES][ENC_WORDS];
    const int wave = threadIdx.x >> 6;
    for (int64_t base = (int64_t)blockIdx.x * ENC_WAVES; base < S.nblocks;
         base += (int64_t)gridDim.x * ENC_WAVES) {
        const int64_t g = base + wave;
        const bool live = g < S.nblocks;
        const EncAt a = where.at(S, (int)g, live);
        enc_emit_block(a.E, coef + 64 * (int64_t)a.first, (int)g - a.first, live,
                       live ? where.bit0(a, off, part, g) : 0, live ? (int)counts[g] : 0,
                       g == a.end - 1, words[wave], raw);
    }
}

// ---- 5. byte stuffing ------------------------------------------------------------------------------
// count: the 0xFF bytes of each ENC_CHUNK-byte chunk (the buffer is zero past the stream, and a
// zero is never counted); write (after the scan): each chunk's bytes at its shifted place, a 0x00
// after every 0xFF.
__device__ __forceinline__ uint32_t enc_chunk_ffs(const uint32_t *__restrict__ raw, int64_t c) {
    const uint4 *p = (const uint4 *)(raw + c * (ENC_CHUNK / 4));
    uint32_t n = 0;
    for (int i = 0; i < ENC_CHUNK / 16; ++i) {
        const uint4 v = p[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < 4; ++k)
            for (int s = 0; s < 32; s += 8) n += ((w[k] >> s) & 0xFF) == 0xFF;
    }
    return n;
}

// where.counted(c): what chunk c's count holds besides its 0xFF bytes
template <class W>
__global__ __launch_bounds__(ENC_BLOCK) void jpeg_enc_stuff_count_kernel(
    W where, const uint32_t *__restrict__ raw, int64_t nchunks, uint32_t *__restrict__ counts) {
    const int64_t c = (int64_t)blockIdx.x * ENC_BLOCK + threadIdx.x;
    if (c >= nchunks) return;
    counts[c] = where.counted(c) + enc_chunk_ffs(raw, c);
}

// bytes [a, e) of raw to out[o ...], a 0x00 after every 0xFF; returns where the next byte goes
__device__ __forceinline__ int64_t enc_stuff_bytes(const uint8_t *__restrict__ raw, int64_t a,
                                                   int64_t e, uint8_t *__restrict__ out, int64_t o) {
    for (int64_t i = a; i < e; ++i) {
        const uint8_t v = raw[i];
        out[o++] = v;
        if (v == 0xFF) out[o++] = 0;
    }
    return o;
}

// where.stuff(raw, c, nbytes, nchunks, o, out): chunk c's bytes to their place in out; o is the
// scan of the counts before c, nbytes the end of raw
template <class W>
__global__ __launch_bounds__(ENC_BLOCK) void jpeg_enc_stuff_write_kernel(
    W where, const uint8_t *__restrict__ raw, int64_t nbytes, int64_t nchunks,
    const int64_t *__restrict__ off, const int64_t *__restrict__ part, uint8_t *__restrict__ out) {
    const int64_t c = (int64_t)blockIdx.x * ENC_BLOCK + threadIdx.x;
    if (c >= nchunks) return;
    where.stuff(raw, c, nbytes, nchunks, enc_offset(off, part, c), out);
}

// ---- which image: one (pano_jpeg_encode) ---------------------------------------------------------
// The image is S itself.  Its bits start at bit 0 of raw, a chunk's count is its 0xFF bytes, so a
// chunk's bytes move up by the scan of the counts, and the stuffed stream is all of out.
struct EncOne {
    static constexpr bool kBatch = false;
    static constexpr int n = 1;
    static constexpr int64_t head = 0;
    __device__ EncAt at(const EncImage &S, int, bool) const { return {S, 0, 0, S.nblocks}; }
    __device__ int64_t bit0(const EncAt &, const int64_t *off, const int64_t *part, int64_t g) const {
        return enc_offset(off, part, g);
    }
    __device__ uint32_t counted(int64_t) const { return 0; }
    static int64_t stuffed(int64_t nbytes, int64_t sum) { return nbytes + sum; }
    __device__ void stuff(const uint8_t *__restrict__ raw, int64_t c, int64_t nbytes, int64_t,
                          int64_t o, uint8_t *__restrict__ out) const {
        const int64_t a = c * ENC_CHUNK, e = a + ENC_CHUNK < nbytes ? a + ENC_CHUNK : nbytes;
        enc_stuff_bytes(raw, a, e, out, a + o);
    }
};

// ---- which image: a batch (pano_jpeg_encode_batch) -----------------------------------------------
// The blocks of all images are numbered one after the other, image by image; first[i] is image
// i's first block (first[n]: the total) and a block finds its image by bisecting that table, so
// the stages run on (image, block in the image) and their workgroups straddle images freely.  (A
// faster search, wave-wide or one per workgroup, goes into at() and nowhere else.)  The counts of
// all blocks are scanned together; an image's bits are the difference of the offsets at its two
// ends.  Every image's raw bits start on a whole stuffing chunk (chunk0[i], from a scan of the
// images' chunk counts), so no word, pad byte or 0xFF of one image touches another's, and the
// stuffed streams are packed byte after byte: a chunk's count is its stream bytes plus its 0xFF
// bytes, and the scan of those is the output position.  out: int64 offsets[n + 1] of the images'
// streams, then (at out + head) the streams.
struct EncDesc {
    const uint8_t *img;
    int64_t pitch;
    int w, h, mx, my;
    int wib[2], hib[2];
};

// the largest i in [0, n) with t[i] <= v (t ascending, t[0] <= v)
template <class T>
__device__ __forceinline__ int enc_find(const T *__restrict__ t, int n, T v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct EncBatch {
    static constexpr bool kBatch = true;
    const EncDesc *__restrict__ desc;
    const int *__restrict__ first;
    int n;
    int64_t *__restrict__ chunk0, *__restrict__ ibytes;     // per image: first chunk, stream bytes
    int64_t head;                                           // bytes of the offsets in front of the streams

    __device__ EncAt at(const EncImage &S, int g, bool live) const {
        const int i = live ? enc_find(first, n, g) : 0;
        const EncDesc d = desc[i];
        EncAt a{S, i, first[i], first[i + 1]};
        a.E.img = d.img;
        a.E.pitch = d.pitch;
        a.E.w = d.w;
        a.E.h = d.h;
        a.E.mx = d.mx;
        a.E.my = d.my;
        a.E.wib[0] = d.wib[0];
        a.E.wib[1] = d.wib[1];
        a.E.hib[0] = d.hib[0];
        a.E.hib[1] = d.hib[1];
        a.E.nblocks = a.end - a.first;
        return a;
    }
    __device__ int64_t bit0(const EncAt &a, const int64_t *off, const int64_t *part, int64_t g) const {
        return chunk0[a.i] * (8 * ENC_CHUNK) + enc_offset(off, part, g) - enc_offset(off, part, a.first);
    }
    // the stream bytes of chunk c, which is image i's
    __device__ int chunk_bytes(int i, int64_t c) const {
        const int64_t left = ibytes[i] - (c - chunk0[i]) * ENC_CHUNK;
        return (int)(left < ENC_CHUNK ? left : ENC_CHUNK);
    }
    __device__ uint32_t counted(int64_t c) const {
        return (uint32_t)chunk_bytes(enc_find(chunk0, n, c), c);
    }
    static int64_t stuffed(int64_t, int64_t sum) { return sum; }
    __device__ void stuff(const uint8_t *__restrict__ raw, int64_t c, int64_t, int64_t nchunks,
                          int64_t o, uint8_t *__restrict__ out) const {
        const int i = enc_find(chunk0, n, c);
        const int64_t a = c * ENC_CHUNK;
        const int64_t end = enc_stuff_bytes(raw, a, a + chunk_bytes(i, c), out + head, o);
        int64_t *offsets = (int64_t *)out;
        if (c == chunk0[i]) offsets[i] = o;
        if (c == nchunks - 1) offsets[n] = end;
    }
};

// per image: its stream's bytes before stuffing (the bits of its blocks, padded to a byte) and its
// chunks.  nparts: the parts of the blocks' scan, part[nparts] their total.
__global__ __launch_bounds__(ENC_BLOCK) void jpeg_enc_batch_images_kernel(
    const int *__restrict__ first, int n, const int64_t *__restrict__ off,
    const int64_t *__restrict__ part, int64_t nparts, int64_t *__restrict__ ibytes,
    int64_t *__restrict__ ichunks) {
    const int i = blockIdx.x * ENC_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t a = enc_offset(off, part, first[i]);
    const int64_t e = i + 1 < n ? enc_offset(off, part, first[i + 1]) : part[nparts];
    const int64_t bytes = (e - a + 7) >> 3;
    ibytes[i] = bytes;
    ichunks[i] = (bytes + ENC_CHUNK - 1) / ENC_CHUNK;
}

// ---- the scratch and the checks --------------------------------------------------------------------
// the scratch of pano_jpeg_encode: coefficients, bit counts, bit offsets, scan parts
struct EncWork {
    int64_t coef, counts, offs, parts, bytes;
};
static EncWork enc_work(int64_t nblocks) {
    EncWork w;
    w.coef = 0;
    w.counts = align_up(128 * nblocks);
    w.offs = w.counts + align_up(4 * nblocks);
    w.parts = w.offs + align_up(8 * nblocks);
    w.bytes = w.parts + align_up(8 * (ceil_div(nblocks, ENC_SCAN_TILE) + 1));
    return w;
}

static bool enc_geometry(int h, int w, int subsampling, EncImage &E) {
    if (h < 1 || w < 1 || h > PANO_JPEG_MAX_SIDE || w > PANO_JPEG_MAX_SIDE || subsampling < 0 ||
        subsampling > 2)
        return false;
    E.w = w;
    E.h = h;
    E.hm = subsampling == 0 ? 1 : 2;
    E.vm = subsampling == 2 ? 2 : 1;
    E.mx = ceil_div(w, 8 * E.hm);
    E.my = ceil_div(h, 8 * E.vm);
    E.bpm = E.hm * E.vm + 2;
    E.wib[0] = ceil_div(w, 8);
    E.hib[0] = ceil_div(h, 8);
    E.wib[1] = ceil_div(ceil_div(w, E.hm), 8);
    E.hib[1] = ceil_div(ceil_div(h, E.vm), 8);
    E.nblocks = E.mx * E.my * E.bpm;
    return true;
}

extern "C" size_t pano_jpeg_encode_work_bytes(int h, int w, int subsampling) {
    EncImage E;
    if (!enc_geometry(h, w, subsampling, E)) return 0;
    return (size_t)enc_work(E.nblocks).bytes;
}

static int enc_scan(pano_ctx *ctx, hipStream_t s, const uint32_t *in, int64_t n, int64_t *out,
                    int64_t *part) {
    const int64_t nparts = ceil_div(n, ENC_SCAN_TILE);
    PANO_TIMED(PK_JPEG_ENC_SCAN, s,
               hipLaunchKernelGGL(jpeg_enc_scan_local_kernel, dim3((unsigned)nparts),
                                  dim3(ENC_SCAN), 0, s, in, n, out, part));
    PANO_LAUNCH_CHECK("jpeg_enc_scan_local_kernel");
    PANO_TIMED(PK_JPEG_ENC_SCAN, s,
               hipLaunchKernelGGL((scan_exclusive_kernel<ENC_SCAN, int64_t>), dim3(1), dim3(ENC_SCAN),
                                  0, s, (const int64_t *)part, nparts, part));
    PANO_LAUNCH_CHECK("scan_exclusive_kernel");
    return PANO_OK;
}

static inline dim3 enc_groups(int64_t n, int per) {
    return capped_grid(ceil_div(n, per), ENC_MAX_GROUPS);
}

// the scratch of pano_jpeg_encode_batch: EncWork, then the first-block table, the descriptors (the
// two are uploaded as one), the images' bytes and their chunks (scanned in place)
struct EncBatchWork {
    EncWork w;
    int64_t first, desc, ibytes, ichunks, bytes;
    int64_t table_bytes;            // first and desc
};
static EncBatchWork enc_batch_work(int64_t nblocks, int64_t n) {
    EncBatchWork b;
    b.w = enc_work(nblocks);
    b.first = b.w.bytes;
    b.desc = b.first + align_up(4 * (n + 1));
    b.ibytes = b.desc + align_up((int64_t)sizeof(EncDesc) * n);
    b.table_bytes = b.ibytes - b.first;
    b.ichunks = b.ibytes + align_up(8 * n);
    b.bytes = b.ichunks + align_up(8 * (n + 1));
    return b;
}

extern "C" size_t pano_jpeg_encode_batch_work_bytes(int64_t blocks, int n) {
    if (blocks < 1 || blocks > PANO_JPEG_BATCH_MAX_BLOCKS || n < 1 || n > PANO_JPEG_BATCH_MAX) return 0;
    return (size_t)enc_batch_work(blocks, n).bytes;
}

// What both entry points check (who: the one that was called, for the messages).  Image i:
// its geometry into E.
static int enc_check_image(const char *who, int i, const uint8_t *img, int h, int w, int64_t pitch,
                           int subsampling, EncImage &E) {
    PANO_REQUIRE(img && enc_geometry(h, w, subsampling, E),
                 "%s: image %d: %d x %d at %p, subsampling %d (1..%d per side, 0..2)", who, i, w, h,
                 (const void *)img, subsampling, PANO_JPEG_MAX_SIDE);
    PANO_REQUIRE(pitch >= 3 * (int64_t)w, "%s: image %d: pitch %lld for %d pixels", who, i,
                 (long long)pitch, w);
    return PANO_OK;
}
// The settings, into S, and the scratch's size.
static int enc_check_call(const char *who, int flags, const uint8_t *qt, int64_t work_bytes,
                          int64_t needed, EncImage &S) {
    PANO_REQUIRE((flags & ~PANO_JPEG_BGR) == 0, "%s: flags %d", who, flags);
    for (int i = 0; i < 128; ++i) PANO_REQUIRE(qt[i] >= 1, "%s: quantiser %d is 0", who, i);
    PANO_REQUIRE(work_bytes >= needed, "%s: work of %lld bytes, %lld needed", who,
                 (long long)work_bytes, (long long)needed);
    S.bgr = flags & PANO_JPEG_BGR;
    for (int i = 0; i < 128; ++i) S.q[i >> 6][i & 63] = qt[i];
    return PANO_OK;
}

static int enc_wait(hipStream_t s, const int64_t *dev, int64_t &v) {
    PANO_HIP(hipMemcpyAsync(&v, dev, 8, hipMemcpyDeviceToHost, s));
    PANO_HIP(hipStreamSynchronize(s));
    return PANO_OK;
}

// ---- the driver of both entry points ---------------------------------------------------------------
// S: what the images share, nblocks the blocks of all of them; work, L: the scratch (checked).
// Leaves in pinned memory at *host, where.head bytes in (the batch's offsets come first), the
// *out_bytes bytes of the stuffed streams.  Waits on the stream three times.
template <class W>
static int enc_run(pano_ctx *ctx, hipStream_t s, const char *who, const EncImage &S, const W &where,
                   void *work, const EncWork &L, const uint8_t **host, int64_t *out_bytes) {
    uint8_t *w8 = (uint8_t *)work;
    int16_t *coef = (int16_t *)(w8 + L.coef);
    uint32_t *counts = (uint32_t *)(w8 + L.counts);
    int64_t *offs = (int64_t *)(w8 + L.offs), *parts = (int64_t *)(w8 + L.parts);
    const int64_t nb = S.nblocks, nbparts = ceil_div(nb, ENC_SCAN_TILE);

    // 1. blocks, 2. bit counts, 3. their scan
    PANO_TIMED(PK_JPEG_ENC_BLOCKS, s,
               hipLaunchKernelGGL(jpeg_enc_blocks_kernel<W>, enc_groups(nb, ENC_TILE), dim3(ENC_BLOCK),
                                  0, s, S, where, coef));
    PANO_LAUNCH_CHECK("jpeg_enc_blocks_kernel");
    PANO_TIMED(PK_JPEG_ENC_COUNT, s,
               hipLaunchKernelGGL(jpeg_enc_count_kernel<W>, enc_groups(nb, ENC_WAVES), dim3(ENC_BLOCK),
                                  0, s, S, where, (const int16_t *)coef, counts));
    PANO_LAUNCH_CHECK("jpeg_enc_count_kernel");
    if (int rc = enc_scan(ctx, s, counts, nb, offs, parts)) return rc;

    // wait for the size of raw: nchunks chunks, nbytes to its end
    int64_t nbytes = 0, nchunks = 0;
    if constexpr (W::kBatch) {      // the images' bytes and chunks, each image on chunks of its own
        PANO_TIMED(PK_JPEG_ENC_SCAN, s,
                   hipLaunchKernelGGL(jpeg_enc_batch_images_kernel, dim3(ceil_div(where.n, ENC_BLOCK)),
                                      dim3(ENC_BLOCK), 0, s, where.first, where.n, (const int64_t *)offs,
                                      (const int64_t *)parts, nbparts, where.ibytes, where.chunk0));
        PANO_LAUNCH_CHECK("jpeg_enc_batch_images_kernel");
        PANO_TIMED(PK_JPEG_ENC_SCAN, s,
                   hipLaunchKernelGGL((scan_exclusive_kernel<ENC_SCAN, int64_t>), dim3(1), dim3(ENC_SCAN),
                                      0, s, (const int64_t *)where.chunk0, (int64_t)where.n,
                                      where.chunk0));
        PANO_LAUNCH_CHECK("scan_exclusive_kernel");
        if (int rc = enc_wait(s, where.chunk0 + where.n, nchunks)) return rc;
        PANO_REQUIRE(nchunks >= where.n && nchunks < ((int64_t)1 << 34), "%s: %lld chunks", who,
                     (long long)nchunks);
        nbytes = nchunks * ENC_CHUNK;
    } else {                        // the bits of the one stream
        int64_t total_bits = 0;
        if (int rc = enc_wait(s, parts + nbparts, total_bits)) return rc;
        PANO_REQUIRE(total_bits > 0 && total_bits < ((int64_t)1 << 40), "%s: %lld bits", who,
                     (long long)total_bits);
        nbytes = ceil_div(total_bits, 8);
        nchunks = ceil_div(nbytes, ENC_CHUNK);
    }

    // the stream buffer: raw words (whole chunks, zeroed), the chunks' counts and offsets
    const int64_t raw_bytes = align_up(nchunks * ENC_CHUNK), cnt_at = raw_bytes,
                  off_at = cnt_at + align_up(4 * nchunks), part_at = off_at + align_up(8 * nchunks),
                  ncparts = ceil_div(nchunks, ENC_SCAN_TILE),
                  dev_bytes = part_at + align_up(8 * (ncparts + 1));
    // (the context's buffers grow with a quarter to spare; the stream is idle, nothing reads them)
    if (int rc = pano_buf_reserve(ctx->buf[BUF_ENC_DEV], dev_bytes, false, dev_bytes / 4)) return rc;
    uint8_t *const dev = (uint8_t *)ctx->buf[BUF_ENC_DEV].p;
    uint32_t *raw = (uint32_t *)dev;
    uint32_t *ccount = (uint32_t *)(dev + cnt_at);
    int64_t *coff = (int64_t *)(dev + off_at), *cpart = (int64_t *)(dev + part_at);
    PANO_HIP(hipMemsetAsync(raw, 0, raw_bytes, s));

    // 4. emission, 5. the chunks' counts and their scan; wait for the stuffed size
    PANO_TIMED(PK_JPEG_ENC_EMIT, s,
               hipLaunchKernelGGL(jpeg_enc_emit_kernel<W>, enc_groups(nb, ENC_WAVES), dim3(ENC_BLOCK),
                                  0, s, S, where, (const int16_t *)coef, (const uint32_t *)counts,
                                  (const int64_t *)offs, (const int64_t *)parts, raw));
    PANO_LAUNCH_CHECK("jpeg_enc_emit_kernel");
    const dim3 cgrid((unsigned)ceil_div(nchunks, ENC_BLOCK));
    PANO_TIMED(PK_JPEG_ENC_STUFF, s,
               hipLaunchKernelGGL(jpeg_enc_stuff_count_kernel<W>, cgrid, dim3(ENC_BLOCK), 0, s, where,
                                  (const uint32_t *)raw, nchunks, ccount));
    PANO_LAUNCH_CHECK("jpeg_enc_stuff_count_kernel");
    if (int rc = enc_scan(ctx, s, ccount, nchunks, coff, cpart)) return rc;
    int64_t sum = 0;
    if (int rc = enc_wait(s, cpart + ncparts, sum)) return rc;
    const int64_t stuffed = W::stuffed(nbytes, sum), all_bytes = where.head + stuffed;
    PANO_REQUIRE(sum >= 0 && stuffed >= where.n && stuffed <= 2 * nbytes,
                 "%s: %lld bytes after stuffing %lld", who, (long long)stuffed, (long long)nbytes);
    if (int rc = pano_buf_reserve(ctx->buf[BUF_ENC_OUT], all_bytes, false, all_bytes / 4)) return rc;
    if (int rc = pano_buf_reserve(ctx->buf[BUF_ENC_HOST], all_bytes, true, all_bytes / 4)) return rc;
    uint8_t *const out = (uint8_t *)ctx->buf[BUF_ENC_OUT].p;
    uint8_t *const pinned = (uint8_t *)ctx->buf[BUF_ENC_HOST].p;
    PANO_TIMED(PK_JPEG_ENC_STUFF, s,
               hipLaunchKernelGGL(jpeg_enc_stuff_write_kernel<W>, cgrid, dim3(ENC_BLOCK), 0, s, where,
                                  (const uint8_t *)raw, nbytes, nchunks, (const int64_t *)coff,
                                  (const int64_t *)cpart, out));
    PANO_LAUNCH_CHECK("jpeg_enc_stuff_write_kernel");

    // the download (a batch's offsets and streams in one copy)
    PANO_HIP(hipMemcpyAsync(pinned, out, all_bytes, hipMemcpyDeviceToHost, s));
    PANO_HIP(hipStreamSynchronize(s));
    *host = pinned;
    *out_bytes = stuffed;
    return PANO_OK;
}

// ---- the entry points ------------------------------------------------------------------------------
extern "C" int pano_jpeg_encode(pano_ctx *ctx, const uint8_t *img, int h, int w, int64_t pitch,
                                int flags, int subsampling, const uint8_t *qt, void *work,
                                int64_t work_bytes, const uint8_t **stream_out,
                                int64_t *stream_bytes) {
    const char *const who = "pano_jpeg_encode";
    PANO_ENTER(ctx, who);
    PANO_REQUIRE(img && qt && work && stream_out && stream_bytes, "%s: null pointer", who);
    *stream_out = nullptr;
    *stream_bytes = 0;
    EncImage S;
    if (int rc = enc_check_image(who, 0, img, h, w, pitch, subsampling, S)) return rc;
    const EncWork L = enc_work(S.nblocks);
    if (int rc = enc_check_call(who, flags, qt, work_bytes, L.bytes, S)) return rc;
    S.img = img;
    S.pitch = pitch;
    return enc_run(ctx, (hipStream_t)stream, who, S, EncOne{}, work, L, stream_out, stream_bytes);
}

extern "C" int pano_jpeg_encode_batch(pano_ctx *ctx, const pano_jpeg_image *images, int n, int flags,
                                      int subsampling, const uint8_t *qt, void *work,
                                      int64_t work_bytes, const uint8_t **streams,
                                      const int64_t **offsets) {
    const char *const who = "pano_jpeg_encode_batch";
    PANO_ENTER(ctx, who);
    PANO_REQUIRE(images && qt && work && streams && offsets, "%s: null pointer", who);
    *streams = nullptr;
    *offsets = nullptr;
    PANO_REQUIRE(n >= 1 && n <= PANO_JPEG_BATCH_MAX, "%s: %d images (1..%d)", who, n,
                 PANO_JPEG_BATCH_MAX);
    EncImage S{};                   // no image or pitch of its own
    int64_t nb = 0;
    for (int i = 0; i < n; ++i) {
        const pano_jpeg_image &m = images[i];
        if (int rc = enc_check_image(who, i, m.img, m.h, m.w, m.pitch, subsampling, S)) return rc;
        nb += S.nblocks;
        PANO_REQUIRE(nb <= PANO_JPEG_BATCH_MAX_BLOCKS, "%s: more than %d blocks", who,
                     PANO_JPEG_BATCH_MAX_BLOCKS);
    }
    const EncBatchWork L = enc_batch_work(nb, n);
    if (int rc = enc_check_call(who, flags, qt, work_bytes, L.bytes, S)) return rc;

    // the tables, staged in the pinned buffer (the last call's streams end here), and their upload
    if (int rc = pano_buf_reserve(ctx->buf[BUF_ENC_HOST], L.table_bytes, true)) return rc;
    uint8_t *const stage = (uint8_t *)ctx->buf[BUF_ENC_HOST].p;
    int *const hfirst = (int *)stage;
    EncDesc *const hdesc = (EncDesc *)(stage + (L.desc - L.first));
    nb = 0;
    for (int i = 0; i < n; ++i) {
        const pano_jpeg_image &m = images[i];
        enc_geometry(m.h, m.w, subsampling, S);
        hfirst[i] = (int)nb;
        hdesc[i] = EncDesc{m.img, m.pitch, S.w, S.h, S.mx, S.my, {S.wib[0], S.wib[1]},
                           {S.hib[0], S.hib[1]}};
        nb += S.nblocks;
    }
    hfirst[n] = (int)nb;
    S.nblocks = (int)nb;
    const hipStream_t s = (hipStream_t)stream;
    uint8_t *w8 = (uint8_t *)work;
    PANO_HIP(hipMemcpyAsync(w8 + L.first, stage, L.table_bytes, hipMemcpyHostToDevice, s));
    const EncBatch where{(const EncDesc *)(w8 + L.desc), (const int *)(w8 + L.first), n,
                         (int64_t *)(w8 + L.ichunks), (int64_t *)(w8 + L.ibytes),
                         align_up(8 * ((int64_t)n + 1))};
    const uint8_t *host = nullptr;
    int64_t out_bytes = 0;
    if (int rc = enc_run(ctx, s, who, S, where, work, L.w, &host, &out_bytes)) return rc;
    *offsets = (const int64_t *)host;
    *streams = host + where.head;
    return PANO_OK;
}

