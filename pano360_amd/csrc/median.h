// ---- median blend: vote out what moved, blend the rest linearly ----------------------------------
// No reference counterpart; DESIGN.md section 5m and include/pano360.h state the contract.  One
// thread per mosaic pixel, like the linear blends above, in up to three walks over the pixel's
// samples (a sampler yields them in index order: the fused one walks prune_masked_cameras'
// candidates and takes each sample with camera_sees and sample_camera, the routines of blend.hip
// that blend_cameras_kernel calls too; the stage one reads whole-patch planes):
//   1. every sample: the integer weight total T, the per-channel range of the colours, the plain
//      linear sums, and (key, weight) of the first PANO_MEDIAN_KEEP samples into LDS.  Where the
//      range is within tol in all three channels every sample is an inlier whichever the median
//      is (float subtraction is monotonic: |c_i - c_j| <= max - min <= tol after rounding too),
//      and the linear sums ARE the result: a static scene takes this walk alone (a dozen
//      instructions per sample more than the linear blend, but at the occupancy the LDS below
//      leaves: DESIGN.md 5m has the times).  T = 0: every sample is an inlier by definition,
//      same exit.
//   2. otherwise the median sample j: the stored entries are consumed in ascending (key, index)
//      order - repeated minimum search, about m^2 / 2 LDS reads for m entries; a bisection of the
//      32-bit key space is 32 m and only wins beyond m = 64 - until twice the running weight
//      reaches T.  Weights are integers, so the sum does not depend on the order they are added in.
//   3. c_j is sampled again (cameras before j are only mapped, not sampled), then every sample
//      again: the inliers' linear sums, in index order.
// Re-sampling instead of keeping the colours: a kept sample would be 16 bytes instead of 8, which
// halves either the samples held or the workgroups per CU, to save the second sampling on the
// pixels that need a vote at all - in a static scene those are the few per cent along
// misregistered edges.  The samples are recomputed by the same instructions on the same operands
// (no contraction, no reassociation), so they are the same bits.
//
// LDS: 2 PANO_MEDIAN_KEEP dwords per thread, laid out [dword][thread]: a wave's 64 lanes read 64
// consecutive dwords, one per bank, whatever entry each lane is at.  32 x 8 B x 256 threads =
// 64 KiB per workgroup, + 3.1 KiB of camera lists and the colour table in the fused kernel =
// 67.1 KiB: floor(160 / 67.1) = 2 workgroups = 8 waves per CU (3 would need KEEP <= 24).  Two
// waves per SIMD leave each 256 VGPRs.  Measured: 2.8 x the linear blend where no
// pixel votes.  The likely cause, a hypothesis no measurement has isolated yet: a sample is a chain
// of dependent loads that two waves per SIMD cannot cover, where the linear kernel runs eight.
//
// More than PANO_MEDIAN_KEEP samples at a pixel (more than 32 frames over one point): the sorted
// order is consumed in passes.  A pass walks the samples again and keeps the MED_OVER smallest
// (key, index) pairs above the last one consumed - an entry then carries its index, 12 bytes, so
// the same LDS holds 21 of them - and consumes those; it ends when 2 S >= T.  ceil(m / 21) passes.
//
// Everything in this file is plain C++ over a sampler, so that a host program can run it
// (tests/test_median_pixel_host.py does, under the address and undefined-behaviour sanitizers): the
// includer provides __device__, __forceinline__, __restrict__, __float_as_uint and __fdiv_rn.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/pano360.h"

#define MED_KEEP PANO_MEDIAN_KEEP
#define MED_OVER ((2 * MED_KEEP) / 3)
#define MED_ALL 0x7fffffff
// PANO_MEDIAN_KEEP may be set when the library is compiled (an A/B of the LDS footprint);
// _lib.MEDIAN_KEEP, which the probe's and the tests' sample-count figures use, must then follow.
static_assert(MED_KEEP >= 2, "an overflow pass holds 2 KEEP / 3 >= 1 entries");
static_assert(2 * MED_KEEP * 256 * 4 + 4096 <= 160 * 1024,
              "the entries and the fused kernel's lists fit a CU's LDS");

__device__ __forceinline__ uint32_t median_weight(float a) {
    return (uint32_t)(fminf(fmaxf(a, 0.0f), 1.0f) * 1073741824.0f);       // exact: a power of two
}

// (c0 + c1) + c2 as an unsigned integer that orders like the float (-0 counts as +0)
__device__ __forceinline__ uint32_t median_key(const float *c) {
    float k = (c[0] + c[1]) + c[2];
    k = k + 0.0f;
    const uint32_t u = __float_as_uint(k);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

// Consumes the m entries of a thread in ascending (key, index) order, those above `last` only,
// adding their weights to S; returns the index of the entry at which 2 S >= T, or -1 when the
// entries run out first (`last` is then the largest of them).  INDEXED: entries of three dwords
// {key, index, weight}; else two, {key, weight}, and the entry's position is its index.
template <bool INDEXED>
__device__ __forceinline__ int median_consume(uint32_t (*mem)[256], int tid, int m, uint64_t T,
                                              uint64_t &S, uint64_t &last, bool &has_last) {
    constexpr int D = INDEXED ? 3 : 2;
    for (int step = 0; step < m; ++step) {
        uint64_t best = ~0ull;
        uint32_t best_w = 0;
        for (int e = 0; e < m; ++e) {
            const uint32_t w = mem[D * e + D - 1][tid];
            const uint32_t idx = INDEXED ? mem[D * e + 1][tid] : (uint32_t)e;
            const uint64_t pair = ((uint64_t)mem[D * e][tid] << 32) | idx;
            if (w != 0 && (!has_last || pair > last) && pair < best) {
                best = pair;
                best_w = w;
            }
        }
        if (best_w == 0) return -1;
        S += best_w;
        last = best;
        has_last = true;
        if (2 * S >= T) return (int)(uint32_t)best;
    }
    return -1;
}

// One pixel.  sm.walk(lo, hi, visit) calls visit(ord, colour[3], alpha) for the pixel's samples
// number lo .. hi in index order (numbered from 0).  Returns whether the pixel has a sample.
template <class Sampler>
__device__ __forceinline__ bool median_pixel(const Sampler &sm, uint32_t (*mem)[256], int tid,
                                             float tol, uint8_t *__restrict__ out) {
    float acc[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint64_t T = 0;
    int count = 0;
    sm.walk(0, MED_ALL, [&](int ord, const float *c, float a) {
        const uint32_t w = median_weight(a);
        T += w;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            acc[ch] = acc[ch] + c[ch] * a;
            lo[ch] = fminf(lo[ch], c[ch]);
            hi[ch] = fmaxf(hi[ch], c[ch]);
        }
        wsum = wsum + a;
        if (ord < MED_KEEP) {
            mem[2 * ord][tid] = median_key(c);
            mem[2 * ord + 1][tid] = w;
        }
        count = ord + 1;
    });
    const bool agree = T == 0 || (hi[0] - lo[0] <= tol && hi[1] - lo[1] <= tol && hi[2] - lo[2] <= tol);
    if (!agree) {
        uint64_t S = 0, last = 0;
        bool has_last = false;
        int j = -1;
        if (count <= MED_KEEP) {
            j = median_consume<false>(mem, tid, count, T, S, last, has_last);
        } else {
            for (int pass = 0; j < 0 && pass * MED_OVER < count; ++pass) {
                int held = 0, top_at = 0;
                uint64_t top = 0;
                sm.walk(0, MED_ALL, [&](int ord, const float *c, float a) {
                    const uint32_t w = median_weight(a);
                    const uint64_t pair = ((uint64_t)median_key(c) << 32) | (uint32_t)ord;
                    if (w == 0 || (has_last && pair <= last)) return;
                    int at;
                    if (held < MED_OVER) {
                        at = held++;
                    } else if (pair < top) {
                        at = top_at;                       // the largest one held makes room
                    } else {
                        return;
                    }
                    mem[3 * at][tid] = (uint32_t)(pair >> 32);
                    mem[3 * at + 1][tid] = (uint32_t)ord;
                    mem[3 * at + 2][tid] = w;
                    if (held < MED_OVER) return;           // (the largest matters once all are taken)
                    top = 0;
                    for (int e = 0; e < MED_OVER; ++e) {
                        const uint64_t p = ((uint64_t)mem[3 * e][tid] << 32) | mem[3 * e + 1][tid];
                        if (p >= top) {
                            top = p;
                            top_at = e;
                        }
                    }
                });
                if (held == 0) break;
                j = median_consume<true>(mem, tid, held, T, S, last, has_last);
            }
        }
        if (j >= 0) {                                      // (always: the weights above 0 add up to T)
            float cj[3] = {0.0f, 0.0f, 0.0f};
            sm.walk(j, j, [&](int, const float *c, float) {
                cj[0] = c[0];
                cj[1] = c[1];
                cj[2] = c[2];
            });
            acc[0] = acc[1] = acc[2] = wsum = 0.0f;
            sm.walk(0, MED_ALL, [&](int, const float *c, float a) {
                if (!(fabsf(c[0] - cj[0]) <= tol && fabsf(c[1] - cj[1]) <= tol &&
                      fabsf(c[2] - cj[2]) <= tol))
                    return;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + c[ch] * a;
                wsum = wsum + a;
            });
        }
    }
    const float ws = wsum == 0.0f ? 1.0f : wsum;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)(int)(255.0f * __fdiv_rn(acc[ch], ws));
    return count > 0;
}

// The samples of whole-patch planes: where the patch covers the pixel and its mask is 0.
struct PatchSampler {
    const pano_patch *patches;
    int n, x, y;

    template <class Visit>
    __device__ __forceinline__ void walk(int lo, int hi, Visit visit) const {
        int ord = 0;
        for (int i = 0; i < n; ++i) {
            const pano_patch *p = patches + i;
            const int px = x - p->x0, py = y - p->y0;
            if ((unsigned)px >= (unsigned)p->w || (unsigned)py >= (unsigned)p->h) continue;
            if (p->mask[(size_t)py * p->w + px]) continue;
            const int at = ord++;
            if (at < lo) continue;
            const size_t plane = (size_t)p->vh * p->vpitch, o = (size_t)py * p->vpitch + px;
            const float rgb[3] = {p->planes[o], p->planes[plane + o], p->planes[2 * plane + o]};
            visit(at, rgb, p->planes[3 * plane + o]);
            if (at >= hi) break;
        }
    }
};
