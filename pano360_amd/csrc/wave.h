// Wave and workgroup primitives of the kernels (gfx950: 64 lanes), and the one kernel that is
// nothing but one of them.  All are for one-dimensional workgroups of whole waves (block_sum_fixed
// also for 64 x 4), every lane active at the call.  (The min / max / key reductions of blend.hip,
// own_tile.inc and crop.hip are interleaved with other work and stay where they are; so do sums
// over fewer lanes or in another order: blur_mfma.hip's 16-lane prefix, msop.hip's sum64.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The sum of v over the wave, in every lane.  The butterfly pairs lane ^ 32, then ^ 16 ... ^ 1:
// a floating-point sum has that one fixed order, the same in all lanes.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The sums of N accumulators over a workgroup of 256 threads, one-dimensional or 64 x 4 (the
// caller says which lane of which wave it is), in ONE fixed order - what makes the statistics of
// gains.hip and photo.hip return the same bytes on every call: wave_sum of each accumulator, the
// four waves' values through r (LDS of the caller's, one barrier), and thread k < N returns
// (r[0][k] + r[1][k]) + (r[2][k] + r[3][k]); the other threads return 0.  Every addition is in the
// order those kernels wrote out themselves before they shared this: another order, other bytes.
template <int N>
__device__ __forceinline__ double block_sum_fixed(double (&acc)[N], double (*r)[N], int lane,
                                                  int wave) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) r[wave][k] = acc[k];
    __syncthreads();
    const int k = wave * 64 + lane;
    return k < N ? (r[0][k] + r[1][k]) + (r[2][k] + r[3][k]) : 0.0;
}

// block_sum_fixed of a pair's nblk partial sums (N doubles each, from src on): thread t adds
// the partials t, t + 256, ... in that order.  One-dimensional workgroups of 256 threads.
template <int N>
__device__ __forceinline__ double block_sum_partials(const double *__restrict__ src, int nblk,
                                                     double (*r)[N]) {
    double acc[N] = {};
    for (int b = threadIdx.x; b < nblk; b += 256)
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += src[(size_t)b * N + k];
    return block_sum_fixed<N>(acc, r, threadIdx.x & 63, threadIdx.x >> 6);
}

// Lane k's result: the sum of v over lanes 0 .. k.
template <class T>
__device__ __forceinline__ T wave_scan_inclusive(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

// Thread t's result: the sum of v over threads 0 .. t - 1 of a workgroup of BLOCK threads, and
// `total` the sum over all of them.  For integers (the order of the additions is not fixed).
// lds: BLOCK / 64 values of the caller's, free again when the call returns (three barriers).
template <int BLOCK, class T>
__device__ __forceinline__ T block_scan_exclusive(T v, T *lds, T &total) {
    static_assert(BLOCK % 64 == 0 && BLOCK <= 64 * 64, "whole waves, and one wave scans their sums");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T x = wave_scan_inclusive(v);
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (wave == 0) {
        const T s = wave_scan_inclusive(lane < BLOCK / 64 ? lds[lane] : T(0));
        if (lane < BLOCK / 64) lds[lane] = s;
    }
    __syncthreads();
    total = lds[BLOCK / 64 - 1];
    const T excl = x - v + (wave ? lds[wave - 1] : T(0));
    __syncthreads();
    return excl;
}

// out[i] = in[0] + ... + in[i - 1] for i = 0 .. n, so out[n] is the total: one workgroup of BLOCK
// threads that walks the values BLOCK at a time.  `in` may be `out` (T = int64_t).
template <int BLOCK, class T>
__global__ __launch_bounds__(BLOCK) void scan_exclusive_kernel(const T *in, int64_t n, int64_t *out) {
    __shared__ int64_t waves[BLOCK / 64];
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += BLOCK) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < n ? (int64_t)in[i] : 0;
        int64_t total;
        const int64_t excl = block_scan_exclusive<BLOCK>(v, waves, total);
        if (i < n) out[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) out[n] = carry;
}
