// The two pyramid filters of cv2.pyrDown / cv2.pyrUp as expressions over one sample type
// (laplacian.hip: float and double planes; fuse.hip: pixels of three or four floats): OpenCV's
// published float path as the oracle restates it, one rounding per operation in the order written.
#pragma once
#include "common.h"

// One pass of pyrDown over the five neighbouring samples a0 .. a4 (a2 the centre):
// c*6 + (l1 + r1)*4 + l2 + r2, left to right; the caller scales by 1/256 after the second pass.
template <class T>
__device__ __forceinline__ T pyr_down_taps(T a0, T a1, T a2, T a3, T a4) {
    return a2 * (T)6 + (a1 + a3) * (T)4 + a0 + a4;
}

// Horizontal pass of pyrUp at output column dx of a source row of n samples, s(i) sample i:
// even dx: s[i-1] + s[i]*6 + s[i+1], odd: (s[i] + s[i+1])*4, with s[-1] := s[1] and
// s[n] := s[n-1] written the way OpenCV's pyrUp_ writes its two edge columns.
template <class T, class At>
__device__ __forceinline__ T pyr_up_row(At s, int n, int dx) {
    const int i = dx >> 1;
    if (dx & 1) {
        if (i == n - 1) return s(i) * (T)8;
        return (s(i) + s(i + 1)) * (T)4;
    }
    if (i == 0) return s(0) * (T)6 + s(1) * (T)2;
    if (i == n - 1) return s(i - 1) + s(i) * (T)7;
    return s(i - 1) + s(i) * (T)6 + s(i + 1);
}

// Vertical pass of pyrUp at an odd / even output row from the row passes v0, v1, v2 of the source
// rows above, at and below (border rows: 1 above the first, the last below the last), and the
// final scale.
template <class T>
__device__ __forceinline__ T pyr_up_col_odd(T v1, T v2) { return ((v1 + v2) * (T)4) * (T)(1.0 / 64.0); }
template <class T>
__device__ __forceinline__ T pyr_up_col_even(T v0, T v1, T v2) { return (v0 + v1 * (T)6 + v2) * (T)(1.0 / 64.0); }
