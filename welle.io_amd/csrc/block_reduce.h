// welle.io_amd/csrc/block_reduce.h -- one value per thread of a work-group of FFT_THREADS threads -> one result in every thread.
#pragma once
#include "dabphy_common.h"

namespace dabphy {

// Tree reduction of one value per thread; every thread gets the result.  op is associative and commutative (max, min), so the result
// does not depend on the tree's order.  red: FFT_THREADS values of LDS.
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T x, T* red, int t, Op op)
{
    __syncthreads();
    red[t] = x;
    __syncthreads();
    for (int s = FFT_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = op(red[t], red[t + s]);
        __syncthreads();
    }
    const T r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_max(float x, float* red, int t) { return block_reduce(x, red, t, [](float a, float b) { return fmaxf(a, b); }); }
__device__ __forceinline__ int block_min_int(int x, int* red, int t) { return block_reduce(x, red, t, [](int a, int b) { return a < b ? a : b; }); }

} // namespace dabphy
