// Fixed-order fp64 reductions: no floating-point atomics, so the same input gives the same bits in every run.  Inside a wave the xor
// butterfly 32, 16, ..., 1 (every lane ends with the same total), the waves of a block in order through LDS, the blocks of a grid in an order
// fixed by their number.
#pragma once
#include <stdint.h>

namespace bs {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// sums of K values over a block of WAVES waves: on return every thread holds the same totals, added in the same order (the butterfly inside
// a wave, then the waves in order).  lds: WAVES * K doubles; the leading barrier lets a caller reuse it from one call to the next.
template <int K, int WAVES>
__device__ __forceinline__ void block_sum(double (&v)[K], double* lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], d, 64);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) lds[w * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double a = lds[k];
#pragma unroll
        for (int i = 1; i < WAVES; ++i) a += lds[i * K + k];
        v[k] = a;
    }
}

// column k of partial [nblocks, stride] by one wave: lane l adds rows l, l + 64, ... in order, then the butterfly.  nblocks = 0 gives +0.
__device__ __forceinline__ double column_sum(const double* __restrict__ partial, int nblocks, int stride, int k, int lane) {
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += partial[(int64_t)b * stride + k];
    return wave_sum(s);
}

}  // namespace bs
