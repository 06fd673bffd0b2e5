// gspl_reduce.h — the fixed-order sums of a wave and of a workgroup (device).  The association is part of the contract: the error
// bounds of tests/test_spotless.py and tests/test_normals_gpu.py are derived from it.
// (gspl_device.h's DPP sums, row_sum / wave_sum_to_lane63, belong to the compositing kernels; mcmc.hip's block_sum2 is an LDS tree.)
#pragma once
#include <hip/hip_runtime.h>

namespace gspl {

// xor butterfly over the 64 lanes, distances 32, 16, ... 1: every lane gets the sum (float, int, double)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The sum of a workgroup of NT threads: each wave by wave_sum, then the waves left to right, (sh[0] + sh[1]) + sh[2] + ..., by thread 0,
// which alone gets the sum (the others get 0).  sh: NT / 64 slots of LDS.  The first barrier publishes the slots to thread 0; the
// second keeps the next writer out of them until thread 0 has read, so that calls in a row may share sh.
template <int NT, class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    static_assert(NT % 64 == 0, "whole waves");
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = 0;
    if (threadIdx.x == 0) {
        s = sh[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) s += sh[w];
    }
    __syncthreads();
    return s;
}

}  // namespace gspl
