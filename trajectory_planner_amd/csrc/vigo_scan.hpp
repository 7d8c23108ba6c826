// vigo_scan.hpp — what the one-workgroup kernels (1024 threads over the whole batch) share: the slice of the batch a
// thread owns and the inclusive scan of the per-thread counts.
#pragma once

#include <hip/hip_runtime.h>

namespace vigo {

// trajectories [lo, hi) of a batch of B are thread threadIdx.x's: ceil(B / 1024) each, in ascending order
struct BatchSlice {
    int lo, hi;
};
__device__ __forceinline__ BatchSlice batch_slice(int B) {
    const int per = (B + 1023) / 1024;
    const int lo = min(B, (int)threadIdx.x * per);
    return {lo, min(B, lo + per)};
}

// inclusive scan of v over the 1024 threads of the workgroup (s: 1024 elements of LDS); returns this thread's inclusive
// value, *total the sum.  Opens with a barrier: every thread of the workgroup has to arrive.
template <class T>
__device__ __forceinline__ T scan1024(T* s, T v, T* total) {
    const int tid = threadIdx.x;
    __syncthreads();                                      // (the previous scan's readers are done)
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const T u = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += u;
        __syncthreads();
    }
    *total = s[1023];
    return s[tid];
}

}  // namespace vigo
