// vigo_dilate_bits.hpp — box dilation of a bit plane (z fastest, 32 voxels per word: the snapshot's plane format), one
// output word per thread: along z with shifts and carries between neighbouring words, along y and x by OR-ing whole
// words.  The one copy of the rule: vigo_inflate_grid (vigo_map.hip) runs it on a plane of the whole grid,
// vigo_update_grid_region (vigo_grid_update.hip) on the compact plane of a window; the word functions compile for the
// host too (tests/grid_update_check.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef VIGO_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_HD __host__ __device__ __forceinline__
#else
#define VIGO_HD inline
#endif
#endif

namespace vigo {

// z: out word = OR over |d| <= r of the row shifted by d bits (r <= 31: one neighbour word each side)
VIGO_HD uint32_t dilate_bits_z_word(int nz, int nzw, int r, const uint32_t* in, size_t wi) {
    const int w = (int)(wi % nzw);
    const uint64_t lo = w > 0 ? in[wi - 1] : 0u, mid = in[wi], hi = w + 1 < nzw ? in[wi + 1] : 0u;
    uint32_t acc = (uint32_t)mid;
    for (int d = 1; d <= r; ++d) {
        acc |= (uint32_t)(((mid << 32 | lo) >> (32 - d)) & 0xffffffffu);   // voxels z - d land on z
        acc |= (uint32_t)(((hi << 32 | mid) >> d) & 0xffffffffu);          // voxels z + d land on z
    }
    const int valid = nz - 32 * w;                                          // bits past nz stay clear
    if (valid < 32) acc &= (1u << valid) - 1u;
    return acc;
}
// y (stride nzw words, length ny) or x (stride ny * nzw, length nx): OR of whole words
VIGO_HD uint32_t dilate_bits_rows_word(size_t stride, int len, int r, const uint32_t* in, size_t wi) {
    const int c = (int)((wi / stride) % (size_t)len);
    const int lo = c - r < 0 ? -c : -r, hi = c + r >= len ? len - 1 - c : r;
    uint32_t acc = 0;
    for (int d = lo; d <= hi; ++d) acc |= in[(ptrdiff_t)wi + (ptrdiff_t)d * (ptrdiff_t)stride];
    return acc;
}

#if defined(__HIPCC__)
namespace {
__global__ void k_dilate_bits_z(int nz, int nzw, size_t n_words, int r, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    out[wi] = dilate_bits_z_word(nz, nzw, r, in, wi);
}
__global__ void k_dilate_bits_rows(size_t n_words, size_t stride, int len, int r, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    out[wi] = dilate_bits_rows_word(stride, len, r, in, wi);
}
}  // namespace
#endif

}  // namespace vigo
