// vigo_esdf_build.hip — vigo_build_esdf: the signed Euclidean distance field of the voxel snapshot, built on the device
// from the packed planes that are already resident (gfx950).  The rule — the sets, the signed int32 per voxel that
// carries both squared distances, the exact outward scan, the sentinel — is vigo_esdf_core.hpp; this file is its three
// launches, one thread per voxel each, z fastest across the lanes so that every global access of a wave is one
// contiguous run of the row (256 B at nz >= 64):
//
//   k_esdf_z            the 1-D squared distance along z from the packed words (clz / ctz; a row's words are read by
//                       all of its lanes: one broadcast line from L1), written as int32
//   k_esdf_line<false>  along y: out[i] = min_j (in[j] + (i - j)^2), element j of a lane's line nz ints further on
//   k_esdf_line<true>   along x (ny * nz ints further on), and the output value written as the row-major float lattice
//
// The scans read global memory directly.  A wave's 64 lanes walk 64 neighbouring lines in step and the waves of
// neighbouring voxels re-read the same lines, so the reads are L1 / L2 hits and HBM sees each buffer about once per
// pass; staging a line tile in LDS would add a second route (a 512-long line of 64 lanes is 128 KiB) for reads the
// caches already serve.  There is ONE route for every shape.
//
// Workspace: two int32 buffers of nx * ny * nz (8 bytes per voxel); the float lattice reuses the first when the caller
// wants none.  It belongs to the handle (vigo_api.cpp: vigo_build_esdf grows it, vigo_destroy frees it).
#include "vigo_esdf_core.hpp"
#include "vigo_internal.hpp"

namespace vigo {
namespace {

constexpr int kEsdfBlock = 256;

__global__ void __launch_bounds__(kEsdfBlock) k_esdf_z(int nz, int nzw, size_t total, int32_t E, const uint32_t* __restrict__ site_plane,
                                                       const uint32_t* __restrict__ unk_plane, int32_t* __restrict__ out) {
    const size_t v = (size_t)blockIdx.x * kEsdfBlock + threadIdx.x;
    if (v >= total) return;
    const size_t row = v / (size_t)nz;
    const int z = (int)(v - row * (size_t)nz);
    const uint32_t* sp = site_plane + row * nzw;
    const uint32_t* up = unk_plane ? unk_plane + row * nzw : nullptr;
    out[v] = esdf_z_value([sp, up](int w) { return up ? (sp[w] | up[w]) : sp[w]; }, nz, nzw, z, E);
}

// element v lies at position i = (v / stride) % n of its line; element j of that line is (j - i) * stride ints away
template <bool kCompose>
__global__ void __launch_bounds__(kEsdfBlock) k_esdf_line(size_t total, size_t stride, int n, const int32_t* __restrict__ in,
                                                          int32_t* __restrict__ out, float* __restrict__ lattice, double res) {
    const size_t v = (size_t)blockIdx.x * kEsdfBlock + threadIdx.x;
    if (v >= total) return;
    const int i = (int)((v / stride) % (size_t)n);
    const int32_t* line = in + (v - (size_t)i * stride);
    const int32_t s = esdf_line_value([line, stride](int j) { return line[(size_t)j * stride]; }, n, i);
    if (kCompose) lattice[v] = esdf_compose(s, res);
    else out[v] = s;
}

}  // namespace

size_t esdf_build_ws_bytes(int nx, int ny, int nz) { return 2 * (size_t)nx * ny * nz * sizeof(int32_t); }

int launch_esdf_build(hipStream_t s, const GridView& g, int plane, int unknown_is_site, int32_t* a, int32_t* b, float* lattice) {
    const int32_t E = esdf_empty_d2(g.nx, g.ny, g.nz);
    if (E == 0) return (int)hipErrorInvalidValue;
    const size_t total = (size_t)g.nx * g.ny * g.nz;
    const dim3 grid((unsigned)((total + kEsdfBlock - 1) / kEsdfBlock)), block(kEsdfBlock);
    const uint32_t* unk = unknown_is_site ? g.planes + g.plane_words : nullptr;
    hipLaunchKernelGGL(k_esdf_z, grid, block, 0, s, g.nz, g.nzw, total, E, g.planes + (size_t)plane * g.plane_words, unk, a);
    hipLaunchKernelGGL(k_esdf_line<false>, grid, block, 0, s, total, (size_t)g.nz, g.ny, a, b, (float*)nullptr, g.res);
    // (the lattice may be the first buffer: the last pass reads the second only)
    hipLaunchKernelGGL(k_esdf_line<true>, grid, block, 0, s, total, (size_t)g.ny * g.nz, g.nx, b, (int32_t*)nullptr, lattice, g.res);
    return (int)hipGetLastError();
}

}  // namespace vigo
