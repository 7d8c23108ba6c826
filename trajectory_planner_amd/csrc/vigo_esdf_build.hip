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
//
// vigo_update_esdf (launch_esdf_region_update): after a box of the snapshot changed, the same three passes on the lines
// the change reaches, on the A, B and lattice a tracked build kept — flags, not lists, say which lines (the rule and its
// per-thread functions: vigo_esdf_core.hpp, "Region update") — and the bricked field's values on those lines rewritten:
//
//   k_esdf_region_z      box footprint x nz threads; a value that differs from A is stored and flags its y line
//   k_esdf_region_y      box slab x ny x nz threads; flagged lines only; a value that differs from B flags its x line
//   k_esdf_region_x      the whole lattice; flagged lines only, the output value into the lattice
//   k_esdf_region_brick  the whole bricked field; the values whose source is on a flagged x line
//
// The count of flagged lines is known to the device only, so the last two launch over everything and unflagged waves
// leave at once: no host round trip, the same one route.
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

// the region update: one region function of vigo_esdf_core.hpp per thread; t runs z fastest in all four, so a wave's
// flag bytes, values and stores are consecutive along z, and a wave whose lanes are all unflagged leaves after one load
__global__ void __launch_bounds__(kEsdfRegionBlock) k_esdf_region_z(EsdfRegion r, const uint32_t* __restrict__ site_plane,
                                                                    const uint32_t* __restrict__ unk_plane, int32_t* __restrict__ a,
                                                                    uint8_t* __restrict__ fy) {
    esdf_region_z(r, (size_t)blockIdx.x * kEsdfRegionBlock + threadIdx.x, site_plane, unk_plane, a, fy);
}
__global__ void __launch_bounds__(kEsdfRegionBlock) k_esdf_region_y(EsdfRegion r, const int32_t* __restrict__ a, int32_t* __restrict__ b,
                                                                    const uint8_t* __restrict__ fy, uint8_t* __restrict__ fx) {
    esdf_region_y(r, (size_t)blockIdx.x * kEsdfRegionBlock + threadIdx.x, a, b, fy, fx);
}
__global__ void __launch_bounds__(kEsdfRegionBlock) k_esdf_region_x(EsdfRegion r, const int32_t* __restrict__ b, float* __restrict__ lattice,
                                                                    const uint8_t* __restrict__ fx, double res) {
    esdf_region_x(r, (size_t)blockIdx.x * kEsdfRegionBlock + threadIdx.x, b, lattice, fx, res);
}
__global__ void __launch_bounds__(kEsdfRegionBlock) k_esdf_region_brick(EsdfRegion r, int nby, int nbz, const uint8_t* __restrict__ fx,
                                                                        const float* __restrict__ lattice, float* __restrict__ bricked) {
    esdf_region_brick(r, (size_t)blockIdx.x * kEsdfRegionBlock + threadIdx.x, nby, nbz, fx, lattice, bricked);
}
// the set flags among n, added to *count: one ballot and one atomic add per wave (only when the caller asked for stats)
__global__ void __launch_bounds__(kEsdfRegionBlock) k_esdf_flag_count(const uint8_t* __restrict__ flags, size_t n, unsigned long long* count) {
    const size_t t = (size_t)blockIdx.x * kEsdfRegionBlock + threadIdx.x;
    const unsigned long long set = __ballot(t < n && flags[t] != 0);
    if ((threadIdx.x & 63) == 0 && set) atomicAdd(count, (unsigned long long)__popcll(set));
}

}  // namespace

int launch_esdf_region_update(hipStream_t s, const GridView& g, const int32_t lo[3], const int32_t n[3], int plane, int unknown_is_site,
                              const EsdfTrackWs& w, float* bricked, bool count) {
    const EsdfRegion r = esdf_region(g.nx, g.ny, g.nz, lo, n);
    if (r.E == 0) return (int)hipErrorInvalidValue;
    const size_t n_fy = (size_t)n[0] * g.nz, n_fx = (size_t)g.ny * g.nz;
    const hipError_t e = hipMemsetAsync(w.counters, 0, w.clear_bytes, s);   // the counts and both flag arrays, ahead of the passes
    if (e != hipSuccess) return (int)e;
    const dim3 block(kEsdfRegionBlock);
    const auto grid = [](size_t threads) { return dim3((unsigned)esdf_region_grid(threads)); };
    const uint32_t* unk = unknown_is_site ? g.planes + g.plane_words : nullptr;
    hipLaunchKernelGGL(k_esdf_region_z, grid(esdf_region_z_threads(r)), block, 0, s, r, g.planes + (size_t)plane * g.plane_words, unk, w.a, w.fy);
    hipLaunchKernelGGL(k_esdf_region_y, grid(esdf_region_y_threads(r)), block, 0, s, r, w.a, w.b, w.fy, w.fx);
    hipLaunchKernelGGL(k_esdf_region_x, grid(esdf_region_x_threads(r)), block, 0, s, r, w.b, w.lattice, w.fx, g.res);
    hipLaunchKernelGGL(k_esdf_region_brick, grid(esdf_bricked_floats(g.nx, g.ny, g.nz)), block, 0, s, r, esdf_bricks_along(g.ny),
                       esdf_bricks_along(g.nz), w.fx, w.lattice, bricked);
    if (count) {
        hipLaunchKernelGGL(k_esdf_flag_count, grid(n_fy), block, 0, s, w.fy, n_fy, w.counters);
        hipLaunchKernelGGL(k_esdf_flag_count, grid(n_fx), block, 0, s, w.fx, n_fx, w.counters + 1);
    }
    return (int)hipGetLastError();
}

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
