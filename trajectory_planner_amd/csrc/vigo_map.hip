// vigo_map.hip — the map kernels: voxel snapshot packing and inflation, point queries, B-spline evaluation, the two
// gates as entry points of their own (hasCollisionTrajectory, hasDynamicCollisionTrajectory: the walks of vigo_grid.hpp,
// which the rebound loop's k_rebound_decide in vigo_reguide.hip runs too) and the map queries of findCollisionSeg
// (k_ctrl_occupancy: the point flags, and the interior line walk of vigo_pathsearch_core.hpp between two free ends).
// All HBM-bound byte/bit work: coalesced reads, one bit per voxel per plane so a 256^3 plane is 2 MiB (L2-resident per
// XCD) and a 512^3 plane 16 MiB (MALL).
//
// The gates look each sample up directly in the packed planes (L2 hits): a trajectory makes
// ~120-240 lookups scattered over a 7 m path, fewer words than staging its bounding volume in
// LDS would read.  The LDS-tiled path is the corridor checker (vigo_corridor_core.hpp), where one
// segment makes ~10^5 lookups inside a small volume.
#include "vigo_dilate_bits.hpp"
#include "vigo_exact_time.hpp"
#include "vigo_grid.hpp"
#include "vigo_pathsearch_core.hpp"

namespace vigo {
namespace {

// one thread per output word triple: reads 32 voxels along z, writes one word per plane
__global__ void k_pack_grid(int nx, int ny, int nz, int nzw, const uint8_t* __restrict__ vox,
                            uint32_t* __restrict__ packed) {
    const size_t plane_words = (size_t)nx * ny * nzw;
    const size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= plane_words) return;
    const size_t col = wi / nzw;
    const int w = (int)(wi % nzw);
    const uint8_t* src = vox + col * nz + (size_t)w * 32;
    const int cnt = min(32, nz - w * 32);
    uint32_t b0 = 0, b1 = 0, b2 = 0;
    if (cnt == 32 && ((reinterpret_cast<uintptr_t>(src) & 15) == 0)) {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4 q[2] = {s4[0], s4[1]};
        const uint32_t* wds = reinterpret_cast<const uint32_t*>(q);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t v = (wds[i] >> (8 * j)) & 0xFFu;
                const int bit = 4 * i + j;
                b0 |= (v & 1u) << bit;
                b1 |= ((v >> 1) & 1u) << bit;
                b2 |= ((v >> 2) & 1u) << bit;
            }
        }
    } else {
        for (int i = 0; i < cnt; ++i) {
            const uint32_t v = src[i];
            b0 |= (v & 1u) << i;
            b1 |= ((v >> 1) & 1u) << i;
            b2 |= ((v >> 2) & 1u) << i;
        }
    }
    packed[wi] = b0;
    packed[plane_words + wi] = b1;
    packed[2 * plane_words + wi] = b2;
}

// ---- inflation on bit planes -----------------------------------------------------------------
// bit0 of the byte grid := box dilation of bit2 (map_manager inflates the occupied voxels by the robot
// size).  The occupied bit is packed to one bit per voxel (z fastest, 32 voxels per
// word — the snapshot's plane format), dilated there — along z with shifts and carries between
// neighbouring words, along y and x by OR-ing whole words — and merged back: 3 bytes of HBM traffic
// per voxel instead of 2 per voxel and pass (a 256^3 plane is 2 MiB: the three dilation passes never
// leave the L2).
__global__ void k_pack_bit(int nz, int nzw, size_t n_words, int bit, const uint8_t* __restrict__ vox, uint32_t* __restrict__ plane) {
    const size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    const size_t col = wi / nzw;
    const int w = (int)(wi % nzw);
    const uint8_t* src = vox + col * nz + (size_t)w * 32;
    const int cnt = min(32, nz - w * 32);
    uint32_t b = 0;
    if (cnt == 32 && ((reinterpret_cast<uintptr_t>(src) & 15) == 0)) {   // 32 voxels = two 16-byte loads
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        const uint4 q[2] = {s4[0], s4[1]};
        const uint32_t* wds = reinterpret_cast<const uint32_t*>(q);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) b |= ((wds[i] >> (8 * j + bit)) & 1u) << (4 * i + j);
    } else {
        for (int i = 0; i < cnt; ++i) b |= (uint32_t)((src[i] >> bit) & 1u) << i;
    }
    plane[wi] = b;
}
// (the dilation kernels k_dilate_bits_z / k_dilate_bits_rows: vigo_dilate_bits.hpp, shared with vigo_grid_update.hip)
// one plane word (32 voxels) per thread: bit0 of the 32 bytes from the word's bits
__global__ void k_merge_bit0(int nz, int nzw, size_t n_words, const uint32_t* __restrict__ plane, uint8_t* __restrict__ vox) {
    const size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (wi >= n_words) return;
    const size_t col = wi / nzw;
    const int w = (int)(wi % nzw);
    uint8_t* dst = vox + col * nz + (size_t)w * 32;
    const int cnt = min(32, nz - w * 32);
    const uint32_t bits = plane[wi];
    if (cnt == 32 && ((reinterpret_cast<uintptr_t>(dst) & 15) == 0)) {
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        uint4 q[2] = {d4[0], d4[1]};
        uint32_t* wds = reinterpret_cast<uint32_t*>(q);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t nib = (bits >> (4 * i)) & 0xFu;
            const uint32_t spread = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);   // one bit per byte
            wds[i] = (wds[i] & 0xFEFEFEFEu) | spread;
        }
        d4[0] = q[0];
        d4[1] = q[1];
    } else {
        for (int i = 0; i < cnt; ++i) dst[i] = (uint8_t)((dst[i] & ~1u) | ((bits >> i) & 1u));
    }
}

// CSR offsets off[n]: off[0] == 0, non-decreasing, off[n-1] <= total; every violation is counted
__global__ void k_check_offsets(const int32_t* __restrict__ off, int64_t n, int64_t total, int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t v = off[i];
    bool wrong = v < 0 || (int64_t)v > total;
    if (i == 0) wrong = wrong || v != 0;
    else wrong = wrong || v < off[i - 1];
    if (wrong) atomicAdd(bad, 1);
}

__global__ void k_query_points(GridView g, int plane, int64_t Q, const double* __restrict__ pts,
                               int stride, uint8_t* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const double* p = pts + q * stride;
    out[q] = (uint8_t)grid_plane_pos(g, plane, p[0], p[1], p[2]);
}

// grid: (ceil(T/256), B)
__global__ void k_bspline_eval(int B, int N, const double* __restrict__ ctrl, double ts, int deriv,
                               int T, const double* __restrict__ times, double* __restrict__ out) {
    const int b = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= T) return;
    double p[3];
    traj_eval(ctrl + (size_t)b * N * 3, N, ts, deriv, times[k], p);
    double* dst = out + ((size_t)b * T + k) * 3;
    dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
}

// one 64-lane wave per trajectory; lanes stride over the samples; first hit = wave min
// t_k of the reference's sample loop `for (t = 0; t <= tmax; t += dt)` (BT.h:313, :347), k = 0 .. T-1, by the
// closed form of vigo_exact_time.hpp — filled once per (dt, tmax) and cached in the handle
__global__ void k_fill_sample_times(double dt, int T, double* __restrict__ times) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < T) times[k] = accumulated_time(dt, k);
}

__global__ void __launch_bounds__(64) k_traj_collision(GridView g, int B, int N, const double* __restrict__ ctrl,
                                                       double ts, int T, const double* __restrict__ times,
                                                       uint8_t* __restrict__ out_flag, int32_t* __restrict__ out_first) {
    const int b = blockIdx.x;
    if (b >= B) return;
    int first = gate_static_first(g, ctrl + (size_t)b * N * 3, N, ts, T, times, threadIdx.x);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) first = min(first, __shfl_xor(first, m, 64));
    if (threadIdx.x == 0) {
        out_flag[b] = first != INT_MAX;
        if (out_first) out_first[b] = first != INT_MAX ? first : -1;
    }
}

__global__ void __launch_bounds__(64) k_traj_dynamic_collision(int B, int N, const double* __restrict__ ctrl, double ts,
                                                               int T, const double* __restrict__ times,
                                                               const int32_t* __restrict__ obs_off,
                                                               const double* __restrict__ obs, int n_obs_shared,
                                                               uint8_t* __restrict__ out_flag) {
    const int b = blockIdx.x;
    if (b >= B) return;
    int hit = gate_dynamic_hit(ctrl + (size_t)b * N * 3, N, ts, T, times, obs_off, obs, n_obs_shared, b, threadIdx.x);
    hit = __any(hit);
    if (threadIdx.x == 0) out_flag[b] = (uint8_t)(hit != 0);
}

// one thread per control point: point flag and the line (i-1, i) flag
__global__ void k_ctrl_occupancy(GridView g, int B, int N, const double* __restrict__ ctrl,
                                 uint8_t* __restrict__ out_pt, uint8_t* __restrict__ out_line) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)B * N) return;
    const int i = (int)(idx % N);
    const double* p = ctrl + idx * 3;
    const unsigned occ = grid_plane_pos(g, 0, p[0], p[1], p[2]);
    out_pt[idx] = (uint8_t)occ;
    unsigned line = 0;
    if (i > 0) {
        const double* q = p - 3;  // previous control point
        line = grid_plane_pos(g, 0, q[0], q[1], q[2]) | occ;
        if (!line) line = line_interior_occupied(GridOcc{g}, g.res, q, p) ? 1u : 0u;
    }
    out_line[idx] = (uint8_t)line;
}

}  // namespace

int launch_pack_grid(hipStream_t s, int nx, int ny, int nz, const uint8_t* vox, uint32_t* packed) {
    const int nzw = (nz + 31) / 32;
    const size_t words = (size_t)nx * ny * nzw;
    const int block = 256;
    const size_t grid = (words + block - 1) / block;
    hipLaunchKernelGGL(k_pack_grid, dim3((unsigned)grid), dim3(block), 0, s, nx, ny, nz, nzw, vox, packed);
    return (int)hipGetLastError();
}

int launch_inflate(hipStream_t s, int nx, int ny, int nz, uint8_t* vox, uint32_t* planeA, uint32_t* planeB, int rx, int ry, int rz) {
    const int nzw = (nz + 31) / 32;
    const size_t nw = (size_t)nx * ny * nzw;
    const unsigned gw = (unsigned)((nw + 255) / 256);
    hipLaunchKernelGGL(k_pack_bit, dim3(gw), dim3(256), 0, s, nz, nzw, nw, 2, vox, planeA);
    hipLaunchKernelGGL(k_dilate_bits_z, dim3(gw), dim3(256), 0, s, nz, nzw, nw, rz, planeA, planeB);
    hipLaunchKernelGGL(k_dilate_bits_rows, dim3(gw), dim3(256), 0, s, nw, (size_t)nzw, ny, ry, planeB, planeA);
    hipLaunchKernelGGL(k_dilate_bits_rows, dim3(gw), dim3(256), 0, s, nw, (size_t)ny * nzw, nx, rx, planeA, planeB);
    hipLaunchKernelGGL(k_merge_bit0, dim3(gw), dim3(256), 0, s, nz, nzw, nw, planeB, vox);
    return (int)hipGetLastError();
}

int launch_check_lists(hipStream_t s, int B, int N, const int32_t* guide_off, int64_t G, const int32_t* obs_off, int64_t O,
                       int* bad) {
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    const int block = 256;
    if (guide_off) {
        const int64_t n = (int64_t)B * N + 1;
        hipLaunchKernelGGL(k_check_offsets, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, s, guide_off, n, G, bad);
    }
    if (obs_off) {
        const int64_t n = (int64_t)B + 1;
        hipLaunchKernelGGL(k_check_offsets, dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, s, obs_off, n, O, bad);
    }
    return (int)hipGetLastError();
}

int launch_query_points(hipStream_t s, const GridView& g, int which, int64_t Q, const double* pts,
                        int pt_stride, uint8_t* out) {
    if (Q <= 0) return hipSuccess;
    const int block = 256;
    hipLaunchKernelGGL(k_query_points, dim3((unsigned)((Q + block - 1) / block)), dim3(block), 0, s, g, which, Q, pts,
                       pt_stride, out);
    return (int)hipGetLastError();
}

int launch_bspline_eval(hipStream_t s, int B, int N, const double* ctrl, double ts_ctrl, int deriv,
                        int T, const double* times, double* out) {
    if (B <= 0 || T <= 0) return hipSuccess;
    const int block = 64;
    // gridDim.y is limited to 65535: larger batches go out in slices of that many trajectories
    for (int b0 = 0; b0 < B; b0 += 65535) {
        const int nb = (B - b0) < 65535 ? (B - b0) : 65535;
        hipLaunchKernelGGL(k_bspline_eval, dim3((T + block - 1) / block, nb), dim3(block), 0, s, nb, N, ctrl + (size_t)b0 * N * 3,
                           ts_ctrl, deriv, T, times, out + (size_t)b0 * T * 3);
    }
    return (int)hipGetLastError();
}

int launch_traj_collision(hipStream_t s, const GridView& g, int B, int N, const double* ctrl,
                          double ts_ctrl, int T, const double* times, uint8_t* out_flag,
                          int32_t* out_first) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_traj_collision, dim3(B), dim3(64), 0, s, g, B, N, ctrl, ts_ctrl, T, times, out_flag, out_first);
    return (int)hipGetLastError();
}

int launch_traj_dynamic_collision(hipStream_t s, int B, int N, const double* ctrl, double ts_ctrl,
                                  int T, const double* times, const int32_t* obs_off,
                                  const double* obs, int n_obs_shared, uint8_t* out_flag) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_traj_dynamic_collision, dim3(B), dim3(64), 0, s, B, N, ctrl, ts_ctrl, T, times, obs_off, obs,
                       n_obs_shared, out_flag);
    return (int)hipGetLastError();
}

int launch_fill_sample_times(hipStream_t s, double dt, int T, double* times) {
    if (T <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fill_sample_times, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, dt, T, times);
    return (int)hipGetLastError();
}

int launch_ctrl_occupancy(hipStream_t s, const GridView& g, int B, int N, const double* ctrl,
                          uint8_t* out_pt, uint8_t* out_line) {
    const int64_t total = (int64_t)B * N;
    if (total <= 0) return hipSuccess;
    const int block = 256;
    hipLaunchKernelGGL(k_ctrl_occupancy, dim3((unsigned)((total + block - 1) / block)), dim3(block), 0, s, g, B, N,
                       ctrl, out_pt, out_line);
    return (int)hipGetLastError();
}

}  // namespace vigo
