// vigo_corridor.hip — the corridor checker's launchers and the kernels around it: the sampler alone (k_poly_sample), the
// box sweep of given poses (k_box_points), the trilinear ESDF query.  The checker itself, k_corridor, and its device
// helpers live in vigo_corridor_core.hpp; the whole-trajectory mode of vigo_traj_corridor_check in vigo_traj_corridor.hip.
#include "vigo_corridor_core.hpp"

namespace vigo {
namespace {

// ---- the sampler alone: polyTrajSolver::getTrajectory (PS.cpp:1125-1137) for S segments ---------------
// Same clock (accumulated_time + the reference's t += delT inside a chunk) and the same poly_pos / poly_pos7 as
// k_corridor, so a parity test of these positions is a parity test of what the checker sweeps.
__global__ void __launch_bounds__(kBlock) k_poly_sample(int S, int deg, const double* __restrict__ coeffs,
                                                        const int32_t* __restrict__ n_samp, const double* __restrict__ delT,
                                                        int stride, double* __restrict__ out_pos, float* __restrict__ out_f32) {
    __shared__ double cf[3 * (kMaxDeg + 1)];
    const int s = blockIdx.x;
    if (s >= S) return;
    const int tid = threadIdx.x;
    const int n = min(n_samp[s], stride);
    const double dT = delT[s];
    if (tid < 3 * (deg + 1)) {
        const int ax = tid / (deg + 1), d = tid % (deg + 1);
        cf[ax * (kMaxDeg + 1) + d] = coeffs[((size_t)s * 3 + ax) * (deg + 1) + d];
    }
    __syncthreads();
    double c7[3][8];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 8; ++d) c7[a][d] = deg == 7 ? cf[a * (kMaxDeg + 1) + d] : 0.0;
    // the float output takes the checker's own route (filtered fast form, sample_f32); the fp64 output is the
    // exact-power chain itself
    double E[3] = {0.0, 0.0, 0.0};
    if (n > 0) {
        const double tl = accumulated_time(dT, n - 1);
#pragma unroll
        for (int a = 0; a < 3; ++a) E[a] = sampler_error_bound(cf + a * (kMaxDeg + 1), deg, tl);
    }
    const int n_chunks = (n + kChunk - 1) / kChunk;
    for (int c = tid; c < n_chunks; c += kBlock) {
        const int k0 = c * kChunk, k1 = min(n, k0 + kChunk);
        double t = accumulated_time(dT, k0);
        for (int k = k0; k < k1; ++k) {
            const size_t o = ((size_t)s * stride + k) * 3;
            if (out_pos) {
                double p[3];
                if (deg == 7) poly_pos7(c7, t, p);
                else poly_pos(cf, deg, t, p);
                out_pos[o] = p[0]; out_pos[o + 1] = p[1]; out_pos[o + 2] = p[2];
            }
            if (out_f32) {
                float f[3];
                const bool ok = deg == 7 ? sample_f32_fast<true>(c7, cf, deg, t, E, f) : sample_f32_fast<false>(c7, cf, deg, t, E, f);
                if (!ok) sample_f32_exact(cf, deg, t, f);
                out_f32[o] = f[0]; out_f32[o + 1] = f[1]; out_f32[o + 2] = f[2];
            }
            t += dT;
        }
    }
}

// ---- box sweep at given sample positions (polyTrajOctomap::checkCollision per pose) -------------
// One thread per pose; lookups go to the packed planes (L2).  Serves the reference's
// checkCollisionTraj(trajectory, ...) signatures, where the samples already exist (PO.cpp:619-656).
__global__ void k_box_points(GridView g, int64_t M, const double* __restrict__ pts, SweepConst C, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    const float fx = (float)pts[3 * i], fy = (float)pts[3 * i + 1], fz = (float)pts[3 * i + 2];  // pose2Octomap
    const bool hit = box_sweep(g, C, fx, fy, fz, nullptr, nullptr);
    out[i] = (uint8_t)hit;
}

// ---- trilinear ESDF (own definition, see oracle/vigo_oracle.c vgo_esdf_query) ------------
// One query per lane (two or four per lane with all their corner loads in flight measured the same: the gather is
// bound by the lines it touches, not by latency).  The eight corners of a cell are one base address + constants.
__global__ void k_esdf_query(EsdfView E, int64_t Q, const double* __restrict__ pts,
                             double* __restrict__ out_d, double* __restrict__ out_g) {
    // Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one, each XCD has its own L2): block b
    // takes the tile (b % 8) * (tiles / 8) + b / 8, so that every XCD walks ONE contiguous eighth of the queries — for
    // spatially coherent queries its L2 then holds lattice lines no other XCD asks for.  (Uniformly random: no effect.)
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
    const unsigned base = nb >> 3, rem = nb & 7u;
    const unsigned tile = xcd * base + (xcd < rem ? xcd : rem) + idx;
    const int64_t q = (int64_t)tile * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int n[3] = {E.nx, E.ny, E.nz};
    int i0[3];
    double f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = (pts[q * 3 + a] - E.origin[a]) / E.res - 0.5;
        const double fl = floor(u);
        int i = (int)fl;
        double fr = u - fl;
        if (i < 0) { i = 0; fr = 0.0; }
        if (i > n[a] - 2) { i = n[a] - 2; fr = 1.0; }
        i0[a] = i;
        f[a] = fr;
    }
    // cell (x, y, z) reads line (x, y / 3, z / 3); its corners are 16 dx + 4 dy + dz further on
    const unsigned by = (unsigned)i0[1] / 3u, bz = (unsigned)i0[2] / 3u;
    const unsigned ly = (unsigned)i0[1] - 3u * by, lz = (unsigned)i0[2] - 3u * bz;
    const float* cell = E.dist + (((size_t)i0[0] * E.nby + by) * E.nbz + bz) * 32 + (ly * 4 + lz);
    double v[2][2][2];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            v[dx][dy][0] = (double)cell[dx * 16 + dy * 4];
            v[dx][dy][1] = (double)cell[dx * 16 + dy * 4 + 1];
        }
    const double c00 = v[0][0][0] * (1 - f[0]) + v[1][0][0] * f[0];
    const double c01 = v[0][0][1] * (1 - f[0]) + v[1][0][1] * f[0];
    const double c10 = v[0][1][0] * (1 - f[0]) + v[1][1][0] * f[0];
    const double c11 = v[0][1][1] * (1 - f[0]) + v[1][1][1] * f[0];
    const double c0 = c00 * (1 - f[1]) + c10 * f[1];
    const double c1 = c01 * (1 - f[1]) + c11 * f[1];
    out_d[q] = c0 * (1 - f[2]) + c1 * f[2];
    const double gx00 = v[1][0][0] - v[0][0][0], gx01 = v[1][0][1] - v[0][0][1];
    const double gx10 = v[1][1][0] - v[0][1][0], gx11 = v[1][1][1] - v[0][1][1];
    const double gx0 = gx00 * (1 - f[1]) + gx10 * f[1];
    const double gx1 = gx01 * (1 - f[1]) + gx11 * f[1];
    out_g[q * 3 + 0] = (gx0 * (1 - f[2]) + gx1 * f[2]) / E.res;
    const double gy0 = c10 - c00, gy1 = c11 - c01;
    out_g[q * 3 + 1] = (gy0 * (1 - f[2]) + gy1 * f[2]) / E.res;
    out_g[q * 3 + 2] = (c1 - c0) / E.res;
}

// The same query at the I/O width SURVEY.md §8(d) config 5 states for this fp32 lattice: float3 point in, float value +
// float3 gradient out (12 + 16 B per query instead of 24 + 32), all arithmetic in fp32 on the fp32 corners.  Own
// definition like the fp64 entry (no reference counterpart); each operation rounded once, in this order
// (-ffp-contract=off; oracle/vigo_oracle.c vgo_esdf_query_f32 is the same text):
//   u = (p - (float)origin) * inv_res - 0.5f with inv_res = 1.0f / (float)res computed ONCE on the host,
//   i = floorf(u) clamped to [0, n - 2] (frac 0 / 1 at the clamps), the trilinear blend x then y then z as above,
//   gradient differences * inv_res.  The result is ONE 16-byte store {d, gx, gy, gz}.
struct EsdfF32Const {
    float origin[3];
    float inv_res;
};
__global__ void k_esdf_query_f32(EsdfView E, EsdfF32Const C, int64_t Q, const float* __restrict__ pts, float4* __restrict__ out) {
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;     // XCD-aware tile map, as above
    const unsigned base = nb >> 3, rem = nb & 7u;
    const unsigned tile = xcd * base + (xcd < rem ? xcd : rem) + idx;
    const int64_t q = (int64_t)tile * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const int n[3] = {E.nx, E.ny, E.nz};
    int i0[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float u = (pts[q * 3 + a] - C.origin[a]) * C.inv_res - 0.5f;
        const float fl = floorf(u);
        // (NaN and out-of-range points: the comparisons are made on the float, so the int conversion is never out of range)
        int i;
        float fr = u - fl;
        if (!(fl >= 0.0f)) { i = 0; fr = 0.0f; }
        else if (fl > (float)(n[a] - 2)) { i = n[a] - 2; fr = 1.0f; }
        else i = (int)fl;
        i0[a] = i;
        f[a] = fr;
    }
    const unsigned by = (unsigned)i0[1] / 3u, bz = (unsigned)i0[2] / 3u;
    const unsigned ly = (unsigned)i0[1] - 3u * by, lz = (unsigned)i0[2] - 3u * bz;
    const float* cell = E.dist + (((size_t)i0[0] * E.nby + by) * E.nbz + bz) * 32 + (ly * 4 + lz);
    float v[2][2][2];
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            v[dx][dy][0] = cell[dx * 16 + dy * 4];
            v[dx][dy][1] = cell[dx * 16 + dy * 4 + 1];
        }
    const float c00 = v[0][0][0] * (1 - f[0]) + v[1][0][0] * f[0];
    const float c01 = v[0][0][1] * (1 - f[0]) + v[1][0][1] * f[0];
    const float c10 = v[0][1][0] * (1 - f[0]) + v[1][1][0] * f[0];
    const float c11 = v[0][1][1] * (1 - f[0]) + v[1][1][1] * f[0];
    const float c0 = c00 * (1 - f[1]) + c10 * f[1];
    const float c1 = c01 * (1 - f[1]) + c11 * f[1];
    float4 r;
    r.x = c0 * (1 - f[2]) + c1 * f[2];
    const float gx00 = v[1][0][0] - v[0][0][0], gx01 = v[1][0][1] - v[0][0][1];
    const float gx10 = v[1][1][0] - v[0][1][0], gx11 = v[1][1][1] - v[0][1][1];
    const float gx0 = gx00 * (1 - f[1]) + gx10 * f[1];
    const float gx1 = gx01 * (1 - f[1]) + gx11 * f[1];
    r.y = (gx0 * (1 - f[2]) + gx1 * f[2]) * C.inv_res;
    const float gy0 = c10 - c00, gy1 = c11 - c01;
    r.z = (gy0 * (1 - f[2]) + gy1 * f[2]) * C.inv_res;
    r.w = (c1 - c0) * C.inv_res;
    out[q] = r;
}

// one thread per destination float (coalesced writes); values past the lattice edge are zero-filled, never read.
// Line (x, by, bz) holds the values [x, x + 1] x [3 by, 3 by + 3] x [3 bz, 3 bz + 3], z fastest.
__global__ void k_esdf_brick(int nx, int ny, int nz, int nby, int nbz, size_t total, const float* __restrict__ src,
                             float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t line = i >> 5;
    const int r = (int)(i & 31);
    const int bz = (int)(line % nbz), by = (int)((line / nbz) % nby);
    const int x = (int)(line / ((size_t)nbz * nby)) + (r >> 4), y = by * 3 + ((r >> 2) & 3), z = bz * 3 + (r & 3);
    dst[i] = (x < nx && y < ny && z < nz) ? src[((size_t)x * ny + y) * nz + z] : 0.0f;
}

}  // namespace

size_t corridor_clock_ws_bytes(int S) { return (size_t)S * sizeof(ClockTable); }

int launch_esdf_brick(hipStream_t s, int nx, int ny, int nz, const float* src, float* dst) {
    const size_t total = esdf_bricked_floats(nx, ny, nz);
    const int block = 256;
    hipLaunchKernelGGL(k_esdf_brick, dim3((unsigned)((total + block - 1) / block)), dim3(block), 0, s, nx, ny, nz,
                       esdf_bricks_along(ny), esdf_bricks_along(nz), total, src, dst);
    return (int)hipGetLastError();
}

int launch_corridor_check2(hipStream_t s, const GridView& g, int S, int deg, const double* coeffs,
                           const int32_t* n_samp, const double* delT, const double box[3],
                           double map_res, uint8_t* out_flag, int32_t* out_first, int32_t* out_count, int* todo, void* clock_ws) {
    if (S <= 0) return hipSuccess;
    CorridorArgs A{};
    A.S = S; A.deg = deg;
    A.coeffs = coeffs; A.n_samp = n_samp; A.delT = delT;
    A.sweep = SweepConst{{box[0], box[1], box[2]}, map_res, 1.0 / g.res};
    A.out_flag = out_flag; A.out_first = out_first; A.out_count = out_count;
    // with the first pass' static LDS (21.6 KB): kCorridorWps workgroups per CU (18 KB of tile for four)
    const int tile_bytes = (160 * 1024 / kCorridorWps - 22 * 1024) & ~255;
    A.tile_words_cap = tile_bytes / 4;
    A.todo = todo;
    A.clocks = static_cast<const ClockTable*>(clock_ws);
    if (clock_ws)
        hipLaunchKernelGGL(k_corridor_clocks, dim3((S + 63) / 64), dim3(64), 0, s, S, n_samp, delT, static_cast<ClockTable*>(clock_ws));
    if (deg == 7) {
        hipLaunchKernelGGL((k_corridor<0, true>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
        hipLaunchKernelGGL((k_corridor<1, true>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
    } else {
        hipLaunchKernelGGL((k_corridor<0, false>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
        hipLaunchKernelGGL((k_corridor<1, false>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
    }
    return (int)hipGetLastError();
}

int launch_poly_sample(hipStream_t s, int S, int deg, const double* coeffs, const int32_t* n_samp, const double* delT,
                       int stride, double* out_pos, float* out_f32) {
    if (S <= 0 || stride <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_poly_sample, dim3(S), dim3(kBlock), 0, s, S, deg, coeffs, n_samp, delT, stride, out_pos, out_f32);
    return (int)hipGetLastError();
}

int launch_box_points(hipStream_t s, const GridView& g, int64_t M, const double* pts, const double box[3],
                      double map_res, uint8_t* out) {
    if (M <= 0) return hipSuccess;
    const int block = 256;
    hipLaunchKernelGGL(k_box_points, dim3((unsigned)((M + block - 1) / block)), dim3(block), 0, s, g, M, pts,
                       SweepConst{{box[0], box[1], box[2]}, map_res, 1.0 / g.res}, out);
    return (int)hipGetLastError();
}

int launch_esdf_query(hipStream_t s, const EsdfView& e, int64_t Q, const double* pts,
                      double* out_dist, double* out_grad) {
    if (Q <= 0) return hipSuccess;
    const int block = 256;
    hipLaunchKernelGGL(k_esdf_query, dim3((unsigned)((Q + block - 1) / block)), dim3(block), 0, s, e, Q, pts,
                       out_dist, out_grad);
    return (int)hipGetLastError();
}

int launch_esdf_query_f32(hipStream_t s, const EsdfView& e, int64_t Q, const float* pts, float* out4) {
    if (Q <= 0) return hipSuccess;
    EsdfF32Const C;
    for (int a = 0; a < 3; ++a) C.origin[a] = (float)e.origin[a];
    C.inv_res = 1.0f / (float)e.res;
    const int block = 256;
    hipLaunchKernelGGL(k_esdf_query_f32, dim3((unsigned)((Q + block - 1) / block)), dim3(block), 0, s, e, C, Q, pts,
                       reinterpret_cast<float4*>(out4));
    return (int)hipGetLastError();
}

}  // namespace vigo
