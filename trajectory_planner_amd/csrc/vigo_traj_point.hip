// vigo_traj_point.hip — vigo_traj_point_check: checkCollisionTraj of polyTrajOccMap (PM.cpp:524-546) on whole
// trajectories.  The stages of vigo_traj_core.hpp (runs, finish) around a plain per-run pass: the test of a sample is ONE
// lookup of its fp64 pose in two bit planes — no float cast, no box — so the corridor checker's span certificates and
// LDS tiles have nothing to save here.
#include "vigo_corridor_core.hpp"
#include "vigo_traj_core.hpp"

namespace vigo {
namespace {

// PM.cpp:532: map_->isInflatedOccupied(p) and map_->isUnknown(p) on the fp64 pose — bits 0 and 1 of voxel
// floor((p - origin) / res), as vigo_query_points; outside the grid (a NaN or infinite coordinate included) every bit is
// set, so such a pose collides
struct PointHit {
    GridView g;
    __device__ bool operator()(double x, double y, double z) const {
        const unsigned v = grid_bits_at(g, grid_index(x, g.origin[0], g.res, g.nx), grid_index(y, g.origin[1], g.res, g.ny),
                                        grid_index(z, g.origin[2], g.res, g.nz));
        return (v & 3u) == 3u;
    }
};

// A wave per run (segment s of the chunk's trajectories): the segment's coefficients and its trajectory's clock table
// are staged in LDS, lanes stride the run's samples — clock from the table as k_corridor's per-sample path, fp64 pose
// from poly_pos7 / poly_pos as k_poly_sample (vigo_poly_sample), so both are bit for bit theirs — and 64-bit ballots
// reduce the run to flag, first hit and count, which lane 0 writes.  No atomics.
constexpr int kPointWaves = 4;
__global__ void __launch_bounds__(64 * kPointWaves) k_traj_point(PointHit hit, TrajWork W, int deg,
                                                                 const double* __restrict__ coeffs) {
    __shared__ double s_cf[kPointWaves][3 * (kMaxDeg + 1)];
    __shared__ ClockTable s_clock[kPointWaves];
    const int wv = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int s = blockIdx.x * kPointWaves + wv;
    int tr = -1, n = 0;
    if (s < W.S) {
        tr = W.seg_traj[s];
        if (tr >= W.t_lo && tr < W.t_hi) n = W.run_len[s];   // (k_traj_runs wrote the results of an empty run)
    }
    double* cf = s_cf[wv];
    ClockTable& C = s_clock[wv];
    if (n > 0) {
        for (int i = lane; i < 3 * (deg + 1); i += 64) {
            const int ax = i / (deg + 1), d = i % (deg + 1);
            cf[ax * (kMaxDeg + 1) + d] = coeffs[((size_t)s * 3 + ax) * (deg + 1) + d];
        }
        const int* src = reinterpret_cast<const int*>(W.clocks + (tr - W.t_lo));
        int* dst = reinterpret_cast<int*>(&C);
        for (int i = lane; i < (int)(sizeof(ClockTable) / sizeof(int)); i += 64) dst[i] = src[i];
    }
    __syncthreads();
    if (n == 0) return;                                          // (wave-uniform)
    const int first = W.run_first[s];
    const double dT = W.delT[tr];
    const double kb = W.knots[s + tr];
    const bool table = C.n > 0;
    double c7[3][8];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 8; ++d) c7[a][d] = deg == 7 ? cf[a * (kMaxDeg + 1) + d] : 0.0;
    int hit_first = -1, count = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {                        // n is the wave's: every lane takes every ballot
        const int j = j0 + lane;
        bool h = false;
        if (j < n) {
            const double tg = table ? clock_at(C, first + j) : accumulated_time(dT, first + j);
            const double t = tg - kb;                            // rule 2: fl(t_j - k[i])
            double p[3];
            if (deg == 7) poly_pos7(c7, t, p);
            else poly_pos(cf, deg, t, p);
            h = hit(p[0], p[1], p[2]);
        }
        const unsigned long long m = __ballot(h);
        if (hit_first < 0 && m) hit_first = j0 + __builtin_ctzll(m);
        count += __popcll(m);
    }
    if (lane == 0) {
        W.run_flag[s] = (uint8_t)(count > 0);
        W.run_hit[s] = hit_first;
        W.run_count[s] = count;
    }
}

}  // namespace

int launch_traj_point(hipStream_t s, const GridView& g, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                      const double* knots, const double* delT, const double* endpoint, int32_t* out_status, int32_t* out_n,
                      uint8_t* out_flag, int32_t* out_first, int32_t* out_count, uint8_t* out_seg, void* ws, int T_chunk) {
    TrajWork W;
    hipError_t e = traj_prepare(s, ws, T, S, T_chunk, seg_off, knots, delT, endpoint, out_seg, W);
    if (e != hipSuccess || T <= 0) return (int)e;
    const PointHit hit{g};
    for (int t0 = 0; t0 < T; t0 += T_chunk) {
        const int t1 = T - t0 < T_chunk ? T : t0 + T_chunk;
        W.t_lo = t0;
        W.t_hi = t1;
        const int nb = (t1 - t0 + 63) / 64;
        hipLaunchKernelGGL(k_traj_runs, dim3(nb), dim3(64), 0, s, W);
        if (S > 0)
            hipLaunchKernelGGL(k_traj_point, dim3((S + kPointWaves - 1) / kPointWaves), dim3(64 * kPointWaves), 0, s, hit, W, deg,
                               coeffs);
        hipLaunchKernelGGL(k_traj_finish<PointHit>, dim3(nb), dim3(64), 0, s, hit, W, out_status, out_n, out_flag, out_first,
                           out_count, out_seg);
    }
    return (int)hipGetLastError();
}

}  // namespace vigo
