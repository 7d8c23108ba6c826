// vigo_traj_corridor.hip — vigo_traj_corridor_check: checkCollisionTraj of polyTrajOctomap (PO.cpp:634-656) on whole
// trajectories, the checker of vigo_corridor_core.hpp in its trajectory mode (k_corridor<PASS, DEG7, true>).  A separate
// translation unit, so that the instantiations vigo_corridor_check launches keep their code.
#include "vigo_corridor_core.hpp"
#include "vigo_traj_core.hpp"

namespace vigo {
namespace {

// ---- whole trajectories (vigo_traj_corridor_check): checkCollisionTraj of polyTrajOctomap, PO.cpp:634-656 ---------------
// k_corridor<PASS, DEG7, true> (a workgroup per run) between the shared stages of vigo_traj_core.hpp: k_traj_runs before
// it, k_traj_finish with the box sweep after it.

// pose2Octomap's float cast and the box sweep (PO.cpp:547-589); a pose at NaN / infinity collides only with
// VIGO_TRAJ_NONFINITE_COLLIDES
struct BoxHit {
    GridView g;
    SweepConst C;
    int nonfinite;
    __device__ bool operator()(double x, double y, double z) const {
        const bool finite = isfinite(x) && isfinite(y) && isfinite(z);
        return (nonfinite && !finite) || box_sweep(g, C, (float)x, (float)y, (float)z, nullptr, nullptr);
    }
};

}  // namespace

size_t traj_ws_bytes(int S, int T_chunk) { return traj_work_bytes(S, T_chunk); }

int launch_traj_corridor(hipStream_t s, const GridView& g, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                         const double* knots, const double* delT, const double* endpoint, const double box[3], double map_res,
                         int nonfinite, int32_t* out_status, int32_t* out_n, uint8_t* out_flag, int32_t* out_first,
                         int32_t* out_count, uint8_t* out_seg, void* ws, int T_chunk) {
    TrajWork W;
    hipError_t e = traj_prepare(s, ws, T, S, T_chunk, seg_off, knots, delT, endpoint, out_seg, W);
    if (e != hipSuccess || T <= 0) return (int)e;

    const SweepConst sweep{{box[0], box[1], box[2]}, map_res, 1.0 / g.res};
    CorridorArgs A{};
    A.S = S; A.deg = deg;
    A.coeffs = coeffs; A.n_samp = W.run_len; A.delT = delT;
    A.sweep = sweep;
    A.out_flag = W.run_flag; A.out_first = W.run_hit; A.out_count = W.run_count;
    const int tile_bytes = (160 * 1024 / kCorridorWps - 22 * 1024) & ~255;   // as launch_corridor_check2
    A.tile_words_cap = tile_bytes / 4;
    A.todo = W.todo;
    A.clocks = W.clocks;
    A.run_first = W.run_first; A.seg_traj = W.seg_traj; A.knots = knots;
    A.nonfinite = nonfinite;
    for (int t0 = 0; t0 < T; t0 += T_chunk) {
        const int t1 = T - t0 < T_chunk ? T : t0 + T_chunk;
        W.t_lo = A.t_lo = t0;
        W.t_hi = A.t_hi = t1;
        const int nb = (t1 - t0 + 63) / 64;
        hipLaunchKernelGGL(k_traj_runs, dim3(nb), dim3(64), 0, s, W);
        if (S > 0) {
            if (deg == 7) {
                hipLaunchKernelGGL((k_corridor<0, true, true>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
                hipLaunchKernelGGL((k_corridor<1, true, true>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
            } else {
                hipLaunchKernelGGL((k_corridor<0, false, true>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
                hipLaunchKernelGGL((k_corridor<1, false, true>), dim3(S), dim3(kBlock), tile_bytes, s, g, A);
            }
        }
        hipLaunchKernelGGL(k_traj_finish<BoxHit>, dim3(nb), dim3(64), 0, s, BoxHit{g, sweep, nonfinite}, W, out_status, out_n,
                           out_flag, out_first, out_count, out_seg);
    }
    return (int)hipGetLastError();
}

}  // namespace vigo
