// vigo_internal.hpp — host-side types shared by the C-ABI layer and the kernel launchers.
// Not part of the public boundary (that is include/vigo.h).  The handle itself (vigo_handle.hpp) is not in here: the kernel
// files cannot depend on it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vigo.h"

namespace vigo {

// Scalars derived from vigo_params_t once on the host, with the reference's own expressions
// (BT.cpp:835, :959, :1007-1009) so the device sees the same bits as the CPU path.
struct DevConst {
    // distance term (BT.cpp:835)
    double dth, da, db, dc;
    double unc_factor;
    // height band (BT.cpp:836-837, plan_in_z only)
    double hth, ha, hb, hc, min_h, max_h;
    // feasibility (BT.cpp:955-959)
    double ts_ctrl, ts_inv_sqr;
    // dynamic obstacles (BT.cpp:1007-1009)
    double ts, thr_dyn, oa, ob, oc;
    int pred_num;
    int plan_in_z;
    int strict_z;      // 1: no level rule
    // default weights
    double w[4];
    // L-BFGS (LB:87-191)
    int mem_size, max_iterations, max_linesearch;
    double g_epsilon, min_step, max_step, ftol, gtol, xtol;
};

DevConst make_dev_const(const vigo_params_t& P);

struct SolveArgs {
    int B, N;
    double* ctrl;  // in/out for optimize, read-only for cost_grad
    const int32_t* guide_off;
    const double* guide_pv;
    const uint8_t* guide_unk;
    const int32_t* obs_off;
    const double* obs;
    int n_obs_shared;
    const double* weights;
    // (vigo_rebound_rounds) the launch works on trajectory active_idx[slot] for slot < *active_count instead of
    // b = slot < B; lbfgs_status_stride != 0: out_status is the lbfgs_status field of a vigo_rebound_state_t array
    const int32_t* active_idx;
    const int32_t* active_count;
    int status_stride;     // in int32 units between consecutive trajectories' out_status (0 = 1)
    // optimize outputs
    double* out_x;
    int32_t* out_status;
    double* out_fx;
    int32_t* out_iters;
    int32_t* out_evals;
    // (set by the solve launcher) 1: the waves whose trajectories are all level are solved by a second launch (D = 2);
    // 2: EVERY level trajectory is solved elsewhere (the axis-per-lane launch, D = 1), whatever it shares a wave with
    int level_waves_elsewhere;
    // cost_grad outputs
    double* out_cost;
    double* out_grad;
    double* out_terms;
};
// (vigo_*_mixed) the arguments of the MIXED instantiations: N is the row stride of ctrl, guide_off and the outputs,
// trajectory b has n_pts[b] control points.  A type of its own: SolveArgs is what every other kernel was measured with
struct MixedSolveArgs : SolveArgs {
    const int32_t* n_pts;
};

// Packed voxel snapshot in HBM: three bit planes (inflated-occupied, unknown, occupied), each
// nx*ny rows of nzw 32-bit words, z fastest (bit k of word w = voxel z = 32*w + k).
struct GridView {
    const uint32_t* planes;  // 3 * plane_words
    size_t plane_words;
    int nx, ny, nz, nzw;
    double origin[3];
    double res;
    double bmin[3], bmax[3];
    int key0[3];  // octomap key of voxel index 0 minus 32768 (corridor checker)
};

// ESDF samples in HBM as one 128-B cache line per group of trilinear cells: line (x, by, bz) holds the 2 x 4 x 4 values
// [x, x+1] x [3 by, 3 by + 3] x [3 bz, 3 bz + 3] (z fastest), i.e. the 1 x 3 x 3 whole cells starting at (x, 3 by, 3 bz):
// all eight corners of ANY cell lie in ONE line (one base address + constant offsets), at 3.56x the lattice's bytes.
// Uniformly random queries are bound by the cache lines they touch (a 256^3 lattice lives in the Infinity Cache, not
// in L2): the row-major lattice costs 4.1 lines per cell, disjoint 4x4x4 bricks 2.3, overlapping 4x4x4 bricks 1.33.
struct EsdfView {
    const float* dist;        // (nx - 1) * nby * nbz lines of 32 floats
    int nx, ny, nz;
    int nby, nbz;             // lines along y and z
    double origin[3];
    double res;
};
inline int esdf_bricks_along(int n) { return (n + 1) / 3; }   // ceil((n - 1) / 3) groups cover the n - 1 cells, n >= 2
inline size_t esdf_bricked_floats(int nx, int ny, int nz) {
    return (size_t)(nx - 1) * esdf_bricks_along(ny) * esdf_bricks_along(nz) * 32;
}

// Per-handle (= per-device) launch state: which kernel instantiations already had their dynamic-LDS limit raised on
// the handle's device, and that device's SIMD count.  Nothing of this kind is kept in function statics.
struct LaunchState {
    uint64_t lds_attr_set = 0;   // bit per k_optimize instantiation (its index in kOptimizeKeys, vigo_solver_plan.hpp)
    bool minsnap_attr_set = false;
    bool astar_attr_set = false;
    int simd_count = 0;          // 4 per CU; 0 = unknown
};

// launchers (each returns hipError_t as int)
// k: host copy (launch geometry), kd: the same constants in device memory (read by the kernels)
int launch_cost_grad(hipStream_t s, const SolveArgs& a, const DevConst& k, const DevConst* kd, int precision);
int launch_optimize(hipStream_t s, const SolveArgs& a, const DevConst& k, const DevConst* kd, int precision, LaunchState& L);
// the mixed-count entries (a.n_pts set, a.N the row stride, 7 .. 64): one launch of the general kernel
int launch_cost_grad_mixed(hipStream_t s, const MixedSolveArgs& a, const DevConst* kd, int precision);
int launch_optimize_mixed(hipStream_t s, const MixedSolveArgs& a, const DevConst& k, const DevConst* kd, int precision, LaunchState& L);

int launch_pack_grid(hipStream_t s, int nx, int ny, int nz, const uint8_t* vox, uint32_t* packed);
int launch_inflate(hipStream_t s, int nx, int ny, int nz, uint8_t* vox, uint32_t* planeA, uint32_t* planeB, int rx, int ry, int rz);
// vigo_grid_update.hip: the box' bytes into the planes in place; in inflate mode plane 0 again on the grown box, through
// the two compact window planes of region_window_words(p) words each
struct RegionPlan;
int launch_grid_region(hipStream_t s, const RegionPlan& p, const uint8_t* vox, uint32_t* planes, size_t plane_words,
                       uint32_t* planeA, uint32_t* planeB);
int launch_query_points(hipStream_t s, const GridView& g, int which, int64_t Q, const double* pts,
                        int pt_stride, uint8_t* out);
int launch_bspline_eval(hipStream_t s, int B, int N, const double* ctrl, double ts_ctrl, int deriv,
                        int T, const double* times, double* out);
int launch_traj_collision(hipStream_t s, const GridView& g, int B, int N, const double* ctrl,
                          double ts_ctrl, int T, const double* times, uint8_t* out_flag,
                          int32_t* out_first);
int launch_traj_dynamic_collision(hipStream_t s, int B, int N, const double* ctrl, double ts_ctrl,
                                  int T, const double* times, const int32_t* obs_off,
                                  const double* obs, int n_obs_shared, uint8_t* out_flag);
int launch_fill_sample_times(hipStream_t s, double dt, int T, double* times);
int launch_ctrl_occupancy(hipStream_t s, const GridView& g, int B, int N, const double* ctrl,
                          uint8_t* out_pt, uint8_t* out_line);
// the corridor checker's two passes (vigo_corridor_core.hpp, k_corridor).  todo: S ints of device scratch (which segments the
// first pass left to the second); clock_ws: corridor_clock_ws_bytes(S) bytes of device scratch, 8-byte aligned, for the
// segments' sample-clock tables, or NULL (every workgroup then builds its own).  (The "2" stays: the call's text is
// part of the error vigo_corridor_check reports when the launch fails.)
size_t corridor_clock_ws_bytes(int S);
int launch_corridor_check2(hipStream_t s, const GridView& g, int S, int deg, const double* coeffs, const int32_t* n_samp,
                           const double* delT, const double box[3], double map_res, uint8_t* out_flag, int32_t* out_first,
                           int32_t* out_count, int* todo, void* clock_ws);
// whole trajectories (vigo_traj_corridor_check): ws = traj_ws_bytes(S, T_chunk) bytes of device scratch, 8-byte aligned;
// the trajectories are taken T_chunk at a time (clock tables per chunk, per-segment state for all S)
size_t traj_ws_bytes(int S, int T_chunk);
int launch_traj_corridor(hipStream_t s, const GridView& g, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                         const double* knots, const double* delT, const double* endpoint, const double box[3], double map_res,
                         int nonfinite, int32_t* out_status, int32_t* out_n, uint8_t* out_flag, int32_t* out_first,
                         int32_t* out_count, uint8_t* out_seg, void* ws, int T_chunk);
// whole trajectories, point test (vigo_traj_point_check): the same workspace (traj_ws_bytes) and chunking
int launch_traj_point(hipStream_t s, const GridView& g, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                      const double* knots, const double* delT, const double* endpoint, int32_t* out_status, int32_t* out_n,
                      uint8_t* out_flag, int32_t* out_first, int32_t* out_count, uint8_t* out_seg, void* ws, int T_chunk);
// the seed-path stage (vigo_seed_paths, vigo_seed.hip): a wave per trajectory, no workspace
int launch_seed_paths(hipStream_t s, const GridView& g, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                      const double* knots, const double* duration, const double* dt0, const double* control_point_distance,
                      const double* max_path_length, const double* prev_in_seed, const double* prev_in_fit, int max_tries,
                      int point_cap, int32_t* out_status, int32_t* out_tries, double* out_dt, double* out_final_time,
                      int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit, double* out_prev_seed,
                      double* out_prev_fit);
int launch_box_points(hipStream_t s, const GridView& g, int64_t M, const double* pts, const double box[3],
                      double map_res, uint8_t* out);
// polyTrajSolver::getTrajectory for S segments: sample k of segment s at out[(s * stride + k) * 3] (fp64 and/or float)
int launch_poly_sample(hipStream_t s, int S, int deg, const double* coeffs, const int32_t* n_samp, const double* delT,
                       int stride, double* out_pos, float* out_f32);
// the gate + decision pass of vigo_rebound_rounds (one wave per trajectory) and the compaction of the active set
struct ReboundArgs {
    int B, N;
    const double* ctrl;
    const int32_t* guide_off;
    const double* guide_pv;
    const int32_t* obs_off;
    const double* obs;
    int n_obs_shared;
    double* weights;
    vigo_rebound_state_t* state;
    double ts_ctrl;
    int T;                   // samples of the whole trajectory (dynamic gate, BT.h:345)
    int T_static;            // samples up to (1 - not_check_ratio) * duration (static gate, BT.h:313); <= T
    const double* times;
    double dthresh, not_check_ratio;
    int32_t* flags;          // see k_rebound_compact
    // (vigo_rebound_rounds_mixed) not NULL: trajectory b has n_pts[b] control points in a row of N, and its gates take
    // {T, T_static} from count_tab[2 * (n_pts[b] - 7)] (one pair per count 7 .. N) instead of the two fields above;
    // `times` then holds the clock of the longest duration, of which every count's samples are a prefix
    const int32_t* n_pts;
    const int32_t* count_tab;
};
// (vigo_rebound_rounds_mixed, before the first compaction) an ACTIVE trajectory whose count breaks the contract of the
// mixed entries is handed to the host: status VIGO_RB_NEEDS_HOST, lbfgs_status LBFGSERR_INVALID_N, nothing else touched
int launch_rebound_check_counts(hipStream_t s, int B, int Ns, const int32_t* n_pts, vigo_rebound_state_t* state);
int launch_rebound_decide(hipStream_t s, const GridView& g, const ReboundArgs& a);
// mode 0: status == ACTIVE && solve_first (clears solve_first); mode 1: status == ACTIVE.  Ascending order.
int launch_rebound_compact(hipStream_t s, int B, vigo_rebound_state_t* state, int mode, int32_t* idx, int32_t* flags);
// counts CSR violations of guide_off[B*N+1] / obs_off[B+1] into *bad (device int, zeroed by the launcher)
int launch_check_lists(hipStream_t s, int B, int N, const int32_t* guide_off, int64_t G, const int32_t* obs_off, int64_t O,
                       int* bad);
int launch_esdf_query(hipStream_t s, const EsdfView& e, int64_t Q, const double* pts,
                      double* out_dist, double* out_grad);
// fp32 I/O and arithmetic: pts float[Q][3], out float[Q][4] = {d, gx, gy, gz} (16-byte aligned)
int launch_esdf_query_f32(hipStream_t s, const EsdfView& e, int64_t Q, const float* pts, float* out4);
// row-major [nx][ny][nz] -> the bricked layout of EsdfView
int launch_esdf_brick(hipStream_t s, int nx, int ny, int nz, const float* src, float* dst);
// the ESDF build (vigo_esdf_build.hip): the snapshot's plane (0 or 2, OR the unknown plane) -> the row-major float
// lattice; a, b: the two int32 buffers of esdf_build_ws_bytes, lattice may be a
size_t esdf_build_ws_bytes(int nx, int ny, int nz);
int launch_esdf_build(hipStream_t s, const GridView& g, int plane, int unknown_is_site, int32_t* a, int32_t* b, float* lattice);
// the region update on what a tracked build kept (w: EsdfTrackWs of vigo_esdf_core.hpp): the checked, non-empty box
// [lo, lo + n) of the snapshot changed; bricked: the installed field; count: also the flagged lines into w.counters
struct EsdfTrackWs;
int launch_esdf_region_update(hipStream_t s, const GridView& g, const int32_t lo[3], const int32_t n[3], int plane, int unknown_is_site,
                              const EsdfTrackWs& w, float* bricked, bool count);
// batched B-spline fit (vigo_fit.hip): one-off device factorisation per (K, ts), then the fit
size_t fit_work_doubles(int K);
size_t fit_pinv_doubles(int K);
int launch_fit_setup(hipStream_t s, int K, double ts, double* work, double* pinvT);
int launch_bspline_fit(hipStream_t s, int B, int K, const double* pinvT, const double* points,
                       const double* conds, double* out);
// mixed point counts (vigo_fit_plan.hpp): the operators of K = 4 .. 62 into `table` (work: fit_table_work_doubles()),
// then the regrouping and the product; perm int32[T] and tab int32[2 * (kFitBins + 1)] are the call's workspace
int launch_fit_setup_table(hipStream_t s, double ts, double* work, double* table);
int launch_bspline_fit_mixed(hipStream_t s, int T, int Ns, int point_stride, const double* table, const int32_t* n_fit,
                             const int32_t* status, const double* points, const double* conds, int32_t* perm, int32_t* tab,
                             double* out, int32_t* out_n_pts);

// the end of a plan (vigo_finish.hip, the rule of vigo_finish_core.hpp): a wave per trajectory.  times_ts[T_ts]: the
// `t += ts` clock below the longest duration (Ns - 3) * ts_ctrl; times_dt[T_dt]: the `t += sample_dt` clock up to it
struct FinishArgs {
    int B, Ns;
    const int32_t* n_pts;        // NULL: every row has Ns control points
    const double* ctrl;          // [B][Ns][3]
    const double* limits;        // [B][2] max_vel, max_acc
    double ts_ctrl, sample_dt;
    int S_cap, T_ts, T_dt;
    const double *times_ts, *times_dt;
    double* out_factor;          // [B]
    double* out_max;             // [B][2] or NULL
    int32_t* out_n;              // [B]
    double* out_pos;             // [B][S_cap][3]
    double* out_vel;             // [B][S_cap][3] or NULL
    int32_t* out_status;         // [B]
};
int launch_traj_finish(hipStream_t s, const FinishArgs& a);

// plan validation (vigo_validate.hip, the rule of vigo_validate_core.hpp): a wave per trajectory, then the ascending list of
// the invalid rows.  times[T]: the `t += dt` clock up to the longest duration (Ns - 3) * ts_ctrl; count_tab: {S, C} of
// every count 4 .. Ns (validate_tab_entries(Ns) int32)
struct ValidateArgs {
    int B, Ns;
    const int32_t* n_pts;        // NULL: every row has Ns control points
    const double* ctrl;          // [B][Ns][3]
    double ts_ctrl;
    int T;
    const double* times;
    const int32_t* count_tab;
    const int32_t* obs_off;
    const double* obs;
    int n_obs_shared;
    int32_t* out_status;         // [B]
    int32_t* out_first;          // [B]
    double* out_pos;             // [B][3] or NULL
    int32_t* out_dyn_first;      // [B] or NULL
    int32_t* out_invalid;        // [B] and [1], or both NULL
    int32_t* out_n_invalid;
};
int launch_traj_validate(hipStream_t s, const GridView& g, const ValidateArgs& a);

// batched min-snap QP (vigo_minsnap.hip)
size_t minsnap_lds_bytes(int W, int cont);
int minsnap_max_waypoints();
bool minsnap_supported(int W, int deg, int diff, int cont);   // vigo_minsnap_supported
int launch_minsnap(hipStream_t s, int T, int W, int deg, int diff, int cont, double vel, double corridor_res,
                   const double* wp, const double* corridor, const double* conds, double* out_coeffs,
                   double* out_knots, int32_t* out_status, LaunchState& L);

// batched A* (vigo_astar.hip): the largest search the kernels hold (pushed nodes, open-set entries)
int astar_max_nodes();
int astar_max_heap();
int launch_astar(hipStream_t s, const GridView& g, int Q, const double* start, const double* end, double step, const int32_t pool[3],
                 double min_h, double max_h, int max_expansions, int path_cap, int32_t* out_status, int32_t* out_len, double* out_path,
                 int32_t* out_stats, LaunchState& L);

// batched guide assignment (vigo_guides.hip): the offsets kernel fills result[2] = {pairs of the call, bad lists} and,
// when the lists are good and the pairs fit, statuses and offsets; the assign kernel then writes the pairs in place.
// n_pts not NULL (the _mixed entries): N is the row stride of ctrl and of the offsets, trajectory b has n_pts[b] points
int guide_path_capacity();
int launch_guide_offsets(hipStream_t s, int B, int N, const int32_t* n_pts, const int32_t* seg_off, const int32_t* seg, const int32_t* path_off, long long pair_cap,
                         int32_t* out_off, int32_t* out_status, long long* result);
int launch_guide_assign(hipStream_t s, const GridView& g, int B, int N, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off,
                        const int32_t* seg, const int32_t* path_off, const double* path, const int32_t* off, double* out_pv, uint8_t* out_unk,
                        const int32_t* status);

// batched findCollisionSeg / pathSearch (vigo_pathsearch.hip).  Everything but the out_* members is device scratch of
// the call; the kernels and what vigo_api.cpp reads back between them are listed in that file's header.
struct PathSearchArgs {
    int B, N;
    const int32_t* n_pts;        // (the _mixed entries) not NULL: N is the row stride, trajectory b has n_pts[b] control points
    const double* ctrl;
    double not_check_ratio;
    const int32_t* seg_off_in;   // the supplied list, or NULL: the scan over pt / ln
    const int32_t* seg_in;
    const int32_t* seg_cnt_in;   // not NULL: trajectory b's list is seg_cnt_in[b] segments at seg_in[b * seg_stride_in]
    int seg_stride_in;           // (seg_off_in is not read; B * seg_stride_in fits an int)
    const uint8_t* pt;           // [B][N] vigo_ctrl_occupancy's flags
    const uint8_t* ln;
    int search_path_cap;
    long long* result;           // [0] first-choice searches, [1] != 0: a bad list, [2] second-choice searches,
                                 // [3] segments of the output, [4] its path points
    int32_t* in_off;             // [B+1] first search / input segment of a trajectory
    int32_t* n_in;               // [B]   its input segments (0 when pre)
    int32_t* pre;                // [B]   != 0: more than VIGO_MAX_COLLISION_SEGS segments
    int32_t* tstatus;            // [B]   k_ps_decide: status, segments, first output segment, first path point, counts
    int32_t* n_out;
    int32_t* oseg_off;
    int32_t* opt_off;
    int32_t* tcounts;            // [B][2]
    int32_t* out_status;
    int32_t* out_seg_off;
    int32_t* out_seg;
    int32_t* out_path_off;
    double* out_path;
    int32_t* out_counts;
};
struct PathSearchWork {          // sized by the searches of the call
    int32_t* seg;                // [S][2] input segments
    int32_t* mseg;               // [S][2] a trajectory's segments after the merges (at in_off)
    int32_t* pick;               // [S]    its paths' searches (path_walk)
    int32_t* retry_of;           // [S]    the second-choice search of a segment, or -1
    double* start1;              // [S][3]
    double* end1;
    double* start2;              // [S][3] (Q2 <= S used)
    double* end2;
    int32_t* status1;            // [S]
    int32_t* len1;
    double* path1;               // [S][search_path_cap][3]
    int32_t* status2;            // [Q2]
    int32_t* len2;
    double* path2;
};
int launch_ps_count(hipStream_t s, const PathSearchArgs& a);
int launch_ps_fill(hipStream_t s, const PathSearchArgs& a, int32_t* dst_seg, double* start, double* end);
int launch_ps_segs_out(hipStream_t s, const PathSearchArgs& a);
int launch_ps_retry(hipStream_t s, const PathSearchArgs& a, const PathSearchWork& w);
int launch_ps_decide(hipStream_t s, const PathSearchArgs& a, const PathSearchWork& w);
int launch_ps_write(hipStream_t s, const PathSearchArgs& a, const PathSearchWork& w, int total_seg, int total_pts);

// the re-guide step of the rebound loop (vigo_reguide.hip); the kernels and what vigo_api.cpp reads back between them
// are listed in that file's header.  Everything but the out_* members and the caller's inputs is device scratch.
struct ReguideArgs {
    int B, N;
    const int32_t* n_pts;        // (vigo_rebound_reguide_mixed) not NULL: N is the row stride, trajectory b has n_pts[b] control points
    const double* ctrl;
    const int32_t* guide_off;    // the current CSR, or NULL: no guides
    const double* guide_pv;
    const uint8_t* guide_unk;    // may be NULL: the merged flags of the old pairs are then queried
    double* weights;
    vigo_rebound_state_t* state;
    double dthresh, not_check_ratio;
    long long* result;           // [0] != 0: guide_off decreases or starts below 0, [1] the merged pairs
    int32_t* kind;               // [B]  k_reguide_list: kReguideSkipped / kReguideDeferred / -1 (eligible, rules run)
    int32_t* n_list;             // [B]  segments of the re-guide list
    int32_t* list;               // [B][VIGO_MAX_COLLISION_SEGS][2]
    int32_t* n_new;              // [B]  the new collisionSeg_
    int32_t* new_seg;            // [B][VIGO_MAX_COLLISION_SEGS][2]
    const int32_t* ps_status;    // [B]  vigo_path_search's outputs on the list
    const int32_t* ps_seg_off;   // [B+1]
    const int32_t* ps_counts;    // [B][2]
    const int32_t* g_status;     // [B]  vigo_guide_assign's outputs on those
    const int32_t* g_off;        // [B*N+1]
    const double* g_pv;
    const uint8_t* g_unk;
    int32_t* outcome;            // [B]  k_guide_merge_offsets: kReguide*
    long long pair_cap;
    int32_t* out_guide_off;
    double* out_guide_pv;
    uint8_t* out_guide_unk;
    int32_t* out_status;
};
int launch_reguide_list(hipStream_t s, const GridView& g, const ReguideArgs& a);
int launch_guide_merge_offsets(hipStream_t s, const ReguideArgs& a);
int launch_guide_merge(hipStream_t s, const GridView& g, const ReguideArgs& a);
int launch_reguide_commit(hipStream_t s, const ReguideArgs& a);

}  // namespace vigo
