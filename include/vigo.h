/*
 * vigo.h — C ABI of libvigo_hip.so, the MI355X (gfx950) batched back-end for the
 * ViGO B-spline optimizer hot path and the min-snap corridor collision checker of
 * hanyujin02/trajectory_planner.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repo, BT = include/trajectory_planner/bsplineTraj.{h,cpp},
 * LB = include/trajectory_planner/solver/lbfgs.hpp, BS = .../bspline.cpp,
 * PO = .../polyTrajOctomap.cpp, PS = .../polyTrajSolver.cpp).
 *
 * Conventions
 *   - plain C types only; no C++/torch types cross this boundary.
 *   - every array argument is a DEVICE pointer unless the function name ends in
 *     `_host` (those stage through an internal device workspace).
 *   - return value: 0 = VIGO_OK, negative = vigo_status_t error.  Per-trajectory solver
 *     results use the reference's own L-BFGS codes (LB:20-80) in `out_status`.
 *   - a handle owns its device buffers and HIP stream binding; calls on one handle are
 *     serialized by the caller; there is no global state.  A handle belongs to the device it was
 *     created on: that device must be the calling thread's current HIP device during every call
 *     (one process per GPU, or hipSetDevice first) — launches go to the bound stream / the current
 *     device's default stream.
 *   - all floating point arrays are fp64 (the reference's arithmetic, BT.h:22) unless the
 *     name says f32.
 *
 * Batch layouts (B trajectories, N control points each, n = 3*(N-6) free scalars):
 *   ctrl        double[B][N][3]      == B copies of Eigen::MatrixXd(3,N) column-major
 *                                       (optData::controlPoints, BT.h:22)
 *   guide_off   int32 [B*N + 1]      CSR offsets: control point (b,i) owns guide pairs
 *                                       [guide_off[b*N+i], guide_off[b*N+i+1])
 *                                       (optData::guidePoints[i][j], BT.h:23-24)
 *   guide_pv    double[G][6]         (p.x p.y p.z v.x v.y v.z) per pair
 *   guide_unk   uint8 [G]            map_->isUnknown(p) per pair (BT.cpp:841); may be NULL
 *                                       (=> all known).  vigo_guides_unknown() fills it.
 *   obs_off     int32 [B + 1]        CSR offsets of dynamic obstacles per trajectory, or NULL
 *                                       with n_obs_shared obstacles shared by the whole batch
 *   obs         double[O][9]         (pos.xyz vel.xyz size.xyz)  (BT.h:26-28)
 *                                       guide_pv == NULL / obs == NULL mean "no guides" / "no
 *                                       obstacles" whatever the offsets say (they are not read)
 *   weights     double[B][4]         (distance, smoothness, feasibility, dynamic) per
 *                                       trajectory; NULL => the handle's params.  The rebound
 *                                       loop doubles them per trajectory (BT.cpp:667,672,678).
 * The *_mixed entries take trajectories of DIFFERENT control-point counts in one call: rows of Ns
 * control points, ctrl double[B][Ns][3], and n_pts int32[B] (device memory), the count of each;
 * guide_off is then int32[B*Ns + 1] with control point (b,i) at b*Ns + i and the control points
 * beyond a count owning empty ranges.  The fit (vigo_bspline_fit_mixed), the prologue
 * (vigo_collision_segs_mixed, vigo_path_search_mixed, vigo_guide_assign_mixed), the solves
 * (vigo_cost_grad_mixed, vigo_optimize_mixed), the rebound rounds (vigo_rebound_rounds_mixed), the
 * re-guide step (vigo_rebound_reguide_mixed) and the finish (vigo_traj_finish) pass these arrays to
 * one another as they lie.
 */
#ifndef VIGO_H
#define VIGO_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vigo_context* vigo_handle_t;

typedef enum {
    VIGO_OK = 0,
    VIGO_ERR_INVALID_ARG = -1,
    VIGO_ERR_NO_DEVICE = -2,     /* no HIP device / HIP runtime error at create      */
    VIGO_ERR_HIP = -3,           /* a HIP call failed; see vigo_last_error()          */
    VIGO_ERR_UNSUPPORTED_N = -4, /* N < 7 or N > VIGO_MAX_CTRL_POINTS                 */
    VIGO_ERR_NO_GRID = -5,       /* a map query was issued before vigo_set_grid*()    */
    VIGO_ERR_UNSUPPORTED = -6    /* parameter combination not implemented             */
} vigo_status_t;

/* vigo_optimize additionally needs its L-BFGS history in the 160 KiB LDS of a CU: for N > 128 (fp64 and fp64
 * fast) mem_size * ((N-5) * 48 + 16) B, plus the alphas and the obstacle table.  That holds N <= 216 at mem_size 16
 * (every N at mem_size <= 8, and every N in fp32); larger N returns VIGO_ERR_UNSUPPORTED_N. */
enum { VIGO_MAX_CTRL_POINTS = 256, VIGO_MAX_MEM_SIZE = 16 };

/* arithmetic mode of the solver / cost kernels */
typedef enum {
    VIGO_PREC_F64 = 0,       /* fp64 state + reductions (parity-gated default)        */
    VIGO_PREC_F32 = 1,       /* fp32 state, fp64 reductions (throughput mode)         */
    VIGO_PREC_F64_FAST = 2   /* fp64 with fused multiply-adds in dot products / axpys /
                                stencils (what GCC's default contraction does to the
                                reference on ARM) and one reciprocal per history pair
                                instead of a division per two-loop step; same 1e-4 gate  */
} vigo_precision_t;

/*
 * Parameters of the hot path.  Field comments give the reference member they mirror.
 * vigo_default_params() loads cfg/bspline_interactive/bspline_planner_param.yaml values and
 * the solver settings of BT.cpp:695-699 / LB:942-954.
 */
typedef struct vigo_params_s {
    /* cost terms */
    double dthresh;              /* dthresh_               BT.cpp:35   */
    double dist_thresh_dynamic;  /* distThreshDynamic_     BT.cpp:143  */
    double ts_ctrl;              /* controlPointsTs_ = 0.2 BT.h:47     */
    double ts;                   /* ts_ (bspline_traj/timestep) BT.cpp:26 */
    double pred_horizon;         /* predHorizon_           BT.cpp:134  */
    double uncertain_factor;     /* uncertainAwareFactor_  BT.cpp:125  */
    double w_distance;           /* weightDistance_        BT.cpp:62   */
    double w_smoothness;         /* weightSmoothness_      BT.cpp:71   */
    double w_feasibility;        /* weightFeasibility_     BT.cpp:80   */
    double w_dynamic;            /* weightDynamicObstacle_ BT.cpp:89   */
    double min_height;           /* minHeight_             BT.cpp:107  */
    double max_height;           /* maxHeight_             BT.cpp:116  */
    int32_t plan_in_z;           /* planInZAxis_           BT.cpp:98   */
    /* L-BFGS (lbfgs_parameter_t, LB:87-191) */
    int32_t mem_size;            /* BT.cpp:697 (16)  */
    int32_t max_iterations;      /* BT.cpp:698 (200); 0 (= unbounded in lbfgs.hpp) is refused */
    int32_t max_linesearch;      /* LB:948 (40)      */
    int32_t past;                /* LB:945 (0); only 0 is supported */
    int32_t strict_z;            /* 1: do NOT apply the level rule (below, at vigo_optimize): the reference's arithmetic on the z
                                    axis whatever the input.  Default 0.  (Was a reserved field: same layout.) */
    double g_epsilon;            /* BT.cpp:699 (0.01) */
    double delta;                /* LB:946 */
    double min_step;             /* LB:949 */
    double max_step;             /* LB:950 */
    double f_dec_coeff;          /* LB:951 ftol */
    double s_curv_coeff;         /* LB:952 gtol */
    double xtol;                 /* LB:953 */
} vigo_params_t;

/* ---- lifecycle ------------------------------------------------------------------- */

/* Replaces: bsplineTraj::bsplineTraj()/init() device-side state (BT.cpp:9-22). */
int vigo_create(vigo_handle_t* out, int device_ordinal);
int vigo_destroy(vigo_handle_t h);
/* Binds all later launches of this handle to a hipStream_t (NULL = default stream). */
int vigo_set_stream(vigo_handle_t h, void* hip_stream);
/* Replaces: bsplineTraj::initParam() (BT.cpp:24-172) for the hot-path subset. */
void vigo_default_params(vigo_params_t* p);
int vigo_set_params(vigo_handle_t h, const vigo_params_t* p);
int vigo_get_params(vigo_handle_t h, vigo_params_t* p);
int vigo_set_precision(vigo_handle_t h, int vigo_precision);
/* Text of the last HIP/runtime failure on this handle (never NULL). */
const char* vigo_last_error(vigo_handle_t h);
/* Library/ABI version (raised when entry points are added; nothing was removed or changed so far: 4 adds
 * vigo_build_esdf / vigo_esdf_from_voxels_host; vigo_seed_capacity / vigo_seed_paths / vigo_seed_paths_host came in at 4
 * as well, and so did vigo_bspline_fit_mixed, then vigo_traj_finish / vigo_traj_finish_host, then vigo_build_esdf_tracked / vigo_update_esdf and
 * their host twins after them — ask the library for the symbol), and whether the code object was built for gfx950. */
int vigo_abi_version(void);
const char* vigo_build_arch(void);
/* "solver:<12 hex> all:<12 hex>": digests of the library's compiled code (host code and gfx950 code objects; the first
 * over the solve kernels' objects, the second over every object).  Source edits that leave the code alone leave it alone.
 * Profiles record it, so a counter file can be told from a stale one. */
const char* vigo_build_id(void);

/* ---- voxel map ------------------------------------------------------------------- */

/*
 * Dense voxel-map contract standing in for mapManager::occMap (external package
 * map_manager, un-vendored; call sites BT.h:197,199,312,319,332, BT.cpp:292,412,435,841).
 *   voxels: uint8[nx][ny][nz] (z fastest), bit0 = inflated-occupied, bit1 = unknown,
 *           bit2 = occupied (un-inflated; used by the corridor checker's octree semantics).
 *   index  = floor((p - origin) / res) per axis; outside the box => occupied AND unknown.
 * The map is SNAPSHOTTED (packed to one bit per voxel per plane in HBM).
 * Replaces: bsplineTraj::setMap (BT.cpp:187-195), polyTrajOctomap::updateMap (PO.cpp:133-145).
 */
int vigo_set_grid(vigo_handle_t h, int nx, int ny, int nz, const double origin[3],
                  double res, const uint8_t* voxels_dev);
int vigo_set_grid_host(vigo_handle_t h, int nx, int ny, int nz, const double origin[3],
                       double res, const uint8_t* voxels_host);
/* Inflation of a byte grid on the device, before vigo_set_grid / vigo_pack_grid: bit0 (inflated-occupied)
 * := OR of bit2 (occupied) over the box |dx| <= rx, |dy| <= ry, |dz| <= rz voxels — what map_manager's
 * occMap does with the robot size (cfg/bspline_interactive/occupancy_map.yaml:9) before the planner's
 * isInflatedOccupied queries (BT.cpp:292,412,435).  In place; other bits are kept. */
int vigo_inflate_grid(vigo_handle_t h, int nx, int ny, int nz, uint8_t* voxels_dev, int rx, int ry, int rz);
/* Size in bytes of the packed snapshot for a grid of these dims (3 bit planes). */
size_t vigo_grid_packed_bytes(int nx, int ny, int nz);
/* Pack a byte grid into the snapshot format into a caller-owned device buffer (so it can
 * be broadcast with RCCL), and adopt an already packed snapshot (copy into the handle). */
int vigo_pack_grid(vigo_handle_t h, int nx, int ny, int nz, const uint8_t* voxels_dev,
                   uint32_t* packed_dev);
int vigo_set_grid_packed(vigo_handle_t h, int nx, int ny, int nz, const double origin[3],
                         double res, const uint32_t* packed_dev);
/* Metric bounds used by the corridor checker's out-of-bounds test
 * (octomap getMetricMin/Max, PO.cpp:572-577).  Default: the grid box. */
int vigo_set_metric_bounds(vigo_handle_t h, const double bmin[3], const double bmax[3]);
/* Update a box of the snapshot IN PLACE: lo = first voxel of the box in the snapshot's lattice, n = its extent,
 * voxels = uint8[n[0]][n[1]][n[2]] (z fastest) under the byte contract above.  Stream-ordered on the handle's stream;
 * the _host form stages through the handle's scratch and synchronises, like vigo_set_grid_host.
 *   inflate_r == NULL (raw): for every voxel of the box the three plane bits become bits 0, 1, 2 of its byte; no other
 *     bit of the snapshot changes (the padding of a z-row's last word stays clear).  After any sequence of raw updates
 *     the snapshot equals, word for word, vigo_set_grid of the byte grid with the boxes written into it.
 *   inflate_r = {rx, ry, rz}: planes 1 and 2 as above, bit 0 of the input bytes is ignored; bit 0 of every voxel of the
 *     box grown by r per axis (clipped to the grid) becomes the box dilation of the new occupied plane — the rule of
 *     vigo_inflate_grid, nothing outside the grid — and is kept elsewhere.  If plane 0 was the r-dilation of plane 2
 *     before the call it is so afterwards: the result of vigo_inflate_grid + vigo_set_grid on the whole updated grid,
 *     for work proportional to the box grown by 2r.
 * Untouched: grid dims, origin and res, the bounds of vigo_set_metric_bounds, the cached sample times — and the
 * handle's ESDF: a field built by vigo_build_esdf is STALE until it is built again.  After vigo_build_esdf_tracked the
 * box joins the handle's pending box instead, and vigo_update_esdf refreshes the field for work that follows the change
 * (see "ESDF region update" below).
 * Errors (nothing is written): VIGO_ERR_INVALID_ARG — NULL handle, lo, n or voxels, a negative lo, n or radius, lo + n
 * beyond the grid; VIGO_ERR_NO_GRID — before any vigo_set_grid*; VIGO_ERR_UNSUPPORTED — rz > 31 (vigo_inflate_grid's
 * limit).  An n[a] == 0 is VIGO_OK with nothing launched. */
int vigo_update_grid_region(vigo_handle_t h, const int32_t lo[3], const int32_t n[3],
                            const uint8_t* voxels_dev, const int32_t inflate_r[3]);
int vigo_update_grid_region_host(vigo_handle_t h, const int32_t lo[3], const int32_t n[3],
                                 const uint8_t* voxels_host, const int32_t inflate_r[3]);
/* Copy the handle's current snapshot (vigo_grid_packed_bytes of its dims) into a caller-owned device buffer,
 * stream-ordered: what a rank broadcasts after region updates. */
int vigo_get_grid_packed(vigo_handle_t h, uint32_t* packed_dev);
/* The host twin of vigo_update_grid_region on a byte grid uint8[nx][ny][nz], in place: no GPU, no handle; the same
 * codes for the same arguments (csrc/vigo_grid_update_core.hpp). */
int vigo_grid_region_apply_host(int nx, int ny, int nz, uint8_t* voxels_host_inout,
                                const int32_t lo[3], const int32_t n[3],
                                const uint8_t* region_voxels_host, const int32_t inflate_r[3]);

/* Point queries, Q points double[Q][3] -> uint8[Q].
 * which: 0 = isInflatedOccupied, 1 = isUnknown  (BT.cpp:412,841). */
int vigo_query_points(vigo_handle_t h, int which, int64_t Q, const double* pts,
                      uint8_t* out);
/* map_->isUnknown(guidePoint) for every guide pair (loop-invariant per solve, BT.cpp:841). */
int vigo_guides_unknown(vigo_handle_t h, int64_t G, const double* guide_pv,
                        uint8_t* out_unk);

/* ---- ViGO cost / gradient --------------------------------------------------------- */

/*
 * Replaces: bsplineTraj::costFunction (BT.cpp:802-821) = getDistanceCost (:823-932) +
 * getSmoothnessCost (:934-950) + getFeasibilityCost (:952-999) + getDynamicObstacleCost
 * (:1001-1064), evaluated for B trajectories in one launch.
 *   out_cost  double[B]            total weighted cost
 *   out_grad  double[B][N-6][3]    gradient w.r.t. the free control points (BT.cpp:819)
 *   out_terms double[B][4] or NULL un-weighted (distance, smoothness, feasibility, dynamic)
 */
int vigo_cost_grad(vigo_handle_t h, int B, int N, const double* ctrl,
                   const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                   const int32_t* obs_off, const double* obs, int n_obs_shared,
                   const double* weights,
                   double* out_cost, double* out_grad, double* out_terms);

/*
 * Replaces: bsplineTraj::optimize (BT.cpp:687-718) -> lbfgs::lbfgs_optimize (LB:1024-1349)
 * with line_search_morethuente (LB:716-937), for B trajectories in one launch.
 *   ctrl       in: initial control points; out: optData_.controlPoints as the reference
 *              leaves them, i.e. the LAST EVALUATED point (BT.cpp:803), not L-BFGS' x.
 *   out_x      double[B][N-6][3] or NULL: the x vector lbfgs_optimize returns
 *              (reverted to xp on line-search failure, LB:1192)
 *   out_status int32[B]  lbfgs_optimize return code (LB:20-80)
 *   out_fx     double[B] final objective (LB:1328)
 *   out_iters  int32[B]  iteration counter k at exit;  out_evals int32[B] cost evaluations
 *   (any out_* except ctrl may be NULL)
 *
 * THE LEVEL RULE (vigo_cost_grad, vigo_optimize, vigo_rebound_rounds; not in the reference).  With plan_in_z = 0 the
 * z coordinate of a control point feels the smoothness and feasibility terms only (BT.cpp:856-858 zeroes the guide
 * term's z gradient, BT.cpp:1022 the obstacle term's).  When all N control points of a trajectory lie at one height
 * — zmax - zmin <= 2^-40 * max(1, |zmin|, |zmax|): a level path as the least-squares fit leaves it — those two z
 * terms are differences of values that differ by rounding noise; the kernels take them as exactly zero (cost and
 * gradient), so such a trajectory's z never moves, where the reference lets it drift by that noise (measured:
 * <= 6e-14 m over 50 iterations).  The deviation is ~12 orders of magnitude inside the 1e-4 parity bar, and exact for
 * a path that is level to the bit (decided once per call, from the control points the call starts with).  What it
 * buys: waves whose trajectories are all level are solved (calls without obstacles, N <= 64) by an instantiation
 * that carries x and y only — two thirds of the L-BFGS history, of every dot product and of the stencils, and on
 * batches that fill the chip most of that history in registers, so that a CU holds eight waves instead of four
 * (-8 % at 1024 x 32, -35 % on such batches).  The rule is applied
 * per trajectory, also where a level trajectory shares a wave with one that is not: results never depend on the
 * batch a trajectory travels in.  The oracle's device-emulation mode applies the same rule; its reference-order mode
 * restates the reference and does not.  vigo_params_t.strict_z = 1 switches the rule off for a handle.
 */
int vigo_optimize(vigo_handle_t h, int B, int N, double* ctrl,
                  const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                  const int32_t* obs_off, const double* obs, int n_obs_shared,
                  const double* weights,
                  double* out_x, int32_t* out_status, double* out_fx,
                  int32_t* out_iters, int32_t* out_evals);

/*
 * Validation of the CSR lists a solve will index (they live in device memory, so vigo_optimize / vigo_cost_grad /
 * vigo_traj_dynamic_collision cannot check them per call): offsets start at 0, never decrease and end within
 * G guide pairs / O obstacles.  Synchronous (one small kernel and a 4-byte read back) — an integration-time
 * check, not part of the hot path.  guide_off / obs_off may be NULL (skipped).
 * Returns the number of violations found (0 = the lists are safe to pass), or a negative vigo_status_t.
 * No reference counterpart: the reference's vector<vector<>> cannot be inconsistent.
 */
int vigo_check_lists(vigo_handle_t h, int B, int N, const int32_t* guide_off, int64_t G,
                     const int32_t* obs_off, int64_t O);

/* ---- B-spline fit, evaluation and the rebound-loop gates --------------------------- */

/*
 * Replaces: bspline::parameterizeToBspline (BS.cpp:74-138) as bsplineTraj::updatePath calls it
 * (BT.cpp:314), for B paths of K waypoints each in one launch: least-squares solution of the
 * (K+4)x(K+2) system [1 4 1]/6 | velocity rows | acceleration rows (three colPivHouseholderQr
 * solves per path in the reference).  The factorisation depends on (K, ts) only; it is computed on
 * the device at the first call with a new (K, ts) and cached in the handle.
 *   points   double[B][K][3]   waypoints
 *   conds    double[B][4][3]   start vel, end vel, start acc, end acc (the startEndConditions order of BT.cpp:290, BS.cpp:117-121);
 *                              NULL => all zero
 *   ctrl_out double[B][K+2][3] control points (the `ctrl` layout of vigo_optimize, N = K + 2)
 * 4 <= K <= VIGO_MAX_CTRL_POINTS - 2 (the reference exit(0)s below 4 points, BS.cpp:83-87).
 */
int vigo_bspline_fit(vigo_handle_t h, int B, int K, double ts, const double* points,
                     const double* conds, double* ctrl_out);

/*
 * The same fit for T paths of DIFFERENT point counts in one call: the head of the mixed chain, its output is the
 * `ctrl double[B][Ns][3]` + `n_pts int32[B]` input of vigo_optimize_mixed / vigo_rebound_rounds_mixed.  All arrays device.
 *   n_fit     int32[T]                    waypoints K_t of path t
 *   status    int32[T] or NULL            path t is fitted only if status[t] == 0
 *   points    double[T][point_stride][3]  the first K_t rows of row t are its waypoints; nothing beyond them is read
 *   conds     double[T][4][3] or NULL     as vigo_bspline_fit
 *   ctrl_out  double[T][Ns][3]            rows 0 .. K_t+1 of row t are written, nothing beyond them
 *   out_n_pts int32[T]                    K_t + 2 for a fitted path, 0 for one that was not
 * 7 <= Ns <= 64, point_stride >= 1.  A path is fitted when 4 <= K_t <= min(Ns - 2, point_stride) and its status, if
 * given, is 0; one that is not keeps its ctrl_out row as it was.  The counts are device data and checked per path:
 * nothing is indexed with a count out of range, and every other path gets the bits it would get without it.
 * Rows 0 .. K_t+1 of a fitted path equal, value for value, what vigo_bspline_fit(h, 1, K_t, ts, ...) gives for that
 * path alone: they depend neither on its position in the batch, nor on the batch size, nor on its neighbours' counts.
 * (The handle keeps the operators of every K = 4 .. 62 at one ts, 0.7 MB, built at the first call with a new ts by the
 * arithmetic of vigo_bspline_fit's own set-up; the paths are regrouped by count on the device, so the host needs no
 * knowledge of which counts occur.)  The shape-class rule of the mixed solve entries (all counts <= 32 or all in
 * 33 .. 64) stays the solver's: the fit does not impose it.  point_stride / n_fit / status match vigo_seed_paths's
 * point_cap / out_fit_n / out_status: its out_fit is passed as it lies.
 * VIGO_ERR_INVALID_ARG: NULL handle, T < 0, point_stride < 1, ts not finite and > 0, a NULL required array with T > 0;
 * VIGO_ERR_UNSUPPORTED_N: Ns outside [7, 64]; on an error nothing is written.  T == 0: VIGO_OK, nothing launched.
 */
int vigo_bspline_fit_mixed(vigo_handle_t h, int T, int Ns, double ts, const int32_t* n_fit, const int32_t* status,
                           const double* points, int point_stride, const double* conds, double* ctrl_out,
                           int32_t* out_n_pts);

/*
 * Replaces: bspline::at (BS.cpp:32-58) on bspline(3, ctrl, ts_ctrl) and its
 * getDerivative() chains (BS.cpp:64-72).  deriv = 0,1,2.
 *   times double[T] shared by the batch; out double[B][T][3].
 */
int vigo_bspline_eval(vigo_handle_t h, int B, int N, const double* ctrl, int deriv,
                      int T, const double* times, double* out);

/*
 * Replaces: bsplineTraj::hasCollisionTrajectory (BT.h:307-325): sample the spline every
 * dt = res/max_vel/2 and test isInflatedOccupied.
 *   out_flag uint8[B]; out_first int32[B] index of the first colliding sample or -1.
 */
int vigo_traj_collision(vigo_handle_t h, int B, int N, const double* ctrl, double dt,
                        uint8_t* out_flag, int32_t* out_first);
/*
 * Replaces: bsplineTraj::hasDynamicCollisionTrajectory (BT.h:344-368).
 */
int vigo_traj_dynamic_collision(vigo_handle_t h, int B, int N, const double* ctrl, double dt,
                                const int32_t* obs_off, const double* obs, int n_obs_shared,
                                uint8_t* out_flag);
/*
 * Replaces the map queries of bsplineTraj::findCollisionSeg (BT.cpp:403-445):
 *   out_pt   uint8[B][N]  isInflatedOccupied(ctrl[i])
 *   out_line uint8[B][N]  isInflatedOccupiedLine(ctrl[i-1], ctrl[i]) (entry 0 = 0)
 * The segment bookkeeping is a serial scan of these flags: on the host in the rebound loop, on the device in
 * vigo_collision_segs / vigo_path_search.
 */
int vigo_ctrl_occupancy(vigo_handle_t h, int B, int N, const double* ctrl,
                        uint8_t* out_pt, uint8_t* out_line);

/* ---- the end of a plan: reparameterisation factor and sampled path ------------------------ */

/* out_status of vigo_traj_finish, per trajectory */
typedef enum {
    VIGO_FINISH_OK = 0,          /* everything written */
    VIGO_FINISH_CAPACITY = 1,    /* n_samp > S_cap: out_n carries the true count; the first S_cap samples and the factor are written */
    VIGO_FINISH_INVALID_N = 2    /* count outside 7 .. Ns: factor and maxima NaN, out_n = 0, no sample row touched */
} vigo_finish_status_t;

/*
 * Replaces: steps 5-6 of bsplineTraj::makePlan() — bspline_ = bspline(3, controlPoints, controlPointsTs_) and
 * linearFeasibilityReparam() (BT.cpp:1116-1137) — and the samples of evalTrajToMsg(dt) (BT.cpp:1502-1518, over evalTraj,
 * BT.h:345) for B trajectories in ONE launch, a wavefront per trajectory, on the control-point rows as
 * vigo_rebound_rounds / vigo_rebound_rounds_mixed leave them.  All arrays device.  ts_ctrl and ts are the handle's params.
 *   n_pts      int32[B] or NULL         control points n_b of row b (NULL: every row has Ns)
 *   ctrl       double[B][Ns][3]         the first n_b points of row b are read, nothing beyond them
 *   limits     double[B][2]             max_vel, max_acc of trajectory b
 *   out_factor double[B]                linearFactor_: min(max_vel / maxV, sqrt(max_acc / maxA)) by std::min's comparison, the
 *                                       maxima of |velocity| and |acceleration| over `for (t = 0; t < duration; t += ts)`,
 *                                       duration = (n_b - 3) * ts_ctrl; a NaN norm never replaces a maximum, and no division
 *                                       is guarded: +inf for a trajectory that does not move
 *   out_max    double[B][2] or NULL     maxV, maxA
 *   out_n      int32[B]                 samples of `for (t = 0; t <= duration; t += sample_dt)`
 *   out_pos    double[B][S_cap][3]      sample i: the position at the i-fold accumulated t; rows i >= out_n stay as they were
 *   out_vel    double[B][S_cap][3] or NULL   the velocity at (double)i * sample_dt — the product clock evalTrajToMsg takes
 *                                       its yaw from; atan2 and the quaternion stay with the caller (libm)
 *   out_status int32[B]                 VIGO_FINISH_*
 * Every value equals, bit for bit, what the reference's serial loops give for the trajectory alone: it depends neither on
 * the batch nor on Ns nor on the neighbours' counts.  The counts are device data and checked per trajectory.  (A NaN
 * coordinate of out_pos / out_vel is stored as the quiet NaN 0x7ff8000000000000: IEEE 754 leaves a NaN's sign and payload to
 * the implementation, and x86 and gfx950 differ there.)
 * VIGO_ERR_UNSUPPORTED_N: Ns < 7 or Ns > VIGO_MAX_CTRL_POINTS.  VIGO_ERR_INVALID_ARG: NULL handle, B < 0, S_cap < 1, a
 * sample_dt / ts / ts_ctrl that is not finite and positive, a NULL required array with B > 0, more than 2^24 samples of a
 * clock.  On an error nothing is written.  B == 0: VIGO_OK, nothing launched.  The two clock tables are cached in the handle
 * per step and longest duration, in slots of their own (the gates' table is not evicted).
 */
int vigo_traj_finish(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const double* limits,
                     double sample_dt, int S_cap, double* out_factor, double* out_max, int32_t* out_n, double* out_pos,
                     double* out_vel, int32_t* out_status);
/* The same rule on the host (csrc/vigo_finish_core.hpp compiled for the CPU; no handle, no GPU): host pointers, ts_ctrl and
 * ts as arguments, the clocks by the plain `t += step` loops.  Same refusals, same statuses, same bits. */
int vigo_traj_finish_host(double ts_ctrl, double ts, int B, int Ns, const int32_t* n_pts, const double* ctrl,
                          const double* limits, double sample_dt, int S_cap, double* out_factor, double* out_max,
                          int32_t* out_n, double* out_pos, double* out_vel, int32_t* out_status);

/* ---- the rebound loop between two A* calls, device-resident ------------------------------ */

/*
 * Replaces: the while loop of bsplineTraj::optimizeTrajectory (BT.cpp:611-685) for B trajectories, for as long as
 * a trajectory needs nothing from the host.  One round per trajectory =
 *     hasCollisionTrajectory / hasDynamicCollisionTrajectory     (BT.cpp:620-626, BT.h:307-368; the dynamic gate
 *                                                                  only when the trajectory has obstacles)
 *     neither          -> VIGO_RB_DONE                            (BT.cpp:628-631)
 *     failCount >= 4   -> VIGO_RB_NEEDS_HOST                      (forced A* re-guide, BT.cpp:640-654)
 *     static collision -> isReguideRequired (BT.cpp:573-608: findCollisionSeg :403-445 on the new control points,
 *                         comparison with the previous segments, isControlPointRequireNewGuide BT.h:417-429):
 *                         required -> VIGO_RB_NEEDS_HOST (A*, BT.cpp:656-665; nothing of the state is touched, the
 *                         host repeats the step itself); else collisionSeg_ := the new segments,
 *                         weightDistance *= 2, ++failCount      (BT.cpp:666-674)
 *     dynamic collision -> weightDynamicObstacle *= 2             (BT.cpp:677-679)
 *     optimize()                                                  (BT.cpp:680, = vigo_optimize on the still-active set,
 *                                                                  compacted on the device)
 * max_rounds rounds are queued without a host round trip; trajectories that are done or wait for the host are
 * skipped, and once a round hands a trajectory to the host the rest of the call is a no-op for the whole batch: the
 * optimize() the still-active trajectories owe is left to the next call (their solve_first is set), where it shares
 * one launch with the re-guided ones — the waiting trajectories are on the batch's critical path.  A trajectory whose state has solve_first != 0 is optimized once before its first gate (the
 * optimize() of BT.cpp:612, or the one that follows a host-side re-guide).
 *   ctrl, guide_*, obs_*       as vigo_optimize (guide_unk from vigo_guides_unknown); ctrl in/out
 *   weights   double[B][4]     in/out, REQUIRED (the loop doubles them per trajectory)
 *   gate_dt                    sample step of the gates, map_->getRes() / maxVel_ / 2 (BT.h:312)
 *   not_check_ratio            notCheckRatio_ of findCollisionSeg (BT.cpp:408; 0 in the reference)
 *   state     vigo_rebound_state_t[B] in/out (device memory)
 * Needs vigo_set_grid.  The 30 ms wall-clock budget of BT.cpp:633 stays with the caller (between calls).
 */
enum { VIGO_MAX_COLLISION_SEGS = 48 };
typedef enum { VIGO_RB_ACTIVE = 0, VIGO_RB_DONE = 1, VIGO_RB_NEEDS_HOST = 2 } vigo_rebound_status_t;
typedef struct {
    int32_t status;        /* vigo_rebound_status_t; only VIGO_RB_ACTIVE entries are worked on      */
    int32_t solve_first;   /* in: optimize before the first gate; out: an optimize() is still owed    */
    int32_t fail_count;    /* failCount, BT.cpp:613                                                 */
    int32_t gate_static;   /* out: last hasCollisionTrajectory result                               */
    int32_t gate_dynamic;  /* out: last hasDynamicCollisionTrajectory result                        */
    int32_t rounds;        /* out: += gate passes made by the call                                  */
    int32_t lbfgs_status;  /* out: lbfgs_optimize return code of the last optimize() (LB:20-80)     */
    int32_t n_seg;         /* collisionSeg_ (BT.h:73) as isReguideRequired left it: n_seg pairs     */
    int32_t seg[2 * VIGO_MAX_COLLISION_SEGS];   /* (first, second); more segments than fit -> NEEDS_HOST */
} vigo_rebound_state_t;

int vigo_rebound_rounds(vigo_handle_t h, int B, int N, double* ctrl,
                        const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                        const int32_t* obs_off, const double* obs, int n_obs_shared,
                        double* weights, double gate_dt, double not_check_ratio, int max_rounds,
                        vigo_rebound_state_t* state);

/* ---- mixed control-point counts in one batch ------------------------------------------------ */

/*
 * vigo_cost_grad, vigo_optimize and vigo_rebound_rounds for trajectories of DIFFERENT length in one call.
 *   Ns     the row stride, in control points, of every per-point array
 *   n_pts  int32[B], device memory: trajectory b has n_pts[b] control points
 * The layouts are those of the uniform entries with N replaced by Ns: ctrl double[B][Ns][3]; guide_off int32[B*Ns+1]
 * with control point i of trajectory b at b*Ns + i; out_x / out_grad double[B][Ns-6][3]; everything per trajectory
 * (obs_off, weights, state, out_cost, out_status, ...) as before.  Trajectory b uses the first n_pts[b] rows of its ctrl
 * row, and the first n_pts[b] - 6 rows of its out_x / out_grad row are written.  Nothing beyond those is read for its
 * value or written; guide_off is read at free control points only (entries b*Ns + 3 .. b*Ns + n_pts[b] - 3), as in the
 * uniform entries — by vigo_rebound_rounds_mixed, as by vigo_rebound_rounds, also at any control point a collision
 * segment names (entries b*Ns .. b*Ns + n_pts[b]).
 *
 * CONTRACT.  7 <= n_pts[b] <= Ns <= 64, and every count lies in the shape class of Ns: all <= 32 (two trajectories per
 * wavefront), or all in 33 .. 64 (one).  A trajectory then runs in exactly the lane layout and reduction tree that a
 * uniform call of its own count gives it, so EVERY OUTPUT OF A TRAJECTORY EQUALS, BIT FOR BIT, ITS OUTPUT IN A UNIFORM
 * CALL OF ITS OWN COUNT — in the three arithmetic modes, under the level rule, plan_in_z and strict_z, with and without
 * obstacles: a result depends neither on the batch a trajectory travels in nor on the lengths of its neighbours.
 * Ns < 7 or Ns > 64 returns VIGO_ERR_UNSUPPORTED_N (such callers keep grouping by exact count); NULL n_pts with B > 0
 * VIGO_ERR_INVALID_ARG.  A call is ONE launch of the general solve kernel (obstacle code, z carried and masked for a
 * level trajectory), where the uniform entries pick a cheaper kernel for level or obstacle-free batches.
 *
 * A count that breaks the contract is device data and is caught per trajectory.  Nothing beyond the row is indexed, the
 * bad trajectory's ctrl row and weights stay untouched, its wavefront partner and every other trajectory get the bits
 * they would get without it, and it is reported as
 *   vigo_optimize_mixed        out_status = LBFGSERR_INVALID_N (-1021, LB:36), nothing else written
 *   vigo_cost_grad_mixed       out_cost = NaN, no gradient rows, no terms
 *   vigo_rebound_rounds_mixed  an ACTIVE entry becomes status = VIGO_RB_NEEDS_HOST with lbfgs_status =
 *                              LBFGSERR_INVALID_N, rounds left as it was, and WITHOUT the batch-wide wait: the other
 *                              trajectories' rounds go on (the state of "the device cannot represent this planner")
 * Otherwise vigo_rebound_rounds_mixed keeps the batch-wide rule of vigo_rebound_rounds: once a round hands a
 * trajectory to the host, the optimize() every still-active trajectory owes is deferred to the next call.  The gates
 * sample each trajectory over its own duration (n_pts[b] - 3) * ts_ctrl.
 */
int vigo_cost_grad_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl,
                         const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                         const int32_t* obs_off, const double* obs, int n_obs_shared,
                         const double* weights,
                         double* out_cost, double* out_grad, double* out_terms);
int vigo_optimize_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, double* ctrl,
                        const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                        const int32_t* obs_off, const double* obs, int n_obs_shared,
                        const double* weights,
                        double* out_x, int32_t* out_status, double* out_fx,
                        int32_t* out_iters, int32_t* out_evals);
int vigo_rebound_rounds_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, double* ctrl,
                              const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                              const int32_t* obs_off, const double* obs, int n_obs_shared,
                              double* weights, double gate_dt, double not_check_ratio, int max_rounds,
                              vigo_rebound_state_t* state);

/* ---- min-snap QP and corridor collision checker ------------------------------------ */

/*
 * Replaces: polyTrajSolver::solve (PS.cpp:849-904) with constructP/constructA/constructBound
 * (:241-846), avgTimeAllocation (:125-138), updateCorridorParam (:985-1012) and the rescale to
 * un-normalised local time (:874-878) — the three per-axis QPs the reference hands to OSQP —
 * for T waypoint paths of W waypoints (W-1 degree-7 segments) each, one wavefront per path,
 * solved exactly (null-space elimination of the equality rows + dual active set on the corridor
 * boxes) instead of ADMM to eps 1e-3.
 *   waypoints  double[T][W][3]
 *   corridor   double[T][W-1]  corridor half-size per segment (0 = no boxes there,
 *                              PS.cpp:992); NULL = no corridor constraint (makePlanAddingWaypoint)
 *   conds      double[T][4][3] init vel, end vel, init acc, end acc (PS.h updateInitVel/...); NULL = 0
 *   out_coeffs double[T][W-1][3][deg+1]   == the `coeffs` layout of vigo_corridor_check (S = T*(W-1))
 *   out_knots  double[T][W]    desiredTime_ (PS.cpp:125-138)
 *   out_status int32[T]        0 solved, -1 numerical failure (coincident waypoints, > 1024 boxes, a singular
 *                              reduced Hessian: diff 5..7 where the minimiser is not unique),
 *                              -2 infeasible corridor (the reference keeps a stale solution silently)
 * deg must be 7; 2 <= W <= 11; diff/cont as polynomial/continuity degrees of cfg/planner*.yaml.
 */
int vigo_minsnap(vigo_handle_t h, int T, int W, int deg, int diff, int cont, double desired_vel,
                 double corridor_res, const double* waypoints, const double* corridor,
                 const double* conds, double* out_coeffs, double* out_knots, int32_t* out_status);

/*
 * 1 when vigo_minsnap takes paths of W waypoints at these degrees, 0 when it refuses them
 * (VIGO_ERR_UNSUPPORTED / VIGO_ERR_UNSUPPORTED_N): one wavefront holds the equality rows, at most
 * 40 free coefficients remain, and every matrix fits in 160 KiB of LDS.  Host only, needs no GPU;
 * vigo_minsnap decides with this same function.
 */
int vigo_minsnap_supported(int W, int deg, int diff, int cont);


/*
 * Replaces: polyTrajOctomap::checkCollisionTraj (PO.cpp:634-656) -> checkCollision
 * (:547-568) -> checkCollisionPoint (:571-589), fed by polyTrajSolver::getTrajectory /
 * getPose (PS.cpp:1125-1137, :1026-1056), for S independent polynomial segments.
 *   coeffs   double[S][3][deg+1]  x,y,z coefficients in un-normalised local time
 *   dur      double[S]            segment duration
 *   n_samp   int32[S]             samples per segment: t_k = k * delT[s], k < n_samp[s]
 *   delT     double[S]
 *   box[3], map_res               collision_box / map_resolution (cfg/planner_interactive.yaml)
 *   out_flag uint8[S]; out_first int32[S] first colliding sample index or -1;
 *   out_count int32[S] number of colliding samples (may be NULL)
 * Every sample's verdict is the reference walk's; how they are reached is not (csrc/vigo_corridor_core.hpp): segments of
 * more than 512 samples are cut into spans of 32 or 16 samples, and a span is decided by ONE evaluation when the kernel
 * can prove that all its samples see the same voxel keys (an interval that holds every sample's float position, taken
 * through the reference's own monotone expressions at both ends); spans it cannot decide are cut in four, and what
 * remains goes through the per-sample sweep.  The accumulated clock t += delT is reproduced exactly
 * (vigo_accumulated_time / vigo_clock_table_time below).
 * A pose at NaN or infinity (non-finite coefficients, overflow to float): the reference's lattice count
 * (int)((xmax - xmin) / map_res) is then the conversion of a NaN — undefined in C++, INT_MIN on x86, where the sweep
 * makes no pass and the pose does NOT collide.  Both entry points below follow x86 (the oracle on this host does);
 * a caller that wants such poses refused tests them itself (the host facade does: host/src/polyTrajOctomap.cpp).
 */
int vigo_corridor_check(vigo_handle_t h, int S, int deg, const double* coeffs,
                        const int32_t* n_samp, const double* delT,
                        const double box[3], double map_res,
                        uint8_t* out_flag, int32_t* out_first, int32_t* out_count);

/*
 * Replaces: polyTrajOctomap::checkCollisionTraj(trajectory, delT, collisionSeg) (PO.cpp:634-656) on the trajectory
 * polyTrajSolver::getTrajectory returns (PS.cpp:1125-1137, getPose :1026-1056), positions only, for T WHOLE trajectories
 * at once — what vigo_corridor_check (independent segments, each on its own clock) does not do.
 *   seg_off   int32[T+1]         CSR: trajectory t owns segments seg_off[t] .. seg_off[t+1]-1 (K_t of them)
 *   coeffs    double[S][3][deg+1] vigo_corridor_check's layout (segment i of trajectory t is row seg_off[t] + i)
 *   knots     double[S+T]        trajectory t's K_t + 1 time knots start at seg_off[t] + t
 *   delT      double[T]          sample step
 *   endpoint  double[T][3]       the sample getTrajectory appends (the last waypoint, path_.back())
 * (A group of vigo_minsnap outputs, [T][W-1][3][8] coefficients and [T][W] knots, concatenated, is this layout.)
 * The rules, for one trajectory with knots k[0..K]:
 *   1 clock      samples t_0 = 0, t_{j+1} = fl(t_j + delT) while t_j < k[K] (PS.cpp:1129: accumulated, not j * delT); n of them
 *   2 segment    sample j lies in the FIRST i with k[i] <= t_j <= k[i+1] (an inner knot belongs to the earlier segment) and
 *                is evaluated there at fl(t_j - k[i]) with pow as vigo_exact_pow; a t_j in no interval (t_j < k[0]) is the
 *                default pose (0, 0, 0) (PS.cpp:1026-1056)
 *   3 endpoint   sample n is the endpoint as given; its clock for attribution is t_n >= k[K] (in practice: attributed only
 *                when t_n == k[K])
 *   4 test       every pose through pose2Octomap's float cast and the box sweep (PO.cpp:547-589), as vigo_corridor_check
 *   5 blame      a colliding sample puts its segment (rule 2 on its clock) into collisionSeg; one in no interval makes the
 *                trajectory collide but blames no segment (PO.cpp:640-651)
 * Outputs (device memory, stream-ordered like the other corridor entries):
 *   out_status int32[T]  VIGO_TRAJ_* below; a rejected trajectory gets n 0, flag 0, first -1, count 0 and no segments
 *                        (the call still returns VIGO_OK)
 *   out_n      int32[T]  the length of the list getTrajectory returns: n + 1 (samples plus endpoint)
 *   out_flag   uint8[T]  checkCollisionTraj's result
 *   out_first  int32[T]  the first colliding index in that list, or -1
 *   out_count  int32[T]  colliding entries of the list (may be NULL)
 *   out_seg    uint8[S]  1 when segment s is in collisionSeg
 * A pose at NaN or infinity (fp64): does NOT collide (x86, as vigo_corridor_check); with VIGO_TRAJ_NONFINITE_COLLIDES in
 * flags it collides and is blamed like any other sample (the host facade's rule).
 * How: a thread per trajectory finds the runs of consecutive samples each segment takes (binary searches over the exact
 * clock, vigo_traj_sample_runs below) and the trajectory's clock table; the segments' runs go through vigo_corridor_check's
 * two passes with the certified spans (a workgroup per run, DESIGN.md §3.4 for the span bound on the subtracted clock);
 * a thread per trajectory reduces the runs in segment order, the leading default-pose run and the endpoint.
 * Scratch: 2.6 KB per trajectory for at most VIGO_TRAJ_CHUNK trajectories (10.6 MB; more trajectories are taken
 * VIGO_TRAJ_CHUNK at a time inside the call) plus 25 bytes per segment for all S at once — the per-segment part is NOT
 * chunked: it grows with S like the caller's own coefficient array (192 bytes per degree-7 segment), at 13 % of it.
 * Errors: as vigo_corridor_check (handle, NULLs, deg in [0, 15], the box, a grid, its origin on the key lattice).
 */
#define VIGO_TRAJ_NONFINITE_COLLIDES 1
#define VIGO_TRAJ_CHUNK 4096
enum {
    VIGO_TRAJ_OK = 0,
    VIGO_TRAJ_BAD_KNOTS = 1,     /* a knot not finite, or knots decreasing                                        */
    VIGO_TRAJ_BAD_DELT = 2,      /* delT not a finite number > 0                                                  */
    VIGO_TRAJ_STALL = 3,         /* the clock stops advancing below k[K] (the reference's loop never ends)        */
    VIGO_TRAJ_TOO_LONG = 4,      /* more than INT32_MAX - 1 samples                                               */
    VIGO_TRAJ_BAD_OFFSETS = 5    /* seg_off is not non-decreasing within [0, S]: every trajectory gets this       */
};
int vigo_traj_corridor_check(vigo_handle_t h, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                             const double* knots, const double* delT, const double* endpoint, const double box[3],
                             double map_res, int flags, int32_t* out_status, int32_t* out_n, uint8_t* out_flag,
                             int32_t* out_first, int32_t* out_count, uint8_t* out_seg);

/*
 * Replaces: polyTrajOccMap::checkCollisionTraj(trajectory, delT, collisionSeg) (PM.cpp:524-546) on the trajectory
 * polyTrajSolver::getTrajectory returns, for T whole trajectories at once: vigo_traj_corridor_check with another test.
 *   seg_off, coeffs, knots, delT, endpoint   as vigo_traj_corridor_check (vigo_minsnap output concatenated is this layout)
 * The rules: 1 clock, 2 segment, 3 endpoint and 5 blame are vigo_traj_corridor_check's, word for word (the sample at
 * fl(t_j - k[i]) with pow as vigo_exact_pow: the fp64 pose vigo_poly_sample returns); rule 4 is replaced by
 *   4' test      the fp64 pose as sampled, no float cast and no box: voxel floor((p - origin) / res) of the handle's grid
 *                (as vigo_query_points); the sample collides iff bit 0 (inflated-occupied) AND bit 1 (unknown) are both
 *                set there (PM.cpp:532, isInflatedOccupied && isUnknown).  Outside the grid every bit is set, so a pose
 *                outside collides — a NaN or infinite coordinate included (x86 and the oracle agree: no flags argument).
 *                The default pose (0, 0, 0) of samples before k[0] is tested like any other.
 * Outputs: out_status, out_n, out_flag, out_first, out_count (may be NULL), out_seg exactly as vigo_traj_corridor_check;
 * status and n of a trajectory are the same in both entries.
 * How: the first and last kernels of vigo_traj_corridor_check (csrc/vigo_traj_core.hpp); between them a wave per run of
 * samples, lanes striding the run, each pose looked up in the two bit planes, a 64-bit ballot per 64 samples for the
 * run's flag, first hit and count.  No atomics on results.
 * Scratch: vigo_traj_corridor_check's (the same layout, taken VIGO_TRAJ_CHUNK trajectories at a time).
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle, T < 0, S < 0, deg outside [0, 15], NULL arrays (out_count may be NULL;
 * coeffs and out_seg may be NULL when S = 0; every per-trajectory array when T = 0); VIGO_ERR_NO_GRID before a grid.
 * The grid origin need not lie on the key lattice (no octomap keys here).
 */
int vigo_traj_point_check(vigo_handle_t h, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                          const double* knots, const double* delT, const double* endpoint, int32_t* out_status,
                          int32_t* out_n, uint8_t* out_flag, int32_t* out_first, int32_t* out_count, uint8_t* out_seg);

/*
 * Replaces: the seed-path stage of bspline_node's replan step (src/bspline_node.cpp:317-378) between the two planners,
 * for T trajectories at once: polyTrajOccMap::getTrajectory(dt) (polyTrajOccMap.cpp:434-446, getPos
 * polyTrajSolver.cpp:1058-1078), bsplineTraj::inputPathCheck with its dt *= 0.8 retries (bsplineTraj.cpp:207-245) and the
 * map-dependent head of bsplineTraj::updatePath (bsplineTraj.cpp:247-312, adjustPathLengthDirect :754-793).
 *   seg_off, coeffs, knots   as vigo_traj_point_check (vigo_minsnap's output concatenated is this layout)
 *   duration                 double[T]  the planner's getDuration()
 *   dt0                      double[T]  the first try's dt (bsplineTraj::getInitTs())
 *   control_point_distance, max_path_length   double[T]  the planner's values
 *   prev_in_seed, prev_in_fit   double[T]  the previous path length (adjustPathLengthDirect's function-static) the seed
 *                            search / updatePath's head starts from; rule 3 takes max(prev, max_path_length)
 *   max_tries                tries of the search (replaces the reference's 50 ms of wall time); point_cap: rows of
 *                            out_seed / out_fit per trajectory
 * The rules, for one trajectory with knots k[0..K] (csrc/vigo_seed_core.hpp):
 *   1 clock    t_0 = 0, t_{j+1} = fl(t_j + dt), kept while t_j <= duration (inclusive; no endpoint is appended)
 *   2 sample   getPos(min(t_j, duration)): the first i with k[i] <= t <= k[i+1], local time fl(t - k[i]), the terms summed
 *              in d = 0..deg order, pow as vigo_exact_pow; a t in no interval gives (0, 0, 0)
 *   3 adjust   adjustPathLengthDirect: the list ends after the first pair whose end lies at least max(prev,
 *              max_path_length) from the first point (straight-line distance), whose line is free and which follows a
 *              free stretch of at least 1.5 (an occupied line resets the stretch); prev becomes the last distance looked
 *              at.  Lines: the ends, then int(dist / res) - 1 interior steps, on bit plane 0 of the handle's grid
 *   4 spacing  a consecutive distance of the adjusted list above 1.5 * control_point_distance fails the try:
 *              dt = fl(dt * 0.8), prev carried over, the next try
 *   5 thin     a point is kept when at least 0.8 * control_point_distance from the last kept one, the last kept point is
 *              repeated once: the seed.  final_time = (adjusted_count - 1) * dt
 *   6 head     the seed's last pose inflated-occupied: refused; rule 3 on the seed from prev_in_fit; fewer than 4 points:
 *              fillPath on the seed (2 poses -> 4 points, 3 -> 5, 4 or more -> the seed whole)
 * Outputs per trajectory: out_status (VIGO_SEED_*), out_tries, out_dt (after a failed try it is already shrunk:
 * dt0 * 0.8^tries for VIGO_SEED_NO_SPACING), out_final_time, out_seed_n and out_seed[t][point_cap][3] (the seed:
 * adjustedInputPolyTraj), out_fit_n and out_fit[t][point_cap][3] (the curve-fit points), out_prev_seed / out_prev_fit
 * (prev after the search / after the head).  VIGO_SEED_DEFERRED writes the status only; VIGO_SEED_BAD_INPUT zero
 * counts, dt0 and the prev values as given.
 * How: a wavefront per trajectory, samples and per-pair line flag / step / distance by the lanes into LDS, rule 3 and 5
 * by one lane, rule 4 a wave-wide any.  No atomics.  vigo_seed_capacity: the samples of one try LDS holds.
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle, T < 0, S < 0, deg outside [0, 15], max_tries < 1, point_cap < 0, NULL
 * arrays (coeffs may be NULL when S = 0; every per-trajectory array when T = 0; out_seed / out_fit when point_cap = 0);
 * VIGO_ERR_NO_GRID before a grid.  On an error nothing is written.
 */
enum {
    VIGO_SEED_OK = 0,
    VIGO_SEED_NO_SPACING = 1,    /* every try failed rule 4: the seed is empty                                    */
    VIGO_SEED_GOAL_OCCUPIED = 2, /* rule 6: the seed is returned, no fit points                                   */
    VIGO_SEED_TOO_SHORT = 3,     /* a seed of at most one pose (no sample: duration < 0)                          */
    VIGO_SEED_DEFERRED = 4,      /* a try beyond vigo_seed_capacity, or a list beyond point_cap: the host's       */
    VIGO_SEED_BAD_INPUT = 5      /* offsets outside [0, S]; a knot, dt0 or duration not finite; dt0 <= 0; a stalled clock */
};
int vigo_seed_capacity(int32_t* max_samples);
int vigo_seed_paths(vigo_handle_t h, int T, int S, int deg, const int32_t* seg_off, const double* coeffs, const double* knots,
                    const double* duration, const double* dt0, const double* control_point_distance,
                    const double* max_path_length, const double* prev_in_seed, const double* prev_in_fit, int max_tries,
                    int point_cap, int32_t* out_status, int32_t* out_tries, double* out_dt, double* out_final_time,
                    int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit, double* out_prev_seed,
                    double* out_prev_fit);
/* The same rules on the CPU, no GPU and no handle: HOST arrays, the map a dense byte grid voxels_host[nx][ny][nz] (bit 0
 * inflated-occupied, outside occupied) with its origin and resolution.  pow_mode 0: the kernels' correctly rounded power
 * (bit for bit vigo_seed_paths); 1: libm's pow, the facade's.  cap: the sample capacity (<= 0: vigo_seed_capacity's).
 * Returns VIGO_OK or VIGO_ERR_INVALID_ARG (also for a grid axis < 1, a resolution not finite and > 0, pow_mode not 0 / 1). */
int vigo_seed_paths_host(int nx, int ny, int nz, const double origin[3], double res, const uint8_t* voxels_host, int pow_mode,
                         int cap, int T, int S, int deg, const int32_t* seg_off, const double* coeffs, const double* knots,
                         const double* duration, const double* dt0, const double* control_point_distance,
                         const double* max_path_length, const double* prev_in_seed, const double* prev_in_fit, int max_tries,
                         int point_cap, int32_t* out_status, int32_t* out_tries, double* out_dt, double* out_final_time,
                         int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit, double* out_prev_seed,
                         double* out_prev_fit);

/*
 * Replaces: AStar::AstarSearch + AStar::getPath (path_search/astarOcc.cpp:120-244, astarOcc.h:41-85) for Q independent
 * searches on the handle's grid snapshot: bit plane 0 (inflated-occupied) of voxel floor((p - origin) / res), outside the
 * grid occupied, as vigo_query_points.
 *   start, end   double[Q][3]   the two points handed to AstarSearch
 *   step         the lattice spacing (the caller's map resolution); pool[3] (HOST pointer) the node pool's extent,
 *                2 * int(max_obstacle_size / res) per axis in the reference (BT.cpp:187-195); min/max_height the band
 * The rules of one search are those of the reference, statement by statement: the lattice centred on (start + end) / 2
 * with index (int)((p - centre) / step + 0.5) + pool / 2; an end whose node is occupied walks away from the other end a
 * step at a time until it is free (or leaves the pool: not found); the diagonal heuristic times 1 + 1/10000; the open
 * set a binary heap with libstdc++'s push_heap / pop_heap ordered by the nodes' CURRENT f; the goal test when a node is
 * popped; neighbours in dx, dy, dz order, nodes on the pool's border never entered; one push per node; a better path to
 * an open node rewrites its g and parent where it sits in the heap.  Instead of the reference's 0.2 s wall clock a
 * search has budgets: at most max_expansions pops, and the kernels' node table and heap (vigo_astar_capacity).
 *   out_status  int32[Q]   VIGO_ASTAR_FOUND      out_len points in out_path, exactly getPath()'s, start side first
 *                          VIGO_ASTAR_NOT_FOUND  an end outside the pool (adjustEnds false), or the open set ran empty
 *                          VIGO_ASTAR_DEFERRED   a budget ran out: NO result either way — run the host search.  The
 *                                                device never returns a path the host would not return.
 *                          VIGO_ASTAR_PATH_TOO_LONG  found, but out_len > path_cap points: none written
 *   out_len     int32[Q]   path points (0 unless found / too long)
 *   out_path    double[Q][path_cap][3]
 *   out_stats   int32[Q][3] or NULL: nodes popped, nodes pushed (the table's entries), the heap's largest size — of a
 *               search that was not deferred, the host search's own counts
 * A search's result does not depend on the batch it is in.
 * How: one wavefront per search, table and heap in LDS; pop and sift on lane 0, the 26 neighbours of an expansion probed
 * by 26 lanes (table, height band, map bit), then committed in the reference's order by lane 0.  Every search runs with
 * a 2048-slot table first (five per CU); the ones that overflow it run again with 8192 slots (one per CU) in a second
 * kernel of the same call.  Plain vector stores, no atomics.
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle or array (out_stats may be NULL; every array when Q = 0), Q < 0, a pool
 * axis < 3, step not finite or <= 0, path_cap < 2, max_expansions < 0; VIGO_ERR_UNSUPPORTED for a pool axis above
 * VIGO_ASTAR_MAX_POOL_AXIS (node keys hold 10 bits per axis); VIGO_ERR_NO_GRID before a grid.  Q = 0 is a no-op.
 */
enum { VIGO_ASTAR_FOUND = 0, VIGO_ASTAR_NOT_FOUND = 1, VIGO_ASTAR_DEFERRED = 2, VIGO_ASTAR_PATH_TOO_LONG = 3 };
enum { VIGO_ASTAR_MAX_POOL_AXIS = 1024 };
int vigo_astar_search(vigo_handle_t h, int Q, const double* start, const double* end, double step, const int32_t pool[3],
                      double min_height, double max_height, int max_expansions, int path_cap, int32_t* out_status,
                      int32_t* out_len, double* out_path, int32_t* out_stats);
/* The largest search vigo_astar_search holds: pushed nodes and open-set entries (host utility, no GPU). */
int vigo_astar_capacity(int32_t* max_nodes, int32_t* max_heap);

/*
 * Replaces: bsplineTraj::assignGuidePointsSemiCircle (BT.cpp:517-571) with shortcutPaths / shortcutPath (BT.h:206-257),
 * checkCollisionLine (BT.h:196-204) and findGuidePointSemiCircle (BT.h:251-304) for B trajectories of N control points
 * on the handle's grid snapshot (bit plane 0, outside the grid occupied, as vigo_query_points; the line checks walk
 * a += res with the snapshot's res).
 *   ctrl      double[B][N][3]
 *   seg_off   int32[B+1]   CSR of collision segments per trajectory
 *   seg       int32[S][2]  (first, second), AFTER pathSearch's merges; the caller applies the reference's
 *                          min(collisionSeg.size(), paths.size()) bound: segment k goes with path k
 *   path_off  int32[S+1]   CSR of path points per segment
 *   path      double[P][3] paths as pathSearch leaves them: point 0 = ctrl[first], ctrl[second] appended
 *   out_guide_off int32[B*N+1]     CSR of the pairs THIS step appends, per control point, in push order
 *   out_guide_pv  double[pair_cap][6]  (point, direction)
 *   out_guide_unk uint8[pair_cap] or NULL: isUnknown(point), as vigo_guides_unknown
 *   out_status    int32[B]  VIGO_GUIDE_OK | VIGO_GUIDE_DEFERRED: a path of the trajectory has more points than the
 *                           kernel's buffer (vigo_guide_capacity); the trajectory owns NO pairs — run the host step.
 *                           The device never returns pairs the host twin of its code would not return.
 * The rules are the reference's, statement by statement, quirks included: the guide point of a control point whose
 * search fails is the previous one (zero for the very first), carried across control points and segments; a segment
 * without interior points pushes one pair onto each of first-1 .. second+1 inside [3, N-4]; interior points outside
 * [0, N) are skipped; a zero guidePoint - controlPoint gives a NaN direction.  The angle is atan2(|a x b|, a . b) with
 * a portable fp64 atan2 (csrc/vigo_guide_core.hpp: vigo_atan2, within 2 ulp of libm's), so pairs equal those of the same
 * header compiled for the host bit for bit, and those of the reference's libm arithmetic up to that difference.
 * A trajectory's pairs do not depend on the batch it is in.
 * How: the pair counts follow from the segments alone, so a one-workgroup kernel checks the lists and scans the
 * offsets; its verdict is read back before anything else runs.  Then one wavefront per trajectory, path and shortcut
 * in LDS; line-check samples, bracket tests and bisection steps spread over the lanes with ballots; pairs written in
 * place with plain vector stores, no atomics.
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle or array (out_guide_unk may be NULL; every array when B = 0), B < 0,
 * N < 1, pair_cap < 0, offsets that decrease or start below 0, a segment with an empty path, a segment without
 * interior points whose ends are not in [0, N), indices beyond +-2^24, and more pairs than pair_cap — in every such
 * case nothing is written; VIGO_ERR_NO_GRID before a grid.  B = 0 is a no-op.
 */
enum { VIGO_GUIDE_OK = 0, VIGO_GUIDE_DEFERRED = 1 };
int vigo_guide_assign(vigo_handle_t h, int B, int N, const double* ctrl, const int32_t* seg_off, const int32_t* seg,
                      const int32_t* path_off, const double* path, int64_t pair_cap, int32_t* out_guide_off,
                      double* out_guide_pv, uint8_t* out_guide_unk, int32_t* out_status);
/* The longest path (points of one segment) vigo_guide_assign holds (host utility, no GPU). */
int vigo_guide_capacity(int32_t* max_path_points);

/*
 * Replaces: bsplineTraj::findCollisionSeg (BT.cpp:403-445) for B trajectories of N control points on the handle's grid
 * snapshot — the segment bookkeeping that vigo_ctrl_occupancy leaves to the host.
 *   ctrl             double[B][N][3]
 *   not_check_ratio  the planner's notCheckRatio_, in [0, 1]
 *   out_seg_off      int32[B+1]        CSR of the segments per trajectory
 *   out_seg          int32[seg_cap][2] (first, second) in the order the reference pushes them
 *   out_status       int32[B]          VIGO_PATHS_OK | VIGO_PATHS_DEFERRED: more than VIGO_MAX_COLLISION_SEGS segments;
 *                                      the trajectory owns none — run the host step
 * The rules are the reference's: control points 3 .. endIdx = int((N - 4) - not_check_ratio * (N - 6)) in order; a run of
 * occupied points opens a segment at the point before it and closes it at the first free point; an occupied point at
 * endIdx - 1 pushes (start, N - 1) — and when the point at endIdx is free the same start is pushed again, closed there:
 * the duplicate is kept; two neighbouring free points whose line is occupied push (i - 1, i).  Point and line tests are
 * vigo_ctrl_occupancy's (isInflatedOccupied / isInflatedOccupiedLine of the dense map contract).
 * How: vigo_ctrl_occupancy's kernel for the flags, a one-workgroup kernel that counts and scans (its verdict is read
 * back before anything is written), then one thread per trajectory repeats the scan and writes in place.
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle or array (every array when B = 0), B < 0, N < 7, seg_cap < 0 or too
 * small, not_check_ratio outside [0, 1] — nothing is written; VIGO_ERR_NO_GRID before a grid.  B = 0 is a no-op.
 */
enum { VIGO_PATHS_OK = 0, VIGO_PATHS_FAILED = 1, VIGO_PATHS_DEFERRED = 2 };
int vigo_collision_segs(vigo_handle_t h, int B, int N, const double* ctrl, double not_check_ratio, int32_t* out_seg_off,
                        int32_t* out_seg, int64_t seg_cap, int32_t* out_status);

/*
 * Replaces: bsplineTraj::pathSearch (BT.cpp:447-514) — the A* search per collision segment, the second-choice search to
 * the next segment's end, searchedPath[0] = pStart, push_back(pEnd) and the merge bookkeeping — for B trajectories, on
 * the segments of vigo_collision_segs(ctrl, not_check_ratio) when seg_off == seg == NULL, or on a caller's list
 * (seg_off int32[B+1], seg int32[S][2], ends in [0, N): the re-guide step of the rebound loop searches a subset).
 *   step, pool (HOST pointer), min/max_height, max_expansions, search_path_cap   the searches, as vigo_astar_search
 *   out_status    int32[B]  VIGO_PATHS_OK        segments and paths are the host's, bit for bit
 *                           VIGO_PATHS_FAILED    the reference's "Path Search Error. Force return.": a search failed
 *                                                and so did its second choice (or there was none); no segments, no paths
 *                           VIGO_PATHS_DEFERRED  a search the walk consulted came back VIGO_ASTAR_DEFERRED or
 *                                                VIGO_ASTAR_PATH_TOO_LONG, or the trajectory has more than
 *                                                VIGO_MAX_COLLISION_SEGS segments: no segments, no paths — run the host
 *                                                steps.  The device never returns what the host would not return.
 *   out_seg_off   int32[B+1], out_seg int32[seg_cap][2], out_path_off int32[seg_cap+1], out_path double[point_cap][3]:
 *                 exactly vigo_guide_assign's seg_off / seg / path_off / path — the segments AFTER the merges with the
 *                 reference's min(collisionSeg.size(), paths.size()) bound applied, path k the k-th path pushed.  Entries
 *                 of out_path_off beyond the call's segments + 1 are not written.
 *   out_counts    int32[B][2] or NULL: the searches run for the trajectory, and how many of them came back FOUND or
 *                 NOT_FOUND
 * The rules, quirks included: a path is the search's points with point 0 replaced by ctrl[first] and ctrl[second]
 * appended; when segment i's search fails and the next segment starts at most 2 after its end, the search runs again to
 * the next segment's end, the next segment is skipped and i is a merge; once ONE merge is taken the segments become the
 * merged pairs (first of i, second of i + 1) ALONE — the unmerged ones are dropped while their paths stay, so segment k
 * then goes with path k by position.  A second-choice search runs for every failed, eligible segment before the walk;
 * one the walk does not consult does not change the status.  A trajectory's result does not depend on its batch.
 * How: the kernels of vigo_collision_segs; every first-choice search in one vigo_astar_search launch; a one-workgroup
 * kernel lists the second-choice searches; those in a second launch; a one-workgroup kernel walks each trajectory and
 * scans segments and points; one wavefront per trajectory then compacts the searches' fixed-stride paths into the CSR
 * output, a point per lane.  Three small reads come back in between (search counts, the totals held against seg_cap and
 * point_cap); segments, ends and paths stay on the device.  Plain vector stores, no atomics.
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle or array (out_counts may be NULL; seg_off and seg both or neither;
 * every array when B = 0), B < 0, N < 7, offsets that decrease or start below 0, a segment end outside [0, N), seg_cap or
 * point_cap negative or too small, not_check_ratio outside [0, 1] when the segments are scanned, and vigo_astar_search's
 * checks of pool, step, search_path_cap and max_expansions (VIGO_ERR_UNSUPPORTED for a pool axis above
 * VIGO_ASTAR_MAX_POOL_AXIS) — in every such case nothing is written; VIGO_ERR_NO_GRID before a grid.  B = 0 is a no-op.
 */
int vigo_path_search(vigo_handle_t h, int B, int N, const double* ctrl, const int32_t* seg_off, const int32_t* seg,
                     double not_check_ratio, double step, const int32_t pool[3], double min_height, double max_height,
                     int max_expansions, int search_path_cap, int64_t seg_cap, int64_t point_cap, int32_t* out_status,
                     int32_t* out_seg_off, int32_t* out_seg, int32_t* out_path_off, double* out_path, int32_t* out_counts);

/* ---- the re-guide step of the rebound loop ------------------------------------------------ */

/*
 * Replaces: the `if (hasCollision)` block of bsplineTraj::optimizeTrajectory's loop (BT.cpp:656-679) for the
 * trajectories vigo_rebound_rounds left VIGO_RB_NEEDS_HOST because isReguideRequired (BT.cpp:573-608) said yes: the
 * re-guide segment list, vigo_path_search on that list, vigo_guide_assign on its output, the new pairs appended to the
 * trajectory's guide lists, and the state transition — so that the next vigo_rebound_rounds call takes ctrl, the merged
 * CSR, weights and state as they are.  The rules are csrc/vigo_reguide_core.hpp.
 * Trajectory b is worked on when state[b].status == VIGO_RB_NEEDS_HOST, gate_static != 0 and fail_count < 4; every
 * other one is VIGO_REGUIDE_SKIPPED: its pairs are copied unchanged, its state is not touched.  The forced A* of
 * failCount >= 4 (BT.cpp:640-654) STAYS WITH THE HOST: it precedes isReguideRequired and changes the guides that step
 * reads.  So does the 30 ms budget of BT.cpp:633.
 *   ctrl, guide_off / guide_pv / guide_unk   the current control points and guide CSR as vigo_rebound_rounds takes them
 *                       (all three guide arrays NULL: no guides; guide_unk alone NULL: the flags of the old pairs are
 *                       queried from the snapshot)
 *   weights             double[B][4] in/out
 *   not_check_ratio     as vigo_rebound_rounds; dthresh of isControlPointRequireNewGuide is the handle's parameter
 *   step .. search_path_cap   as vigo_path_search
 *   state               vigo_rebound_state_t[B] in/out
 *   out_guide_off int32[B*N+1], out_guide_pv double[pair_cap][6], out_guide_unk uint8[pair_cap] (may be NULL)
 *                       the MERGED CSR: per control point the old pairs, then the pairs this step pushed, in push order
 *   out_path_seg_off int32[B+1], out_path_off int32[seg_cap+1], out_path double[point_cap][3]   (NULL together)
 *                       astarPaths_ of the step as vigo_path_search returns paths: of every trajectory whose search
 *                       succeeded (the VIGO_REGUIDE_DONE ones, and those the guide step then deferred or whose
 *                       merges were cut, which the caller ignores — but seg_cap and point_cap must hold them too:
 *                       size both for every eligible trajectory, or the call is VIGO_ERR_INVALID_ARG)
 *   out_status int32[B] VIGO_REGUIDE_DONE          collisionSeg_ (state.seg, n_seg) = the new segments, guides appended
 *                       VIGO_REGUIDE_SEARCH_FAILED the new segments, guides unchanged, weights[0] *= 2, ++fail_count
 *                       VIGO_REGUIDE_NOT_REQUIRED  an empty list (a caller-made state): the same transition
 *                         — these three: gate_dynamic != 0 -> weights[3] *= 2; status = VIGO_RB_ACTIVE; solve_first = 1
 *                       VIGO_REGUIDE_DEFERRED      the search or the guide step deferred the trajectory, its merges
 *                                                  left more paths than segments, or there are more than
 *                                                  VIGO_MAX_COLLISION_SEGS new segments: state untouched (it stays
 *                                                  NEEDS_HOST), pairs copied unchanged — run the host step
 *                       VIGO_REGUIDE_SKIPPED       not eligible
 * A trajectory's result does not depend on its batch.  The call synchronises with the host for the counts
 * vigo_path_search and vigo_guide_assign read (three and one) and for the merged total (one).
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle or array (the guide inputs, out_guide_unk and the path outputs as
 * above; every array when B = 0), B < 0, N < 7, negative or too small pair_cap / seg_cap / point_cap, guide offsets that
 * decrease or start below 0, not_check_ratio outside [0, 1], the checks of vigo_path_search on pool, step,
 * search_path_cap and max_expansions (VIGO_ERR_UNSUPPORTED for a pool axis above VIGO_ASTAR_MAX_POOL_AXIS or more than
 * 2^20 trajectories; VIGO_ERR_UNSUPPORTED_N above VIGO_MAX_CTRL_POINTS) — in every such case nothing is written;
 * VIGO_ERR_NO_GRID before a grid.  B = 0 is a no-op.
 */
enum { VIGO_REGUIDE_DONE = 0, VIGO_REGUIDE_SEARCH_FAILED = 1, VIGO_REGUIDE_NOT_REQUIRED = 2, VIGO_REGUIDE_DEFERRED = 3, VIGO_REGUIDE_SKIPPED = 4 };
int vigo_rebound_reguide(vigo_handle_t h, int B, int N, const double* ctrl,
                         const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                         double* weights, double not_check_ratio, double step, const int32_t pool[3],
                         double min_height, double max_height, int max_expansions, int search_path_cap,
                         vigo_rebound_state_t* state, int64_t pair_cap, int32_t* out_guide_off,
                         double* out_guide_pv, uint8_t* out_guide_unk, int64_t seg_cap, int64_t point_cap,
                         int32_t* out_path_seg_off, int32_t* out_path_off, double* out_path, int32_t* out_status);

/* ---- prologue and re-guide for mixed control-point counts ---------------------------------- */

/*
 * vigo_collision_segs, vigo_path_search, vigo_guide_assign and vigo_rebound_reguide for a batch whose trajectories have
 * DIFFERENT control-point counts, in the layouts of vigo_bspline_fit_mixed / vigo_optimize_mixed /
 * vigo_rebound_rounds_mixed, so that every array passes between those calls and these as it lies:
 *   Ns        the row stride, 7 .. VIGO_MAX_CTRL_POINTS (no shape-class rule: nothing here depends on a lane layout)
 *   n_pts     int32[B] in DEVICE memory: trajectory b has n_pts[b] control points, 7 .. Ns
 *   ctrl      double[B][Ns][3]; rows are padded.  The control points i >= n_pts[b] are never read for their value: they
 *             may hold anything, NaN included
 *   guide CSRs (out_guide_off of vigo_guide_assign_mixed; guide_off and out_guide_off of vigo_rebound_reguide_mixed)
 *             int32[B*Ns+1], control point i of trajectory b at b*Ns + i.  In every CSR these calls write, the control
 *             points i >= n_pts[b] own an EMPTY range, so the output is a valid CSR over all B*Ns+1 entries and
 *             vigo_optimize_mixed / vigo_rebound_rounds_mixed take it unchanged
 *   segment and path CSRs   per trajectory and per segment, as in the uniform entries
 * Every other argument is its uniform sibling's.
 * Contract: every output of a trajectory — segments in push order with the duplicate-segment quirk, search counts,
 * paths, pairs per control point in push order, unknown flags, statuses; for the re-guide state, weights and the merged
 * CSR — equals, bit for bit, its output in the uniform call of its own count on it alone.  A result does not depend on
 * the batch, on the neighbours' counts or on what lies in a row beyond the count.  The count is the trajectory's own
 * wherever the reference's rules name N: endIdx and the closing segment (start, N - 1) of findCollisionSeg, the
 * [3, N - 4] clip and the [0, N) skip of the guide pushes, the rules of the re-guide list, the end-in-range checks of a
 * caller's segments.
 * A count outside [7, Ns] is device data and is caught per trajectory, as vigo_rebound_rounds_mixed does: nothing beyond
 * the row is indexed, every other trajectory gets the bits it would get without it, and the trajectory itself reads
 *   vigo_collision_segs_mixed, vigo_path_search_mixed   VIGO_PATHS_DEFERRED, no segments, no searches (out_counts 0, 0)
 *   vigo_guide_assign_mixed                             VIGO_GUIDE_DEFERRED, no pairs
 *   vigo_rebound_reguide_mixed                          VIGO_REGUIDE_DEFERRED, state untouched
 * (the segments a caller supplies for such a trajectory are not held against a count; offsets must still not decrease).
 * The merged CSR of the re-guide copies the old pairs of every (b, i) unchanged, whatever the count.
 * How: the uniform entries' kernels — there is one copy of each; the uniform entries run them with n_pts == NULL.  The
 * count check is part of the one-workgroup count-and-scan kernels whose verdicts are read back anyway: a call
 * synchronises with the host exactly as often as its uniform sibling.
 * Errors: those of the uniform entry with N replaced by Ns, and nothing is written in any such case; Ns outside
 * [7, VIGO_MAX_CTRL_POINTS] is VIGO_ERR_UNSUPPORTED_N; n_pts == NULL with B > 0 is VIGO_ERR_INVALID_ARG; for the re-guide
 * guide_off must not decrease over all B*Ns+1 entries.  B = 0 is a no-op.
 */
int vigo_collision_segs_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, double not_check_ratio,
                              int32_t* out_seg_off, int32_t* out_seg, int64_t seg_cap, int32_t* out_status);
int vigo_path_search_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off,
                           const int32_t* seg, double not_check_ratio, double step, const int32_t pool[3], double min_height,
                           double max_height, int max_expansions, int search_path_cap, int64_t seg_cap, int64_t point_cap,
                           int32_t* out_status, int32_t* out_seg_off, int32_t* out_seg, int32_t* out_path_off, double* out_path,
                           int32_t* out_counts);
int vigo_guide_assign_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off,
                            const int32_t* seg, const int32_t* path_off, const double* path, int64_t pair_cap,
                            int32_t* out_guide_off, double* out_guide_pv, uint8_t* out_guide_unk, int32_t* out_status);
int vigo_rebound_reguide_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl,
                               const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                               double* weights, double not_check_ratio, double step, const int32_t pool[3],
                               double min_height, double max_height, int max_expansions, int search_path_cap,
                               vigo_rebound_state_t* state, int64_t pair_cap, int32_t* out_guide_off,
                               double* out_guide_pv, uint8_t* out_guide_unk, int64_t seg_cap, int64_t point_cap,
                               int32_t* out_path_seg_off, int32_t* out_path_off, double* out_path, int32_t* out_status);

/* Rules 1-3 of vigo_traj_corridor_check for one trajectory, on the host (no GPU), with the very code its first kernel
 * runs: knots double[K+1] -> status (VIGO_TRAJ_OK .. VIGO_TRAJ_TOO_LONG; VIGO_ERR_INVALID_ARG for NULLs or K < 0) and
 *   run_first, run_len  int32[K]  segment i's samples are run_first[i] .. run_first[i] + run_len[i] - 1
 *   *n_total            n + 1, the list length (0 on rejection)
 * Samples 0 .. run_first[0] - 1 (all n when K = 0) precede k[0]: the leading default-pose run. */
int vigo_traj_sample_runs(int K, const double* knots, double delT, int32_t* run_first, int32_t* run_len, int32_t* n_total);

/*
 * Replaces: polyTrajOctomap::checkCollision(point3d) (PO.cpp:547-568) for M already-sampled
 * poses, as the reference's checkCollisionTraj(trajectory, ...) overloads use it (PO.cpp:619-656).
 *   pts double[M][3] (cast to float like pose2Octomap); out uint8[M].
 */
int vigo_box_collision_points(vigo_handle_t h, int64_t M, const double* pts, const double box[3],
                              double map_res, uint8_t* out);

/*
 * Replaces: polyTrajSolver::getTrajectory (PS.cpp:1125-1137) -> getPose (PS.cpp:1026-1056), positions only,
 * for S independent polynomial segments: the sampler vigo_corridor_check runs internally, on its own.
 *   coeffs, n_samp, delT as in vigo_corridor_check; sample k of segment s is written at index s * stride + k
 *   (samples k >= stride are not produced);
 *   out_pos     double[S][stride][3] or NULL   x, y, z as getPose returns them
 *   out_pos_f32 float [S][stride][3] or NULL   the same after pose2Octomap's cast to octomap::point3d (PO.cpp:634-656)
 * pow(t, d) of PS.cpp:1035-1039 is evaluated as the correctly rounded power (see vigo_exact_pow below).
 */
int vigo_poly_sample(vigo_handle_t h, int S, int deg, const double* coeffs, const int32_t* n_samp,
                     const double* delT, int stride, double* out_pos, float* out_pos_f32);

/* The reference's sample clock: t_k of `for (t = 0; ...; t += delT)` (PS.cpp:1129), i.e. the
 * k-fold floating-point accumulation, evaluated in closed form (host utility, no GPU). */
double vigo_accumulated_time(double delT, int64_t k);

/* The same clock through the table vigo_corridor_check builds once per segment (csrc/vigo_exact_time.hpp: one piece
 * per run of equal increments, a binary search per lookup): t_k for 0 <= k <= k_last from the table made for k_last,
 * or NaN when the kernel would build none (delT outside [2^-1000, 1e300), more than 128 pieces) and fall back to
 * vigo_accumulated_time.  Host utility for the tests (no GPU): must equal vigo_accumulated_time(delT, k) bit for bit. */
double vigo_clock_table_time(double delT, int64_t k_last, int64_t k);

/* pow(t, d) of polyTrajSolver::getPose (PS.cpp:1035-1039) for an integer 0 <= d <= 15 as the sampler kernels
 * evaluate it: the CORRECTLY ROUNDED power (libm's pow returns it or its neighbour, depending on the libm
 * build).  Host utilities, no GPU:
 *   vigo_exact_pow          the kernels' two-tier evaluation (NaN for d outside [0, 15]);
 *   vigo_exact_pow_dd       its first tier alone — the running double-double product — and whether that tier
 *                           could certify the rounding (*ambiguous = 0) or defers to the second;
 *   vigo_exact_pow_integer  its second tier alone: exact integer arithmetic, rounded once. */
double vigo_exact_pow(double t, int d);
double vigo_exact_pow_dd(double t, int d, int* ambiguous);
double vigo_exact_pow_integer(double t, int d);

/* ---- ESDF trilinear query (config 5; no reference counterpart) -------
 * vigo_set_esdf copies the row-major float lattice dist_dev[nx][ny][nz] (device memory) into the handle's own layout
 * (one 128-B line per group of 1x3x3 trilinear cells): 3.56x the lattice's bytes of device memory, stream-ordered, the caller's
 * buffer is not referenced afterwards.  nx, ny, nz >= 2. */

int vigo_set_esdf(vigo_handle_t h, int nx, int ny, int nz, const double origin[3],
                  double res, const float* dist_dev);
int vigo_esdf_query(vigo_handle_t h, int64_t Q, const double* pts,
                    double* out_dist, double* out_grad);
/* The same query at the I/O width SURVEY.md §8(d) config 5 states for the fp32 lattice: pts float[Q][3] in (12 B),
 * out float[Q][4] = {distance, d/dx, d/dy, d/dz} out (16 B, 16-byte aligned), all arithmetic in fp32, every operation
 * rounded once: u = (p - (float)origin) * inv_res - 0.5f with inv_res = 1.0f / (float)res, floorf, clamps, the blend
 * x then y then z, gradient differences * inv_res.  Own definition (no reference counterpart); oracle twin
 * vgo_esdf_query_f32.  Differs from the fp64 entry by fp32 rounding only (~1e-6 relative). */
int vigo_esdf_query_f32(vigo_handle_t h, int64_t Q, const float* pts, float* out_dist_grad);

/* ---- ESDF build (no reference counterpart) --------------------------
 * vigo_build_esdf builds the signed Euclidean distance field of the handle's current voxel snapshot on the device and
 * installs it as the handle's ESDF (what vigo_set_esdf does with a finished lattice): dims, origin and res are the
 * grid's, any earlier field is replaced, vigo_esdf_query* read it from then on.  Stream-ordered on the handle's stream;
 * the workspace (8 bytes per voxel) belongs to the handle, grows on demand and is freed by vigo_destroy.
 *   plane            0 = inflated-occupied, 2 = occupied: the SITES are the voxels whose bit is set in that plane of
 *                    the snapshot; unknown_is_site != 0 ORs the unknown plane in
 *   out_lattice_dev  float[nx][ny][nz] (row-major, z fastest) or NULL: the same field as a plain lattice
 * The transform is the EXACT Euclidean distance transform in integer voxel units (csrc/vigo_esdf_core.hpp):
 *   d2_site[v] = min dx^2 + dy^2 + dz^2 from voxel v to a site (0 on a site), d2_free[v] the same to a non-site voxel
 *   of the lattice (0 on a non-site);
 *   value[v]   = (float)((sqrt((double)d2_site) - sqrt((double)d2_free)) * res), every operation rounded once:
 *                positive outside, negative inside, sampled at voxel centres (u = (p - origin) / res - 0.5 of the query).
 * Padding rule: the bits of a z-row's last word beyond nz belong to neither the sites nor their complement — no distance
 * is ever measured to them, whatever a vigo_set_grid_packed caller left there.
 * Empty-set rule: where a set is empty (no site at all, or no non-site voxel), its squared distance is
 * nx^2 + ny^2 + nz^2 everywhere: finite, and larger than anything attainable inside the lattice.
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle, a plane other than 0 or 2, a grid with an axis < 2; VIGO_ERR_NO_GRID
 * before any vigo_set_grid*; VIGO_ERR_UNSUPPORTED for nx^2 + ny^2 + nz^2 > 2^30 (int32 squared distances) or more than
 * 2^33 voxels; VIGO_ERR_HIP with vigo_last_error(). */
int vigo_build_esdf(vigo_handle_t h, int plane, int unknown_is_site, float* out_lattice_dev);
/* The host twin: the same rule compiled for the CPU, on a byte grid uint8[nx][ny][nz] (bit `plane` — and bit 1 with
 * unknown_is_site — marks a site) -> out_lattice_host float[nx][ny][nz].  Host-only like vigo_accumulated_time (no GPU,
 * no handle); bit-identical to vigo_build_esdf's lattice for the same voxels.  VIGO_ERR_INVALID_ARG for a NULL pointer,
 * a plane other than 0 or 2, a dimension < 2, res not finite or <= 0; VIGO_ERR_UNSUPPORTED for the same two size
 * limits, and for a lattice whose working memory (8 bytes per voxel and the packed words) the host cannot allocate.
 * Nothing is written on an error. */
int vigo_esdf_from_voxels_host(int nx, int ny, int nz, const uint8_t* voxels_host, int plane, int unknown_is_site,
                               double res, float* out_lattice_host);

/* ---- ESDF region update (no reference counterpart; DESIGN.md §3.5b "Region update") ------
 * vigo_build_esdf_tracked is vigo_build_esdf — the same arguments, codes, lattice bits and installed field — and KEEPS
 * what an update needs in a handle buffer of its own: the z-pass and y-pass results (int32 each), the row-major float
 * lattice, two byte flags per line and two counters.  That is 12 bytes per voxel plus nx * nz + ny * nz flag bytes:
 * 201 MB (192 MiB) at 256^3 and 1.6 GB (1.5 GiB) at 512^3, grown on demand, freed by vigo_destroy; vigo_build_esdf's own
 * workspace is not used.  From this call on the handle is TRACKING: it remembers plane and unknown_is_site and holds a
 * PENDING BOX, host integers, empty after the build.
 *   While tracking, vigo_update_grid_region and vigo_update_grid_region_host add their box to the pending box as a
 *   bounding-box union — with inflate_r the box grown by r and clipped to the grid, which covers every plane the call may
 *   have changed; an n[a] == 0 adds nothing.  Nothing those entries launch or return changes.  ONE bounding box, not a
 *   list: a caller with far-apart boxes calls vigo_update_esdf between them.
 *   Tracking ends with vigo_set_grid, vigo_set_grid_host, vigo_set_grid_packed, vigo_build_esdf, vigo_set_esdf and a failed
 *   allocation of the tracking buffer; not with parameters, metric bounds, the stream or the precision.
 * vigo_update_esdf brings the kept results, the lattice and the installed field to what vigo_build_esdf_tracked would
 * produce on the current snapshot, bit for bit, and clears the pending box.  The transform is separable: a y line depends
 * on its own z-pass line only, an x line on its own y-pass line only, so only lines whose input changed are recomputed —
 * no truncation radius, no approximation.  Work: the z pass over the box' footprint columns, the y pass over the box'
 * slab of x where the z pass changed a value, the x pass and the re-tiling on the (y, z) lines where the y pass changed
 * one — at most one whole x pass (a site added to an empty column changes whole y lines: DESIGN.md §3.5b).  Stream-ordered
 * on the handle's stream.
 *   out_lattice_dev  float[nx][ny][nz] or NULL: the whole row-major lattice is also copied there
 *   stats            NULL, or filled after a synchronise of the stream (without it the call makes no host round trip):
 *                    the pending box the call worked on and the lines the y pass and the x pass recomputed
 * Errors: VIGO_ERR_INVALID_ARG for a NULL handle; VIGO_ERR_NO_GRID, with a vigo_last_error text, when the handle is not
 * tracking.  An empty pending box is VIGO_OK with nothing launched but the optional copy; the stats are then zeros. */
typedef struct {
    int32_t box_lo[3], box_n[3];   /* the pending box this call worked on (n = 0: nothing pending) */
    int64_t y_lines, x_lines;      /* lines recomputed by the y pass / the x pass */
} vigo_esdf_update_stats_t;
int vigo_build_esdf_tracked(vigo_handle_t h, int plane, int unknown_is_site, float* out_lattice_dev);
int vigo_update_esdf(vigo_handle_t h, float* out_lattice_dev, vigo_esdf_update_stats_t* stats_or_NULL);
/* The host twins (no GPU, no handle; csrc/vigo_esdf_core.hpp compiled for the CPU).  _tracked: vigo_esdf_from_voxels_host
 * with the z-pass and y-pass results in a_out, b_out (int32[nx][ny][nz] each).  vigo_esdf_update_host: a, b and the
 * lattice of the grid BEFORE the box [lo, lo + n) changed become those of new_voxels_host, the whole byte grid after it;
 * for a pending box of several updates pass their bounding box.  Codes as vigo_esdf_from_voxels_host; also
 * VIGO_ERR_INVALID_ARG for a NULL lo, n, a, b or lattice, a negative lo or n, lo + n beyond the lattice.  An n[a] == 0 is
 * VIGO_OK, nothing changes and the stats are zeros.  Nothing is written on an error. */
int vigo_esdf_from_voxels_host_tracked(int nx, int ny, int nz, const uint8_t* voxels_host, int plane, int unknown_is_site,
                                       double res, int32_t* a_out, int32_t* b_out, float* out_lattice_host);
int vigo_esdf_update_host(int nx, int ny, int nz, const uint8_t* new_voxels_host, int plane, int unknown_is_site,
                          double res, const int32_t lo[3], const int32_t n[3], int32_t* a_inout, int32_t* b_inout,
                          float* lattice_inout, vigo_esdf_update_stats_t* stats_or_NULL);

#ifdef __cplusplus
}
#endif
#endif /* VIGO_H */
