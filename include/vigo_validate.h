/* vigo_validate.h — plan validation: which of the plans a service holds are still valid on the current map, and where
 * does the first collision sit on the ones that are not?  An addition to vigo.h in a header of its own; the types, the
 * error codes and the handle are vigo.h's.
 *
 * Trajectory b has n = n_pts[b] control points (Ns when n_pts is NULL) in row b of ctrl[B][Ns][3]; the spline, its
 * duration (n - 3) * ts_ctrl and the accumulated sample clock t_k (the k-fold `t += dt`) are those of the gates
 * (vigo_traj_collision, vigo_traj_dynamic_collision).  S(n) = #{ k : t_k <= duration } samples.
 *
 *   static check    sample k collides when its position is inflated-occupied (outside the box or not finite: occupied),
 *                   over the first C(n) samples:
 *                     VIGO_VALIDATE_BY_TIME   the k with t_k <= (1.0 - not_check_ratio) * duration
 *                                             (hasCollisionTrajectory(ctrl), the gate of vigo_rebound_rounds)
 *                     VIGO_VALIDATE_BY_INDEX  the k with (double)k < (1.0 - not_check_ratio) * (int)S(n)
 *                                             (hasCollisionTrajectory(ctrl, pos), what isCurrTrajValid(pos) runs)
 *   dynamic check   over all S(n) samples: sample k lies inside an obstacle of b — obs_off's range of obs[][9], or the
 *                   n_obs_shared shared ones when obs_off is NULL; none when obs is NULL — by the strict test
 *                   sqrt(dx^2 + dy^2) - min(sx / 2, sy / 2) < 0 of vigo_traj_dynamic_collision
 *
 * Outputs, each value a function of the trajectory alone (not of B, Ns or its neighbours):
 *   out_status    int32[B]     VIGO_VALID_* bits, 0 = valid.  A count outside 4 .. Ns sets VIGO_VALID_BAD_COUNT alone:
 *                              out_first and out_dyn_first are -1, out_pos is not touched, the row counts as invalid
 *   out_first     int32[B]     the first colliding static sample, or -1
 *   out_pos       double[B][3] (may be NULL) that sample's position; rows without a static hit are not written; a NaN
 *                              coordinate is stored as the quiet NaN 0x7ff8000000000000
 *   out_dyn_first int32[B]     (may be NULL) the first sample inside an obstacle, or -1
 *   out_invalid   int32[B], out_n_invalid int32[1] (both or neither NULL): the b with out_status[b] != 0 in ascending
 *                              order, and their number; entries beyond the number are not written
 *
 * vigo_traj_validate works on device pointers in stream order on the handle's stream and makes no host round trip:
 * one launch answers every row, a second one writes the list.  The per-count sample counts and the clock are cached in
 * the handle (the clock in a slot of its own: the gates' and vigo_traj_finish's tables stay cached).
 *
 * Errors (nothing is written): VIGO_ERR_INVALID_ARG — NULL handle, B < 0, dt or ts_ctrl not finite and > 0,
 * not_check_ratio outside [0, 1] or NaN, rule not 0 or 1, n_obs_shared < 0, ctrl, out_status or out_first NULL with
 * B > 0, exactly one of out_invalid / out_n_invalid NULL, more than 2^24 samples; VIGO_ERR_UNSUPPORTED_N — Ns < 4 or
 * Ns > VIGO_MAX_CTRL_POINTS; VIGO_ERR_NO_GRID — before a grid is set.  B == 0: VIGO_OK, nothing launched,
 * out_n_invalid untouched.
 *
 * vigo_traj_validate_host is the same rule on the host, on host pointers and the byte-per-voxel grid of
 * vigo_set_grid_host (bit 0: inflated-occupied): no handle, no GPU, the same codes and the same bits
 * (VIGO_ERR_INVALID_ARG also for a grid axis < 1, a NULL origin or grid, a resolution not finite and > 0). */
#ifndef VIGO_VALIDATE_H
#define VIGO_VALIDATE_H

#include "vigo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_status bits of vigo_traj_validate */
enum {
    VIGO_VALID_STATIC = 1,       /* a checked sample is inflated-occupied */
    VIGO_VALID_DYNAMIC = 2,      /* a sample lies inside a dynamic obstacle */
    VIGO_VALID_BAD_COUNT = 4     /* count outside 4 .. Ns: nothing of the row was read */
};

/* rule of vigo_traj_validate: which prefix of the samples the static check covers */
enum {
    VIGO_VALIDATE_BY_TIME = 0,
    VIGO_VALIDATE_BY_INDEX = 1
};

int vigo_traj_validate(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, double dt,
                       double not_check_ratio, int rule, const int32_t* obs_off, const double* obs, int n_obs_shared,
                       int32_t* out_status, int32_t* out_first, double* out_pos, int32_t* out_dyn_first,
                       int32_t* out_invalid, int32_t* out_n_invalid);

int vigo_traj_validate_host(int nx, int ny, int nz, const double origin[3], double res, const uint8_t* voxels_host,
                            double ts_ctrl, int B, int Ns, const int32_t* n_pts, const double* ctrl, double dt,
                            double not_check_ratio, int rule, const int32_t* obs_off, const double* obs,
                            int n_obs_shared, int32_t* out_status, int32_t* out_first, double* out_pos,
                            int32_t* out_dyn_first, int32_t* out_invalid, int32_t* out_n_invalid);

#ifdef __cplusplus
}
#endif
#endif /* VIGO_VALIDATE_H */
