// vigo_finish_core.hpp — the end of a bsplineTraj plan, one copy for the kernel (vigo_finish.hip: k_traj_finish) and
// its host twin (vigo_traj_finish_host): linearFeasibilityReparam() (BT.cpp:1116-1137) and the sampled path of
// evalTrajToMsg (BT.cpp:1502-1518) over evalTraj (BT.h:345).
//
// For a trajectory of n control points (7 <= n <= Ns) at ts_ctrl, with its own max_vel / max_acc:
//
//   duration   = (n - 3) * ts_ctrl                                      knot(n), as deboor<3> computes it
//   maxV = maxA = 0.0
//   for k = 0, 1, ...  while t_k < duration, t_k the k-fold `t += ts`   (strict <, BT.cpp:1122)
//       nv = sqrt((v0*v0 + v1*v1) + v2*v2), v = traj_eval(deriv 1, t_k);  if (nv > maxV) maxV = nv
//       na = likewise on deriv 2;                                         if (na > maxA) maxA = na
//   factorVel = max_vel / maxV;  factorAcc = sqrt(max_acc / maxA)
//   factor    = (factorAcc < factorVel) ? factorAcc : factorVel           (std::min's own comparison)
//   n_samp    = #{ i : s_i <= duration }, s_i the i-fold `t += dt`        (<=, BT.h:347)
//   pos[i]    = traj_eval(deriv 0, s_i)
//   vel[i]    = traj_eval(deriv 1, (double)i * dt)                        (the PRODUCT clock of BT.cpp:1509)
//   (a NaN coordinate of pos / vel is stored as the one quiet NaN 0x7ff8000000000000, see finish_nan)
//
// Nothing guards the divisions: a trajectory that does not move has factor +inf, a straight evenly spaced one has
// factorAcc +inf and factor = factorVel.  A NaN norm never replaces a maximum (`>` is false against NaN), so the maxima
// are those of the finite samples, and since the maximum of non-NaN values does not depend on the order they are
// visited in, the lanes of a wave that stride over the clock and then reduce get the serial loop's bits.
//
// The two accumulated clocks come as tables shared by the whole call (times_ts[0 .. T_ts), times_dt[0 .. T_dt)), both
// non-decreasing and filled up to the longest duration (Ns - 3) * ts_ctrl: every function below takes (lane, stride) —
// (threadIdx.x, 64) in the kernel, (0, 1) on the host.
#pragma once

#include "vigo_exact_time.hpp"
#include "vigo_grid.hpp"

namespace vigo {

// out_status of vigo_traj_finish (VIGO_FINISH_* of include/vigo.h)
constexpr int kFinishOk = 0, kFinishCapacity = 1, kFinishInvalidN = 2;

// a clock step the entries accept: finite and positive
VIGO_HD bool finish_step_ok(double d) { return d > 0.0 && d < INFINITY; }

VIGO_HD double finish_duration(int n, double ts_ctrl) { return (n - 3) * ts_ctrl; }

// the facade's norm() and the reference harness's default summation order
VIGO_HD double finish_norm(const double (&v)[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

VIGO_HD void finish_take_max(double& m, double v) {
    if (v > m) m = v;
}

// the lane's share of the two maxima: samples k = lane, lane + stride, ... of the ts clock below `duration`
VIGO_HD void finish_maxima(const double* ctrl, int n, double ts_ctrl, double duration, int T_ts, const double* times_ts, int lane,
                           int stride, double& maxV, double& maxA) {
    for (int k = lane; k < T_ts && times_ts[k] < duration; k += stride) {
        double v[3], a[3];
        traj_eval(ctrl, n, ts_ctrl, 1, times_ts[k], v);
        traj_eval(ctrl, n, ts_ctrl, 2, times_ts[k], a);
        finish_take_max(maxV, finish_norm(v));
        finish_take_max(maxA, finish_norm(a));
    }
}

VIGO_HD double finish_factor(double max_vel, double max_acc, double maxV, double maxA) {
    const double factorVel = max_vel / maxV;
    const double factorAcc = sqrt(max_acc / maxA);
    return (factorAcc < factorVel) ? factorAcc : factorVel;
}

// #{ i < T : times[i] <= duration } of a non-decreasing table
VIGO_HD int finish_count(const double* times, int T, double duration) {
    int lo = 0, hi = T;                              // times[i] <= duration below lo, > duration from hi on
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (times[mid] <= duration) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the quiet NaN an INVALID_N row reports, and the one every NaN sample is stored as: IEEE 754 leaves a NaN's sign and
// payload to the implementation, and gfx950 (which folds the negation of a subtraction into its operand) and x86 differ
// in the sign of c[i + 1] - c[i] on a NaN control point.  x86 gives this pattern for inputs that carry it.
VIGO_HD double finish_nan() {
    const uint64_t bits = 0x7ff8000000000000ull;
    double v;
    memcpy(&v, &bits, sizeof v);
    return v;
}
VIGO_HD double finish_sample(double v) { return v != v ? finish_nan() : v; }

// the lane's share of the sample rows i < n_out: pos[i][3], and vel[i][3] unless vel is NULL
VIGO_HD void finish_samples(const double* ctrl, int n, double ts_ctrl, double dt, int n_out, const double* times_dt, int lane, int stride,
                            double* pos, double* vel) {
    for (int i = lane; i < n_out; i += stride) {
        double p[3];
        traj_eval(ctrl, n, ts_ctrl, 0, times_dt[i], p);
        for (int a = 0; a < 3; ++a) pos[3 * (size_t)i + a] = finish_sample(p[a]);
        if (vel) {
            const double t = (double)i * dt;
            traj_eval(ctrl, n, ts_ctrl, 1, t, p);
            for (int a = 0; a < 3; ++a) vel[3 * (size_t)i + a] = finish_sample(p[a]);
        }
    }
}

}  // namespace vigo
