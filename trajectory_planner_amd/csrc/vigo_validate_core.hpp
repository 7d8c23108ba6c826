// vigo_validate_core.hpp — are held plans still valid on the current map?  One copy of the rule for the kernel
// (vigo_validate.hip: k_traj_validate) and its host twin (vigo_traj_validate_host).
//
// For a trajectory of n control points (4 <= n <= Ns) at ts_ctrl, duration = (n - 3) * ts_ctrl, t_k the k-fold `t += dt`:
//
//   S(n)     = #{ k : t_k <= duration }                               the samples of evalTraj (BT.h:347)
//   static   sample k < C(n) collides when isInflatedOccupied(at(t_k)) (outside the box and non-finite: occupied)
//     C(n), rule BY_TIME  = #{ k : t_k <= (1.0 - ratio) * duration }  hasCollisionTrajectory(ctrl), BT.h:313
//     C(n), rule BY_INDEX = #{ k : (double)k < (1.0 - ratio) * (int)S(n) }   hasCollisionTrajectory(ctrl, pos), BT.h:329
//   dynamic  sample k < S(n) collides when it lies inside an obstacle of the trajectory: sqrt(dx^2 + dy^2 + 0) - size < 0,
//            size = min(sx / 2, sy / 2) (BT.h:344-368, the expression of dyn_point_hit in vigo_grid.hpp)
//
//   status    = VALID_STATIC if a static sample collides | VALID_DYNAMIC if a dynamic one does; VALID_BAD_COUNT alone for
//               a count outside 4 .. Ns
//   first     = the smallest colliding static k or -1, pos its position (NaN coordinates as the one quiet NaN)
//   dyn_first = the smallest k inside an obstacle or -1
//
// S(n) and C(n) come from a host-made table with one pair per count 4 .. Ns (validate_counts); the clock is the table
// of the longest duration, of which every count's samples are a prefix.  The samples are visited in blocks of
// `stride` consecutive k (64 lanes in the kernel, 1 on the host), each sample evaluated once for both checks; after a
// block validate_done says whether a later block can still matter.  A first hit is the smallest k of the first block
// that holds one, so blocks after it are not needed and the result does not depend on the stride.
#pragma once

#include "vigo_exact_time.hpp"
#include "vigo_finish_core.hpp"

namespace vigo {

// out_status bits and rules (VIGO_VALID_* / VIGO_VALIDATE_* of include/vigo_validate.h)
constexpr int kValidStatic = 1, kValidDynamic = 2, kValidBadCount = 4;
constexpr int kValidateByTime = 0, kValidateByIndex = 1;
constexpr int kValidateMinN = 4;                            // gate_N_ok's lower end

VIGO_HD bool validate_count_ok(int n, int Ns) { return n >= kValidateMinN && n <= Ns; }
// entries of the per-count table: {S, C} of count n at tab[2 * (n - 4)]
VIGO_HD int validate_tab_entries(int Ns) { return 2 * (Ns - kValidateMinN + 1); }

// C(n) of rule BY_INDEX from S: the k >= 0 with (double)k < x, x = (1.0 - ratio) * S, are 0 .. ceil(x) - 1
VIGO_HD int validate_checked_by_index(double ratio, int S) {
    const double x = (1.0 - ratio) * S;
    if (!(x > 0.0)) return 0;
    const double c = ceil(x);
    return c < (double)S ? (int)c : S;
}

// {S(n), C(n)} for one count.  false: more than 2^24 samples
inline bool validate_counts(double dt, double ts_ctrl, double ratio, int rule, int n, int32_t* S_out, int32_t* C_out) {
    const double duration = finish_duration(n, ts_ctrl);
    const int S = count_sample_times(dt, duration);
    if (S < 0) return false;
    int C;
    if (rule == kValidateByIndex) {
        C = validate_checked_by_index(ratio, S);
    } else {
        C = count_sample_times(dt, (1.0 - ratio) * duration);
        if (C < 0 || C > S) C = S;
    }
    *S_out = S;
    *C_out = C;
    return true;
}

// the obstacles of trajectory b: obs_off's range, or the shared ones; none without obs (gate_dynamic_hit's rule)
VIGO_HD void validate_obs_range(const int32_t* obs_off, const double* obs, int n_obs_shared, int b, int& o0, int& o1) {
    o0 = (obs && obs_off) ? obs_off[b] : 0;
    o1 = !obs ? 0 : (obs_off ? obs_off[b + 1] : n_obs_shared);
    if (o1 < o0) o1 = o0;
}

// what one lane knows of a trajectory before the loop over the blocks
struct ValidateRow {
    int n, S, C, o0, o1;
};

// sample k of the row, evaluated once: bit kValidStatic if it is a checked sample and collides with the map, bit
// kValidDynamic if it lies inside an obstacle; p its position.  k >= S: nothing is evaluated, 0.
template <class Occ>
VIGO_HD int validate_sample(const double* ctrl, const ValidateRow& r, double ts_ctrl, const double* times, int k, const Occ& occ,
                            const double* obs, bool want_static, bool want_dynamic, double (&p)[3]) {
    const bool st = want_static && k < r.C, dy = want_dynamic && r.o1 > r.o0;
    if (k >= r.S || !(st || dy)) return 0;
    traj_eval(ctrl, r.n, ts_ctrl, 0, times[k], p);
    int bits = 0;
    if (st && occ(p[0], p[1], p[2])) bits |= kValidStatic;
    if (dy) {
        for (int j = r.o0; j < r.o1; ++j)
            if (dyn_point_hit(p, obs + 9 * (size_t)j)) { bits |= kValidDynamic; break; }
    }
    return bits;
}

// after the block of samples [base, base + stride): no later block can change first / dyn_first (-1: none yet)
VIGO_HD bool validate_done(const ValidateRow& r, int base, int stride, int first, int dyn_first) {
    const int next = base + stride;
    const bool static_done = first >= 0 || next >= r.C || next >= r.S;
    const bool dynamic_done = dyn_first >= 0 || r.o1 <= r.o0 || next >= r.S;
    return static_done && dynamic_done;
}

VIGO_HD int validate_status(int first, int dyn_first) { return (first >= 0 ? kValidStatic : 0) | (dyn_first >= 0 ? kValidDynamic : 0); }

}  // namespace vigo
