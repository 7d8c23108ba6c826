// vigo_seed_core.hpp — the rules of the seed-path stage between polyTrajOccMap and bsplineTraj (bspline_node.cpp:317-378),
// one copy for the kernel of vigo_seed.hip (vigo_seed_paths) and its host twin (vigo_seed_paths_host, vigo_api.cpp).
// For one trajectory with knots k[0..K] and coefficients cf[K][3][deg + 1] (vigo_traj_point_check's layout):
//
//   1 clock    t_0 = 0, t_{j+1} = fl(t_j + dt), kept while t_j <= duration — inclusive, no endpoint appended
//              (polyTrajOccMap.cpp:434-446).  seed_sample_count() is the trip count, the lanes take t_j from
//              accumulated_time() (vigo_exact_time.hpp).
//   2 sample   getPos(min(t_j, duration)) (polyTrajOccMap.cpp:484-490, polyTrajSolver.cpp:1058-1078): the FIRST i with
//              k[i] <= t <= k[i+1], local time fl(t - k[i]), the terms summed in d = 0..deg order, the power from a
//              functor (SeedPowExact: the correctly rounded power of vigo_exact_pow.hpp; the twin may take libm's);
//              a t in no interval gives (0, 0, 0).
//   3 adjust   adjustPathLengthDirect (bsplineTraj.cpp:754-793) as bsplineTraj::adjustPathLengthWith has it: the list
//              is cut after the first pair that lies past max(prev, max_path_length) from the first point, is free and
//              follows a free stretch of at least 1.5 — the result is always a PREFIX of the input, so the rule returns
//              its length.  Lines are line_occupied (vigo_pathsearch_core.hpp) on plane 0.
//   4 spacing  a consecutive distance of the adjusted list above 1.5 * control_point_distance fails the try
//              (bsplineTraj.cpp:215-222); dt = fl(dt * 0.8), prev carried over, at most max_tries tries.
//   5 thin     keep a point at least 0.8 * control_point_distance from the last kept one, repeat the last kept point
//              (bsplineTraj.cpp:224-241); final_time = (adjusted_count - 1) * dt.
//   6 head     updatePath's head on the seed (bsplineTraj.cpp:290-312): goal test, rule 3 again, fillPath
//              (bsplineTraj.cpp:247-288) when fewer than 4 points result.
//
// Norms are sqrt((dx*dx + dy*dy) + dz*dz); every fp64 expression is compiled without contraction.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vigo_exact_pow.hpp"
#include "vigo_exact_time.hpp"
#include "vigo_pathsearch_core.hpp"

namespace vigo {

// per-trajectory status (include/vigo.h VIGO_SEED_*)
enum {
    kSeedOk = 0,
    kSeedNoSpacing = 1,      // every try failed rule 4: no seed
    kSeedGoalOccupied = 2,   // the seed's last pose is inflated-occupied: no fit points
    kSeedTooShort = 3,       // a seed of at most one pose
    kSeedDeferred = 4,       // a try with more samples than the capacity, or a list longer than point_cap: nothing written
    kSeedBadInput = 5,       // offsets outside [0, S], a knot / dt0 / duration not finite, dt0 <= 0, a stalled clock
};
constexpr int kSeedCapacity = 1536;   // samples of one try (vigo_seed_capacity): what 64 KiB of LDS hold, see vigo_seed.hip
constexpr int kSeedMaxDeg = 15;

VIGO_HD bool seed_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// rule 1: n = the number of j with t_j <= duration.  Returns kSeedOk, kSeedBadInput (the clock stops advancing at or below
// duration: the reference's loop never ends) or kSeedDeferred (n > cap; *n is then not exact).  dt is finite and > 0,
// duration finite.  The accumulated clock stays within a relative j 2^-52 of j dt, so an estimate well past cap decides.
VIGO_HD int seed_sample_count(double duration, double dt, int cap, int64_t* n) {
    *n = 0;
    if (!(duration >= 0.0)) return kSeedOk;
    if (duration > 0.0 && dt <= ldexp(1.0, ilogb(duration) - 53)) return kSeedBadInput;
    const double est_d = duration / dt;
    if (est_d > (double)cap + 8.0) { *n = (int64_t)cap + 1; return kSeedDeferred; }
    int64_t lo = (int64_t)est_d, hi = lo + 2;
    lo = lo > 2 ? lo - 2 : 0;
    while (lo > 0 && accumulated_time(dt, lo) > duration) lo = lo > 4 ? lo - 4 : 0;     // wanted: t_lo <= duration
    while (!(accumulated_time(dt, hi) > duration)) { lo = hi; hi += 4; }                // wanted: t_hi > duration
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (accumulated_time(dt, mid) > duration) hi = mid; else lo = mid;
    }
    *n = hi;                                                                            // t_0 .. t_{hi-1} qualify
    return hi > cap ? kSeedDeferred : kSeedOk;
}

// the powers of rule 2, asked in d = 0..deg order: Pow::Run(t).next(d) = t^d
struct SeedPowExact {        // the kernels' power: correctly rounded (the running double-double, pow_exact where it is unsure)
    struct Run {
        double t, hi, lo;
        VIGO_HD explicit Run(double t_) : t(t_), hi(1.0), lo(0.0) {}
        VIGO_HD double next(int d) {
            if (d == 0) return 1.0;
            if (d == 1) { hi = t; return t; }
            return pow_step(hi, lo, t) ? pow_exact(t, d) : hi;
        }
    };
};

struct SeedPowLibm {         // the facade's power: libm's pow(t, d) (polyTrajSolver.cpp:1035-1039) — the twin's pow_mode 1
    struct Run {
        double t;
        VIGO_HD explicit Run(double t_) : t(t_) {}
        VIGO_HD double next(int d) { return pow(t, (double)d); }
    };
};

// rule 2: getPos at clock value t
template <class Pow>
VIGO_HD void seed_sample(int K, const double* k, const double* cf, int deg, double t, double duration, const Pow&, double* p) {
    if (t > duration) t = duration;
    p[0] = p[1] = p[2] = 0.0;
    for (int i = 0; i < K; ++i) {
        if (t >= k[i] && t <= k[i + 1]) {
            const double lt = t - k[i];
            typename Pow::Run power(lt);
            const double* c = cf + (size_t)i * 3 * (deg + 1);
            double x = 0, y = 0, z = 0;
            for (int d = 0; d <= deg; ++d) {
                const double pw = power.next(d);
                x += c[d] * pw;
                y += c[(deg + 1) + d] * pw;
                z += c[2 * (deg + 1) + d] * pw;
            }
            p[0] = x; p[1] = y; p[2] = z;
            break;
        }
    }
}

VIGO_HD double seed_norm(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// what rule 3 and rule 4 ask of the pair (pts[i], pts[i+1]): independent per pair
template <class Occ>
VIGO_HD void seed_pair(const Occ& occ, double res, const double* pts, int i, uint8_t* line, double* step, double* dist) {
    const double *p1 = pts + 3 * (size_t)i, *p2 = p1 + 3;
    *line = line_occupied(occ, res, p1, p2) ? 1 : 0;
    *step = seed_norm(p2, p1);
    *dist = seed_norm(p2, pts);
}

// rule 3 over the pairs' arrays: the length of the adjusted prefix of an n-point list, *prev_out the value the
// reference's function-static holds afterwards
VIGO_HD int seed_adjust(int n, double prev_in, double max_path_length, const uint8_t* line, const double* step, const double* dist,
                        double* prev_out) {
    *prev_out = prev_in;
    if (n <= 0) return 0;
    const double limit = prev_in < max_path_length ? max_path_length : prev_in;   // std::max(prevPathLength, maxPathLength_)
    double total = 0.0, min_length = 0.0;
    bool exceed = false;
    for (int i = 0; i + 1 < n; ++i) {
        total = dist[i];
        if (total >= limit) exceed = true;
        const bool occupied = line[i] != 0;
        if (exceed && !occupied && min_length >= 1.5) {
            *prev_out = total;
            return i + 2;
        }
        if (occupied) min_length = 0.0;
        else min_length += step[i];
    }
    *prev_out = total;
    return n;
}

// rule 4 for pair i of an adjusted list of c points
VIGO_HD bool seed_too_far(int i, int c, const double* step, double control_point_distance) {
    return i + 1 < c && step[i] > control_point_distance * 1.5;
}

// rule 5, in place on pts[0 .. c) (c >= 1; pts holds c + 1 points): the seed's pose count, repeated last pose included
VIGO_HD int seed_thin(double* pts, int c, double control_point_distance) {
    int kept = 1;
    double last[3] = {pts[0], pts[1], pts[2]};
    for (int i = 1; i < c; ++i) {
        const double* p = pts + 3 * (size_t)i;
        if (seed_norm(p, last) >= control_point_distance * 0.8) {
            last[0] = p[0]; last[1] = p[1]; last[2] = p[2];
            pts[3 * (size_t)kept] = last[0]; pts[3 * (size_t)kept + 1] = last[1]; pts[3 * (size_t)kept + 2] = last[2];
            ++kept;
        }
    }
    pts[3 * (size_t)kept] = last[0]; pts[3 * (size_t)kept + 1] = last[1]; pts[3 * (size_t)kept + 2] = last[2];
    return kept + 1;
}

// rule 6's fillPath for a seed of 2 or 3 poses: 4 or 5 points into out[5][3], their number returned
VIGO_HD int seed_fill(const double* seed, int n, double* out) {
    if (n == 2) {
        for (int a = 0; a < 3; ++a) {
            const double ps = seed[a], pf = seed[3 + a], d = pf - ps;
            out[a] = ps;
            out[3 + a] = d / 3.0 + ps;
            out[6 + a] = d * 2.0 / 3.0 + ps;
            out[9 + a] = pf;
        }
        return 4;
    }
    for (int a = 0; a < 3; ++a) {
        const double ps = seed[a], pm = seed[3 + a], pf = seed[6 + a];
        out[a] = ps;
        out[3 + a] = (ps + pm) / 2.0;
        out[6 + a] = pm;
        out[9 + a] = (pm + pf) / 2.0;
        out[12 + a] = pf;
    }
    return 5;
}

// rule 6 once the seed's pairs are known: where the fit points come from.  *from_fill: seed_fill's points, otherwise the
// first (return value) poses of the seed.  n >= 2.
VIGO_HD int seed_fit_count(int n, int adjusted, bool* from_fill) {
    *from_fill = false;
    if (adjusted >= 4) return adjusted;
    if (n >= 4) return n;             // fillPath hands a path of four or more poses back whole
    *from_fill = true;
    return n == 2 ? 4 : 5;
}

// one trajectory's inputs and results
struct SeedIn {
    int K, deg;
    const double* knots;     // [K + 1]
    const double* coeffs;    // [K][3][deg + 1]
    double duration, dt0, control_point_distance, max_path_length, prev_seed, prev_fit;
    int max_tries, point_cap;
};
struct SeedOut {
    int status, tries, seed_n, fit_n;
    double dt, final_time, prev_seed, prev_fit;
};

VIGO_HD void seed_reset(const SeedIn& in, int status, SeedOut* o) {
    o->status = status; o->tries = 0; o->seed_n = 0; o->fit_n = 0;
    o->dt = in.dt0; o->final_time = 0.0; o->prev_seed = in.prev_seed; o->prev_fit = in.prev_fit;
}

VIGO_HD bool seed_input_ok(const SeedIn& in) {
    if (!seed_finite(in.duration) || !seed_finite(in.dt0) || !(in.dt0 > 0.0)) return false;
    for (int i = 0; i <= in.K; ++i)
        if (!seed_finite(in.knots[i])) return false;
    return true;
}

// The whole stage for one trajectory, serially (the host twin; the kernel runs the same rules with the lanes of a wave
// on the per-sample and per-pair parts).  Work arrays: pts[3 * (cap + 1)], step[cap], dist[cap], line[cap].  seed / fit:
// the caller's rows of point_cap points, written only for the statuses that have them.
template <class Occ, class Pow>
inline void seed_one(const SeedIn& in, const Occ& occ, double res, const Pow& power, int cap, double* pts, double* step, double* dist,
                     uint8_t* line, SeedOut* o, double* seed, double* fit) {
    if (!seed_input_ok(in)) { seed_reset(in, kSeedBadInput, o); return; }
    double dt = in.dt0, prev = in.prev_seed;
    int tries = 0, c = 0;
    bool found = false;
    while (tries < in.max_tries) {
        int64_t n64;
        const int st = seed_sample_count(in.duration, dt, cap, &n64);
        if (st != kSeedOk) { seed_reset(in, st, o); return; }
        const int n = (int)n64;
        ++tries;
        for (int j = 0; j < n; ++j) seed_sample(in.K, in.knots, in.coeffs, in.deg, accumulated_time(dt, j), in.duration, power, pts + 3 * (size_t)j);
        for (int i = 0; i + 1 < n; ++i) seed_pair(occ, res, pts, i, line + i, step + i, dist + i);
        c = seed_adjust(n, prev, in.max_path_length, line, step, dist, &prev);
        bool far = false;
        for (int i = 0; i + 1 < c; ++i) far = far || seed_too_far(i, c, step, in.control_point_distance);
        if (!far) { found = true; break; }
        dt = dt * 0.8;
    }
    o->tries = tries; o->dt = dt; o->prev_seed = prev; o->prev_fit = in.prev_fit;
    o->seed_n = 0; o->fit_n = 0; o->final_time = 0.0;
    if (!found) { o->status = kSeedNoSpacing; return; }
    if (c == 0) { o->status = kSeedTooShort; return; }     // no sample at all (duration < 0): an empty seed
    const int sn = seed_thin(pts, c, in.control_point_distance);
    if (sn > in.point_cap) { seed_reset(in, kSeedDeferred, o); return; }
    o->final_time = (double)(c - 1) * dt;
    const double* goal = pts + 3 * (size_t)(sn - 1);
    int fn = 0;
    bool from_fill = false;
    double fill[15];
    int status = kSeedOk;
    if (occ(goal[0], goal[1], goal[2])) {
        status = kSeedGoalOccupied;
    } else {
        for (int i = 0; i + 1 < sn; ++i) seed_pair(occ, res, pts, i, line + i, step + i, dist + i);
        const int c2 = seed_adjust(sn, in.prev_fit, in.max_path_length, line, step, dist, &o->prev_fit);
        fn = seed_fit_count(sn, c2, &from_fill);
        if (fn > in.point_cap) { seed_reset(in, kSeedDeferred, o); return; }
        if (from_fill) seed_fill(pts, sn, fill);
    }
    o->status = status; o->seed_n = sn; o->fit_n = fn;
    for (int i = 0; i < 3 * sn; ++i) seed[i] = pts[i];
    for (int i = 0; i < 3 * fn; ++i) fit[i] = from_fill ? fill[i] : pts[i];
}

// the inflated-occupied predicate on a dense byte grid [nx][ny][nz] (bit 0; outside the grid: occupied), as the facade's
// dense map answers it
struct SeedByteGrid {
    const uint8_t* vox;
    int nx, ny, nz;
    double origin[3], res;
    bool operator()(double x, double y, double z) const {
        const double f[3] = {floor((x - origin[0]) / res), floor((y - origin[1]) / res), floor((z - origin[2]) / res)};
        const int n[3] = {nx, ny, nz};
        for (int a = 0; a < 3; ++a)
            if (!(f[a] >= 0.0 && f[a] < (double)n[a])) return true;
        return (vox[((size_t)f[0] * ny + (size_t)f[1]) * nz + (size_t)f[2]] & 1u) != 0;
    }
};

}  // namespace vigo
