// vigo_traj_runs.hpp — where the samples of ONE whole trajectory fall.
//
// polyTrajSolver::getTrajectory (PS.cpp:1125-1137) samples a trajectory with knots k[0..K] at
// `for (t = 0; t < k[K]; t += delT)` and appends the last waypoint; getPose (PS.cpp:1026-1056) evaluates sample t in the
// FIRST segment i with k[i] <= t <= k[i+1], at local time fl(t - k[i]), and gives the default pose (0, 0, 0) to a t in
// no interval; checkCollisionTraj (PO.cpp:634-656) blames a colliding sample on that same segment.  For non-decreasing
// finite knots and delT > 0 the clock t_j (vigo_exact_time.hpp) is non-decreasing in j, so each segment's samples form
// one run of consecutive indices:
//   leading    t_j <  k[0]           (default pose, no segment)
//   segment 0  t_j in [k[0], k[1]]
//   segment i  t_j in (k[i], k[i+1]]   for i >= 1   (a sample exactly on an inner knot belongs to the earlier segment)
// and every run boundary is a binary search over the exact clock.  The endpoint (sample n) has clock t_n >= k[K]; it is
// attributed only when t_n == k[K], to the first segment whose end knot is k[K].
// Compiled for host (vigo_traj_sample_runs, the tests) and device (k_traj_runs in vigo_traj_core.hpp) alike.
#pragma once

#include "vigo_exact_time.hpp"

namespace vigo {

// per-trajectory status (include/vigo.h VIGO_TRAJ_*)
enum {
    kTrajOk = 0,
    kTrajBadKnots = 1,     // a knot not finite, or knots decreasing
    kTrajBadDelT = 2,      // delT not a finite number > 0
    kTrajStall = 3,        // the clock stops advancing below k[K]: the reference's loop never ends
    kTrajTooLong = 4,      // more than kTrajMaxSamples samples
    kTrajBadOffsets = 5,   // (device entry only) seg_off is not a CSR over [0, S]
};
constexpr int64_t kTrajMaxSamples = 0x7ffffffe;   // INT32_MAX - 1: with the endpoint the list length fits an int32

// t_j from the table when there is one (the pre-kernel's, built for k_last = n), the closed form otherwise
VIGO_HD double traj_clock(const ClockTable* C, double d, int64_t k) {
    return (C && C->n > 0) ? clock_at(*C, (int)k) : accumulated_time(d, k);
}

// the first j in [lo, hi] with t_j >= x (strict: t_j > x), given t_hi qualifies or j == hi is the answer anyway
VIGO_HD int64_t clock_search(const ClockTable* C, double d, double x, bool strict, int64_t lo, int64_t hi) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const double t = traj_clock(C, d, mid);
        if (strict ? (t > x) : (t >= x)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The same search on the table: the clock is t0[p] + (k - k0[p]) inc[p] on piece p (clock_from's expression), so the
// answer lies in the piece before the first one whose start qualifies, at about (x - t0) / inc into it: a search over
// the pieces, two probes around the estimate, a bisection between them.  A handful of table reads instead of a binary
// search over k with a piece search per probe (k_traj_runs is one thread per trajectory: its reads are latency).
VIGO_HD int64_t table_search(const ClockTable& C, double x, bool strict, int64_t lo, int64_t hi) {
    auto pred = [&](double t) { return strict ? (t > x) : (t >= x); };
    int a = 0, b = C.n;                                   // the first piece whose first value qualifies (C.n: none)
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (pred(C.t0[mid])) b = mid; else a = mid + 1;
    }
    int64_t f;
    if (a == 0) {
        f = 0;
    } else {
        const int q = a - 1;                              // its value at j = 0 does not qualify
        const int64_t k0 = C.k0[q], end = a < C.n ? (int64_t)C.k0[a] : hi + 1;
        const int64_t len = end - k0;                     // j = len: the next piece's first value, or none
        const double t0 = C.t0[q], inc = C.inc[q];
        auto val = [&](int64_t j) { return t0 + (double)j * inc; };
        int64_t jl = 1, jh = len;
        if (inc > 0.0 && len > 1) {
            const double e = ceil((x - t0) / inc);
            const int64_t est = e < 1.0 ? 1 : e > (double)len ? len : (int64_t)e;
            const int64_t e0 = est - 2 < 1 ? 1 : est - 2, e1 = est + 2 > len ? len : est + 2;
            if (e0 < len && !pred(val(e0))) jl = e0 + 1;
            if (e1 < len && pred(val(e1))) jh = e1;
        }
        while (jl < jh) {
            const int64_t mid = jl + ((jh - jl) >> 1);
            if (pred(val(mid))) jh = mid; else jl = mid + 1;
        }
        f = k0 + jl;
    }
    return f < lo ? lo : f > hi ? hi : f;
}

// n = the number of samples t_j < k[K] (the loop's trip count), or a status.  The clock stalls below end exactly when
// delT is at most half an ulp of the largest double below end: the increment fl(t + d) - t of a binade is d rounded to
// the binade's ulp, and it only grows with t.  A gallop from the estimate end / d brackets n (the accumulated clock
// stays within a relative n 2^-52 of j d), bisection finishes.
VIGO_HD int traj_sample_count(double end, double d, int64_t* n_out) {
    *n_out = 0;
    if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return kTrajBadDelT;   // NaN, <= 0, inf
    if (!(end > 0.0)) return kTrajOk;                                          // t_0 = 0 already ends the loop
    const double below = nextafter(end, 0.0);
    if (below > 0.0 && d <= ldexp(1.0, ilogb(below) - 53)) return kTrajStall;
    const double est_d = end / d;
    int64_t est = est_d < (double)kTrajMaxSamples ? (int64_t)est_d : kTrajMaxSamples;
    int64_t lo = est > 2 ? est - 2 : 0, hi = est + 2 < kTrajMaxSamples ? est + 2 : kTrajMaxSamples;
    int64_t g = 2;
    while (lo > 0 && traj_clock(nullptr, d, lo) >= end) {   // invariant wanted: t_lo < end (t_0 = 0 qualifies)
        hi = lo;
        g *= 2;
        lo = lo > g ? lo - g : 0;
    }
    g = 2;
    while (traj_clock(nullptr, d, hi) < end) {               // invariant wanted: t_hi >= end
        if (hi == kTrajMaxSamples) return kTrajTooLong;
        lo = hi;
        g *= 2;
        hi = hi < kTrajMaxSamples - g ? hi + g : kTrajMaxSamples;
    }
    *n_out = clock_search(nullptr, d, end, false, lo, hi);
    return kTrajOk;
}

VIGO_HD int traj_knots_status(int K, const double* k) {
    for (int i = 0; i <= K; ++i) {
        if (!(fabs(k[i]) <= 1.7976931348623157e308)) return kTrajBadKnots;
        if (i > 0 && !(k[i - 1] <= k[i])) return kTrajBadKnots;
    }
    return kTrajOk;
}

// The runs of one trajectory once n is known and (optionally) its clock table built for k_last = n:
//   *lead       the leading default-pose run is samples [0, *lead)
//   first/len   segment i's run, i < K (stride: element spacing of both arrays)
//   *end_seg    the segment the endpoint is attributed to, or -1
VIGO_HD void traj_runs(int K, const double* k, double d, int64_t n, const ClockTable* C, int32_t* lead, int32_t* first,
                       int32_t* len, int stride, int32_t* end_seg) {
    const bool table = C && C->n > 0;
    auto search = [&](double x, bool strict, int64_t lo) {
        return table ? table_search(*C, x, strict, lo, n) : clock_search(C, d, x, strict, lo, n);
    };
    int64_t b = search(k[0], false, 0);
    *lead = (int32_t)b;
    for (int i = 0; i < K; ++i) {
        const int64_t e = search(k[i + 1], true, b);
        first[(size_t)i * stride] = (int32_t)b;
        len[(size_t)i * stride] = (int32_t)(e - b);
        b = e;
    }
    *end_seg = -1;
    if (K >= 1 && traj_clock(C, d, n) == k[K])
        for (int i = 0; i < K; ++i)
            if (k[i + 1] == k[K]) { *end_seg = i; break; }
}

}  // namespace vigo
