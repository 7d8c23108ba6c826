// vigo_guide_core.hpp — the guide assignment of bsplineTraj's prologue (host/src/bsplineTraj.cpp:494-595:
// checkCollisionLine, shortcutPath, findGuidePointSemiCircle, assignGuidePointsSemiCircle), written once for the kernel
// (vigo_guides.hip) and for the host (host/src/cabi_host.cpp: vigo_host_guide_core; the facade's setDeviceGuides).
//
// The core is templated on a map predicate occ(x, y, z) — bit plane 0 of the snapshot, outside the grid occupied, as
// vigo_query_points — and on an atan2 functor.  With std::atan2 it is the facade's step bit for bit
// (tests/test_guide_core.py pins that); with vigo_atan2 below, which is plain fp64 arithmetic, the host build is the
// bit-exact twin of what the kernel computes.  Vector arithmetic follows mini_eigen.h's evaluation order:
// dot = (x0*y0 + x1*y1) + x2*y2, norm = sqrt(squaredNorm), a scalar times a vector multiplies component by scalar.
// Every fp64 expression is compiled without contraction, with IEEE sqrt and division.
//
// Kept as the facade writes them: the a += res walk of a line check and the a -= 0.1 walk of the bisection (the
// accumulated values, not k * step), the truncated pi, the guide point that survives a failed search (carried across
// control points and segments by guide_assign, zero at first), the line-collision pushes onto first-1 .. second+1
// clipped to [3, N-4], the idx < 0 || idx >= N skip, diff / diff.norm() with a zero diff (NaNs), and a shortcut that
// ends without the path's last point when the last line check collides.
//
// The kernel spreads the line checks, the bracket tests and the bisection steps over lanes; it calls the pieces below
// (guide_line_point, guide_bracket, guide_bisect_eval, guide_bisect_event, guide_bisect_point), so a lane computes
// what the serial loops of guide_shortcut and guide_find compute at the same step.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef VIGO_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_HD __host__ __device__ __forceinline__
#else
#define VIGO_HD inline
#endif
#endif

namespace vigo {

// per-trajectory status (include/vigo.h VIGO_GUIDE_*)
enum { kGuideOk = 0, kGuideDeferred = 1 };
constexpr int kGuidePathCap = 256;          // path points of one segment the kernel holds in LDS (vigo_guide_capacity)
constexpr int kGuideMaxIndex = 1 << 24;     // |first|, |second| of a segment beyond this are refused (index arithmetic)
constexpr double kGuidePi = 3.1415926;      // utils.h: PI_const, truncated on purpose

// ---- atan2 in plain fp64 operations ------------------------------------------------------------------------------
// q = min(|y|, |x|) / max(|y|, |x|) in [0, 1].  Below 3/64: atan(q) = q + q * s * P(s), s = q * q, the odd Taylor series
// to q^17.  Otherwise c = k / 32 nearest to q, t = (q - c) / (1 + q * c) with |t| <= 1/64 (q - c is exact), and
// atan(q) = atan(c) + atan(t) with atan(c) from a table of (hi, lo) pairs (17 significant decimal digits: each literal
// names one double).  The quadrant constants pi/2 and pi are (hi, lo) pairs too and are combined with the table's hi
// by an exact two-term sum, so one rounding is left at the end.
// Design bound 2 ulp (half an ulp of q carried through, the roundings of t, the final sum); sign and zero cases as IEEE
// atan2: (+-0, +0) -> +-0, (+-0, x < 0) -> +-pi, (y, +-0) -> +-pi/2, infinities, NaN -> NaN.
VIGO_HD double vigo_atan_series(double t) {   // atan(t) - t for |t| <= 3/64
    const double s = t * t;
    double p = 1.0 / 17.0;
    p = -1.0 / 15.0 + s * p;
    p = 1.0 / 13.0 + s * p;
    p = -1.0 / 11.0 + s * p;
    p = 1.0 / 9.0 + s * p;
    p = -1.0 / 7.0 + s * p;
    p = 1.0 / 5.0 + s * p;
    p = -1.0 / 3.0 + s * p;
    return t * (s * p);
}

VIGO_HD double vigo_atan2(double y, double x) {
    static constexpr double kAtan32[33][2] = {
        {0.0, 0.0},
        {0.031239833430268277, -1.188442711587748e-18},
        {0.06241880999595735, -1.5490756308295046e-18},
        {0.09347678115858947, -6.2844725995420954e-18},
        {0.12435499454676144, -3.1253241424539383e-18},
        {0.15499674192394097, 9.585415594114324e-18},
        {0.18534794999569476, 4.180692268843079e-18},
        {0.21535769969773805, 4.738160130078733e-19},
        {0.24497866312686414, 1.0698755618734451e-17},
        {0.2741674511196588, 8.261353575163773e-18},
        {0.3028848683749714, -1.1010827903001369e-17},
        {0.3310960767041321, -7.952610375793799e-18},
        {0.35877067027057225, -2.4623815582638635e-17},
        {0.38588266939807375, 2.378822732491941e-17},
        {0.4124104415973873, -1.587652227770689e-17},
        {0.43833655985795783, -2.494277030626541e-17},
        {0.4636476090008061, 2.2698777452961687e-17},
        {0.48833395105640554, -1.1373236189329585e-17},
        {0.5123894603107377, -2.5462781472855804e-17},
        {0.5358112379604637, -4.0637956834825575e-18},
        {0.5585993153435624, -5.4556305485916264e-18},
        {0.5807563535676704, -1.441464378193067e-17},
        {0.6022873461349642, 2.950430737228402e-17},
        {0.6231993299340659, 2.672403885140095e-17},
        {0.6435011087932844, 1.5834785051444286e-17},
        {0.6632029927060933, -3.076054864429649e-17},
        {0.6823165548747481, 6.943223671560008e-18},
        {0.7008544078844502, -1.987626234335816e-17},
        {0.7188299996216245, -2.1478388444456983e-17},
        {0.7362574289814281, 3.473937648299457e-17},
        {0.7531512809621944, -2.4256934659182068e-17},
        {0.7695264804056583, -3.704991905602721e-17},
        {0.7853981633974483, 3.061616997868383e-17},
    };
    constexpr double kPio2Hi = 1.5707963267948966, kPio2Lo = 6.123233995736766e-17;
    if (x != x || y != y) return x + y;
    const double ax = fabs(x), ay = fabs(y);
    const bool swap = ay > ax;                       // the angle is measured from the y axis
    const bool neg_x = signbit(x);
    double q;
    if (ax == ay) q = (ax == 0.0) ? 0.0 : 1.0;       // 0 / 0 and inf / inf
    else q = swap ? ax / ay : ay / ax;
    double hi, lo;                                   // atan(q) = hi + lo
    if (q < 0.046875) {
        hi = q;
        lo = vigo_atan_series(q);
    } else {
        const int k = (int)(q * 32.0 + 0.5);
        const double c = (double)k / 32.0;
        const double t = (q - c) / (1.0 + q * c);
        hi = kAtan32[k][0];
        lo = kAtan32[k][1] + (t + vigo_atan_series(t));
    }
    double r;
    if (!swap && !neg_x) {
        r = hi + lo;
    } else {
        // base -/+ atan(q): base = pi/2 (swap) or pi; the sign is minus for (swap, x >= 0) and (no swap, x < 0)
        const double bh = swap ? kPio2Hi : 2.0 * kPio2Hi, bl = swap ? kPio2Lo : 2.0 * kPio2Lo;
        const bool minus = swap != neg_x;
        const double h = minus ? -hi : hi, l = minus ? -lo : lo;
        const double s = bh + h;
        const double e = (bh - s) + h;               // exact: |bh| >= |h|
        r = s + (e + (bl + l));
    }
    return signbit(y) ? -r : r;
}

struct GuideAtan2 {
    VIGO_HD double operator()(double y, double x) const { return vigo_atan2(y, x); }
};

// ---- vectors (mini_eigen.h's order of evaluation) -------------------------------------------------------------------
struct G3 {
    double v[3];
};
VIGO_HD G3 g3(double x, double y, double z) { G3 r; r.v[0] = x; r.v[1] = y; r.v[2] = z; return r; }
VIGO_HD G3 g3_load(const double* p) { return g3(p[0], p[1], p[2]); }
VIGO_HD G3 g3_add(const G3& a, const G3& b) { return g3(a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2]); }
VIGO_HD G3 g3_sub(const G3& a, const G3& b) { return g3(a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]); }
VIGO_HD G3 g3_scale(const G3& a, double s) { return g3(a.v[0] * s, a.v[1] * s, a.v[2] * s); }
VIGO_HD G3 g3_div(const G3& a, double s) { return g3(a.v[0] / s, a.v[1] / s, a.v[2] / s); }
VIGO_HD double g3_dot(const G3& a, const G3& b) { return (a.v[0] * b.v[0] + a.v[1] * b.v[1]) + a.v[2] * b.v[2]; }
VIGO_HD double g3_norm(const G3& a) { return sqrt(g3_dot(a, a)); }
VIGO_HD G3 g3_cross(const G3& a, const G3& b) {
    return g3(a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]);
}

// utils.h: angleBetweenVectors
template <class Atan>
VIGO_HD double guide_angle(const Atan& at, const G3& a, const G3& b) {
    return at(g3_norm(g3_cross(a, b)), g3_dot(a, b));
}

// ---- checkCollisionLine (BT.h:196-204) ------------------------------------------------------------------------------
// sample s of a line check sits at a = res + res + ... (s additions onto 0.0); the check has guide_line_samples(res)
VIGO_HD double guide_line_a(double res, int s) {
    double a = 0.0;
    for (int k = 0; k < s; ++k) a += res;
    return a;
}
VIGO_HD int guide_line_samples(double res) {
    int n = 0;
    for (double a = 0.0; a <= 1.0; a += res) ++n;
    return n;
}
VIGO_HD G3 guide_line_point(const G3& p1, const G3& p2, double a) { return g3_add(g3_scale(p1, a), g3_scale(p2, 1 - a)); }

template <class Occ>
VIGO_HD bool guide_line_hit(const Occ& occ, const G3& p1, const G3& p2, double res) {
    for (double a = 0.0; a <= 1.0; a += res) {
        const G3 m = guide_line_point(p1, p2, a);
        if (occ(m.v[0], m.v[1], m.v[2])) return true;
    }
    return false;
}

// ---- shortcutPath (BT.h:206-240): path[n] -> sc, returns the number of points (<= n) --------------------------------
template <class Occ>
VIGO_HD int guide_shortcut(const Occ& occ, double res, const double* path, int n, G3* sc) {
    int m = 0, ptr1 = 0, ptr2 = 2;
    sc[m++] = g3_load(path);
    if (n == 1) return m;
    if (n == 2) { sc[m++] = g3_load(path + 3); return m; }
    while (true) {
        if (ptr2 > n - 1) break;
        if (!guide_line_hit(occ, g3_load(path + 3 * ptr1), g3_load(path + 3 * ptr2), res)) {
            if (ptr2 >= n - 1) { sc[m++] = g3_load(path + 3 * ptr2); break; }
            ++ptr2;
        } else {
            sc[m++] = g3_load(path + 3 * (ptr2 - 1));
            ptr1 = ptr2 - 1;
            ptr2 = ptr1 + 2;
        }
    }
    return m;
}

// ---- findGuidePointSemiCircle (BT.h:251-304) ----------------------------------------------------------------------
struct GuideFrame {
    double target;
    G3 pseudo, dir;
};
VIGO_HD void guide_frame(GuideFrame& F, int idx, int first, int second, const G3& p0, const G3& pback) {
    const double minAngle = 0.0, maxAngle = kGuidePi;
    const int numControlpoints = second - first - 1;
    if (numControlpoints != 0) {
        const int order = idx - first;
        double targetAngle = order * kGuidePi / (numControlpoints + 2);
        const double lo = (minAngle < targetAngle) ? targetAngle : minAngle;      // std::max(minAngle, targetAngle)
        F.target = (maxAngle < lo) ? maxAngle : lo;                               // std::min(.., maxAngle)
        const double ratio = double(order) / double(numControlpoints + 1.0);
        F.pseudo = g3_add(g3_scale(g3_sub(pback, p0), ratio), p0);
    } else {
        F.target = kGuidePi / 2.0;
        F.pseudo = g3_div(g3_add(p0, pback), 2.0);
    }
    F.dir = g3_sub(p0, F.pseudo);
}

template <class Atan>
VIGO_HD bool guide_bracket(const Atan& at, const GuideFrame& F, const G3& wpCurr, const G3& wpNext) {
    const double angleCurr = guide_angle(at, F.dir, g3_sub(wpCurr, F.pseudo));
    const double angleNext = guide_angle(at, F.dir, g3_sub(wpNext, F.pseudo));
    return F.target >= angleCurr && F.target <= angleNext;
}

// step k of the bisection sits at a = 1.0 - 0.1 - 0.1 ... (k subtractions); the walk has guide_bisect_steps() steps
VIGO_HD double guide_bisect_a(int k) {
    double a = 1.0;
    for (int j = 0; j < k; ++j) a -= 0.1;
    return a;
}
VIGO_HD int guide_bisect_steps() {
    int n = 0;
    for (double a = 1.0; a >= 0.0; a -= 0.1) ++n;
    return n;
}
template <class Atan>
VIGO_HD double guide_bisect_eval(const Atan& at, const GuideFrame& F, const G3& wpCurr, const G3& wpNext, double a, G3& tempPoint) {
    tempPoint = g3_add(g3_scale(wpCurr, a), g3_scale(wpNext, 1 - a));
    return guide_angle(at, F.dir, g3_sub(tempPoint, F.pseudo)) - F.target;
}
// 0: the walk goes on; 1: angleDiff == 0; 2: the sign changed against the previous step (prevAngleDiff = 0 at step 0)
VIGO_HD int guide_bisect_event(double angleDiff, double prevAngleDiff) {
    if (angleDiff == 0) return 1;
    if (angleDiff * prevAngleDiff < 0) return 2;
    return 0;
}
VIGO_HD G3 guide_bisect_point(int event, double angleDiff, double prevAngleDiff, const G3& tempPoint, const G3& prevTempPoint) {
    if (event == 1) return tempPoint;
    const double totalDiff = fabs(angleDiff) + fabs(prevAngleDiff);
    return g3_add(g3_scale(g3_sub(tempPoint, prevTempPoint), fabs(prevAngleDiff) / totalDiff), prevTempPoint);
}

// decision[3] (may be NULL): found, the path segment, the bisection step.  guidePoint is left alone when nothing is found.
template <class Atan>
VIGO_HD bool guide_find(const Atan& at, int idx, int first, int second, const G3* path, int n, G3& guidePoint, int32_t* decision) {
    GuideFrame F;
    guide_frame(F, idx, first, second, path[0], path[n - 1]);
    if (decision) { decision[0] = 0; decision[1] = -1; decision[2] = -1; }
    for (int i = 0; i + 1 < n; ++i) {
        const G3 wpCurr = path[i], wpNext = path[i + 1];
        if (!guide_bracket(at, F, wpCurr, wpNext)) continue;
        double prevAngleDiff = 0.0;
        G3 prevTempPoint = g3(0, 0, 0);
        int k = 0;
        for (double a = 1.0; a >= 0.0; a -= 0.1, ++k) {
            G3 tempPoint;
            const double angleDiff = guide_bisect_eval(at, F, wpCurr, wpNext, a, tempPoint);
            const int ev = guide_bisect_event(angleDiff, prevAngleDiff);
            if (ev) {
                guidePoint = guide_bisect_point(ev, angleDiff, prevAngleDiff, tempPoint, prevTempPoint);
                if (decision) { decision[0] = 1; decision[1] = i; decision[2] = k; }
                return true;
            }
            prevAngleDiff = angleDiff;
            prevTempPoint = tempPoint;
        }
    }
    return false;
}

// ---- assignGuidePointsSemiCircle (BT.cpp:517-571) ---------------------------------------------------------------------
// the pairs segment (first, second) pushes onto control point idx of N: an interior point one; a segment without
// interior points one onto each of first-1 .. second+1 inside [3, N-4]
VIGO_HD int guide_pushes(int N, int first, int second, int idx) {
    int n = 0;
    if (idx > first && idx < second && idx >= 0 && idx < N) ++n;
    if (second - first - 1 == 0 && idx >= first - 1 && idx <= second + 1 && idx >= 3 && idx <= N - 3 - 1) ++n;
    return n;
}
// ... and onto all control points together
VIGO_HD int guide_pushes_total(int N, int first, int second) {
    const int lo = first + 1 > 0 ? first + 1 : 0, hi = second < N ? second : N;
    int n = hi > lo ? hi - lo : 0;
    if (second - first - 1 == 0) {
        const int l2 = first - 1 > 3 ? first - 1 : 3, h2 = second + 1 < N - 4 ? second + 1 : N - 4;
        if (h2 >= l2) n += h2 - l2 + 1;
    }
    return n;
}
// what the entries refuse: index arithmetic that would overflow, a segment without interior points whose own ends are
// not control points (the step reads them), a path without a point
VIGO_HD bool guide_segment_ok(int N, int first, int second, int path_len) {
    if (first < -kGuideMaxIndex || first > kGuideMaxIndex || second < -kGuideMaxIndex || second > kGuideMaxIndex) return false;
    if (second - first - 1 == 0 && (first < 0 || second >= N)) return false;
    return path_len >= 1;
}
VIGO_HD void guide_direction(const G3& guidePoint, const G3& from, G3& dir) {
    const G3 diff = g3_sub(guidePoint, from);
    dir = g3_div(diff, g3_norm(diff));
}

// One trajectory: ctrl[N][3], n_seg segments seg[k][2] with paths path[path_off[k] .. path_off[k + 1]) (the caller has
// applied the min(collisionSeg.size(), paths.size()) bound).  sc: room for the longest path.  emit(idx, point,
// direction, decision[3]) is called in push order.
template <class Occ, class Atan, class Emit>
VIGO_HD void guide_assign(const Occ& occ, const Atan& at, double res, int N, const double* ctrl, int n_seg, const int32_t* seg,
                          const int32_t* path_off, const double* path, G3* sc, Emit emit) {
    G3 guidePoint = g3(0, 0, 0), guideDirection;
    int32_t dec[3];
    for (int i = 0; i < n_seg; ++i) {
        const int first = seg[2 * i], second = seg[2 * i + 1];
        const int n = guide_shortcut(occ, res, path + 3 * (size_t)path_off[i], path_off[i + 1] - path_off[i], sc);
        const int lo = first + 1 > 0 ? first + 1 : 0, hi = second < N ? second : N;     // (the idx < 0 || idx >= N skip)
        for (int idx = lo; idx < hi; ++idx) {
            guide_find(at, idx, first, second, sc, n, guidePoint, dec);
            guide_direction(guidePoint, g3_load(ctrl + 3 * (size_t)idx), guideDirection);
            emit(idx, guidePoint, guideDirection, dec);
        }
        if (second - first - 1 == 0) {  // line collision
            guide_find(at, first, first, second, sc, n, guidePoint, dec);
            const G3 midPoint = g3_div(g3_add(g3_load(ctrl + 3 * (size_t)first), g3_load(ctrl + 3 * (size_t)second)), 2.0);
            guide_direction(guidePoint, midPoint, guideDirection);
            for (int idx = first - 1; idx <= second + 1; ++idx)
                if (idx >= 3 && idx <= N - 3 - 1) emit(idx, guidePoint, guideDirection, dec);
        }
    }
}

}  // namespace vigo
