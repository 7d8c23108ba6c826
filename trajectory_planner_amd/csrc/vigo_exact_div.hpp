// vigo_exact_div.hpp — two rules that give the bits of a long fp64 operation sequence from a short one, each with the
// set of inputs for which that holds; outside the set the caller runs the long sequence itself.
//
//   1. a / d for a divisor d that stays the same over many divisions (ConstDiv): Markstein's three operations on the
//      stored reciprocal instead of the 13-instruction fp64 division.
//   2. the L-BFGS convergence test  sqrt(G) / max(sqrt(X), 1) <= eps  (conv_filter): a comparison of squares with a
//      guard band instead of two square roots and a division.
//
// Plain C++ with explicit __builtin_fma, no contraction wanted or needed (-ffp-contract=off everywhere): a CPU program
// compiles the very text the kernel uses (tests/exact_div_check.cpp).  Round-to-nearest-even, no flush to zero.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_DIV_HD __host__ __device__ __forceinline__
#else
#define VIGO_DIV_HD inline
#endif

namespace vigo {

// |a| in [2^-500, 2^500): the range rule of the two-loop's YSv<false> / exp_in_safe_range.  False for 0, denormals, inf
// and NaN.
VIGO_DIV_HD bool exact_div_in_range(double a) { return __builtin_fabs(a) >= 0x1p-500 && __builtin_fabs(a) < 0x1p500; }

// ---- 1. division by a constant ---------------------------------------------------------------------------------------
// r = RN(1 / d) for a d in range, else NaN; lim = 2^500 for a d in range, else 0.
//
// CONTRACT.  quotient(a) has the bits of a / d whenever usable(a) and (a == +0 or |a| >= 2^-500):
//   * d in range and |a| in [2^-500, 2^500): q = RN(a r) is within one ulp of a / d, e = RN(a - q d) is exact (a
//     multiple of ulp(q) ulp(d) >= 2^-105 |a| >= 2^-605 that is at most ulp(q) |d| in magnitude: it fits 53 bits and
//     is no denormal), and q' = RN(q + e r) is then RN(a / d) by Markstein's theorem (1990) for a correctly rounded r.
//     |q| lies in (2^-1001, 2^1001): nothing overflows or underflows.  The same sequence under the same rule as
//     over_ys<MARK> in vigo_solver.hip.
//   * a = +0: q = (+0) r has the sign of d, e = RN(-q d + (+0)) = (-0) + (+0) = +0 for either sign of d, and
//     q' = RN((+0) r + q) = q = (+0) / d.
//   * usable(a) is false for a NaN, an infinity, every |a| >= 2^500, and for EVERY a when d is out of range (lim = 0,
//     r = NaN: nothing is below 0): the caller divides.
// NOT covered, although usable(a) holds: a = -0, where q' = +0 for d > 0 (a / d = -0), and 0 < |a| < 2^-500, where e may
// be rounded.  For those the sequence still gives
//   * |q'| <= 1, as |a / d| < 1 is: (q normal) q = (a / d)(1 + t), |t| <= 2^-52, so e = RN(-a t) up to 2^-1075 and
//     q + e r = (a / d)(1 + O(2^-104)) + O(2^-575), whose rounding cannot pass 1 when |a / d| < 1 — the doubles next
//     to 1 are 2^-53 away; (q denormal or zero) |a| < 2^-521, |e| <= |a| + |q d| < 2^-520 and |q'| < 2^-19.
// So a caller that looks only at whether the quotient exceeds 1 in magnitude, and not at the sign of a zero, may use
// quotient(a) for every usable(a).  The velocity stencil's first division is such a caller (stencil_axis).
//
// lim2 = min(2^500, 2^498 |d|) (0 for a d out of range) bounds a CHAIN of two divisions, the second dividend made of the
// first quotient: usable2(a) implies usable(a) and usable(b) for every |b| <= 2 |quotient(a)|, since |a / d| < 2^498
// and rounding is monotone (and |quotient(a)| <= 1 for the |a| below 2^-500, above).  One test, on the first dividend,
// then answers for both divisions.
struct ConstDiv {
    double d, r, lim, lim2;
    VIGO_DIV_HD bool usable(double a) const { return __builtin_fabs(a) < lim; }
    VIGO_DIV_HD bool usable2(double a) const { return __builtin_fabs(a) < lim2; }
    VIGO_DIV_HD double quotient(double a) const {
        const double q = a * r;
        const double e = __builtin_fma(-q, d, a);
        return __builtin_fma(e, r, q);
    }
};
VIGO_DIV_HD ConstDiv make_const_div(double d) {
    const bool ok = exact_div_in_range(d);
    const double l2 = 0x1p498 * __builtin_fabs(d);
    return ConstDiv{d, ok ? 1.0 / d : __builtin_nan(""), ok ? 0x1p500 : 0.0, ok ? (l2 < 0x1p500 ? l2 : 0x1p500) : 0.0};
}

// ---- 2. the convergence test -----------------------------------------------------------------------------------------
// The reference expression (LB:1154-1157, :1200-1225), G = g.g and X = x.x:
VIGO_DIV_HD bool conv_reference(double G, double X, double eps) {
    double xn = __builtin_sqrt(X);
    const double gn = __builtin_sqrt(G);
    if (xn < 1.0) xn = 1.0;
    return gn / xn <= eps;
}

// eps2 = RN(eps^2) and whether the filter may run at all: eps = +-0, or eps positive with |eps| in [2^-250, 2^250) (so
// that eps2 is normal with one rounding and c below stays within 2^+-1000).  A negative or NaN eps: never.
struct ConvFilter {
    double eps2;
    bool ok;
};
VIGO_DIV_HD ConvFilter make_conv_filter(double eps) {
    return ConvFilter{eps * eps, eps == 0.0 || (eps >= 0x1p-250 && eps < 0x1p250)};
}

// conv_filter: +1 = the reference says converged, 0 = it says not converged, -1 = undecided: evaluate conv_reference.
//
// CONTRACT.  A decision (0 or +1) is conv_reference(G, X, eps).  Decisions are made only for F.ok and G, X both in
// [2^-500, 2^500) (false for zero, denormal, negative, infinite and NaN sums).  There:
//   * rho = sqrt(G) / max(sqrt(X), 1) in exact arithmetic; max(RN(sqrt X), 1) is 1 for X <= 1 and RN(sqrt X) >= 1
//     otherwise (RN is monotone and sqrt(1) = 1), so the reference's three roundings — both roots lie in 2^+-250, the
//     quotient in 2^+-500, nothing underflows — give rho' = rho (1 + t) with |t| < 2^-51, and rho^2 = G / max(X, 1).
//   * c = RN(max(X, 1) eps2) = max(X, 1) eps^2 (1 + u), |u| < 2^-51 (two roundings of normal numbers), or c = 0 when
//     eps = 0; hi = RN(c (1 + 2^-40)) and lo = RN(c (1 - 2^-40)) add one rounding each.
//   * G > hi  =>  rho^2 > eps^2 (1 + 2^-40)(1 - 2^-50) > eps^2 (1 + 2^-41)  =>  rho > eps (1 + 2^-43)
//            =>  rho' > eps (1 + 2^-43)(1 - 2^-51) > eps: not converged.  With eps = 0: hi = 0 < G, and rho' > 0 = eps.
//   * G < lo  =>  rho^2 < eps^2 (1 - 2^-41)  =>  rho < eps (1 - 2^-43)  =>  rho' < eps: converged.  (eps = 0: lo = 0,
//     never.)
//   * a G inside the band, or any comparison with a NaN: undecided.
// (Straight-line on purpose — & and |, no early return: on the device it is a dozen instructions of one basic block.
// Outside the admitted range c may be anything, a NaN included; `in` masks what is made of it.)
VIGO_DIV_HD int conv_filter(double G, double X, const ConvFilter& F) {
    const bool in = F.ok & (G >= 0x1p-500) & (G < 0x1p500) & (X >= 0x1p-500) & (X < 0x1p500);
    const double c = (X > 1.0 ? X : 1.0) * F.eps2;
    const bool no = G > c * (1.0 + 0x1p-40);
    const bool yes = G < c * (1.0 - 0x1p-40);
    return (in & (no | yes)) ? (int)yes : -1;
}
VIGO_DIV_HD bool conv_test(double G, double X, double eps, const ConvFilter& F) {
    const int f = conv_filter(G, X, F);
    return f >= 0 ? f != 0 : conv_reference(G, X, eps);
}

}  // namespace vigo
