// vigo_linesearch.hpp — the scalar side of one Moré–Thuente line search (solver/lbfgs.hpp LB:716-937 with
// update_trial_interval LB:506-714 and the minimizer macros LB:295-391), as the whole-solve kernel runs it: everything
// between two cost evaluations that is NOT a vector operation.  One trial is
//
//     set-up (interval ends, clamps, step override)  ->  x = xp + step d, evaluation (the kernel's)  ->
//     exit code (LB:832-866)  ->  stage and interval update (LB:868-931)
//
// in two forms that give the same bits:
//   * the GENERIC form, any trial: ls_begin, ls_setup, ls_exit_code, ls_update;
//   * the FIRST-TRIAL form.  On the first trial of a search the bracket state is a set of constants — brackt = 0,
//     uinfo = 0, stage1 = 1, count = 0, xt = yt = 0, xf = yf = finit, xd = yd = dginit — so its set-up is the two clamps
//     (ls_first_setup), only four of the six exits can fire (ls_first_exit_code), and the state itself is needed only if
//     the trial is rejected (ls_first_reject forms it then, from the expressions ls_begin and ls_setup use, on the same
//     operands).  About nine searches in ten accept their first trial.
// Plain C++, no contraction wanted (-ffp-contract=off everywhere): a CPU program compiles the very text the kernel uses
// and holds the first-trial form to the generic one (tests/linesearch_first_trial_check.cpp).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_LS_FN __device__ __forceinline__
#else
#include <cmath>
#define VIGO_LS_FN static inline
#endif

namespace vigo {

// reference status codes, LB:20-80
enum : int {
    LB_CONVERGENCE = 0,
    LB_STOP = 1,
    LB_ALREADY_MINIMIZED = 2,
    LBERR_UNKNOWN = -1024,
    LBERR_LOGIC,
    LBERR_CANCELED,
    LBERR_INVALID_N,
    LBERR_INVALID_MEMSIZE,
    LBERR_INVALID_GEPSILON,
    LBERR_INVALID_TESTPERIOD,
    LBERR_INVALID_DELTA,
    LBERR_INVALID_MINSTEP,
    LBERR_INVALID_MAXSTEP,
    LBERR_INVALID_FDECCOEFF,
    LBERR_INVALID_SCURVCOEFF,
    LBERR_INVALID_XTOL,
    LBERR_INVALID_MAXLINESEARCH,
    LBERR_OUTOFINTERVAL,
    LBERR_INCORRECT_TMINMAX,
    LBERR_ROUNDING_ERROR,
    LBERR_MINIMUMSTEP,
    LBERR_MAXIMUMSTEP,
    LBERR_MAXIMUMLINESEARCH,
    LBERR_MAXIMUMITERATION,
    LBERR_WIDTHTOOSMALL,
    LBERR_INVALIDPARAMETERS,
    LBERR_INCREASEGRADIENT
};

namespace {

// ---- More-Thuente helpers (per-lane scalar code, group-uniform values) -------------------

// LB:308-324
VIGO_LS_FN double cubic_min(double u, double fu, double du, double v, double fv, double dv) {
    double d = v - u;
    double theta = (fu - fv) * 3 / d + du + dv;
    double p = fabs(theta), q = fabs(du), r = fabs(dv);
    double s = p >= q ? p : q;
    s = s >= r ? s : r;
    double a = theta / s;
    double gamm = s * sqrt(a * a - (du / s) * (dv / s));
    if (v < u) gamm = -gamm;
    p = gamm - du + theta;
    q = gamm - du + gamm + dv;
    r = p / q;
    return u + r * d;
}
// LB:338-366
VIGO_LS_FN double cubic_min_bounded(double u, double fu, double du, double v, double fv,
                                    double dv, double xmin, double xmax) {
    double d = v - u;
    double theta = (fu - fv) * 3 / d + du + dv;
    double p = fabs(theta), q = fabs(du), r = fabs(dv);
    double s = p >= q ? p : q;
    s = s >= r ? s : r;
    double a = theta / s;
    double gamm = a * a - (du / s) * (dv / s);
    gamm = gamm > 0 ? s * sqrt(gamm) : 0;
    if (u < v) gamm = -gamm;
    p = gamm - dv + theta;
    q = gamm - dv + gamm + du;
    r = p / q;
    if (r < 0. && gamm != 0.) return v - r * d;
    if (a < 0) return xmax;
    return xmin;
}
// LB:377-379
VIGO_LS_FN double quad_min(double u, double fu, double du, double v, double fv) {
    double a = v - u;
    return u + du / ((fu - fv) / a + du) / 2 * a;
}
// LB:389-391
VIGO_LS_FN double quad_min_secant(double u, double du, double v, double dv) {
    double a = u - v;
    return v + dv / (dv - du) * a;
}

// LB:506-714 on scalars held in registers: (xt,xf,xd) best point, (yt,yf,yd) other end,
// (tt,tf,td) trial; tt receives the new trial step.
VIGO_LS_FN int trial_interval(double& xt, double& xf, double& xd, double& yt, double& yf,
                              double& yd, double& tt, const double tf, const double td,
                              const double tmin, const double tmax, int& brackt) {
    int bound;
    const int dsign = td * (xd / fabs(xd)) < 0.;
    double mc, mq, newt;
    if (brackt) {
        const double lo = xt <= yt ? xt : yt;
        const double hi = xt >= yt ? xt : yt;
        if (tt <= lo || hi <= tt) return LBERR_OUTOFINTERVAL;
        if (0. <= xd * (tt - xt)) return LBERR_INCREASEGRADIENT;
        if (tmax < tmin) return LBERR_INCORRECT_TMINMAX;
    }
    if (xf < tf) {
        brackt = 1;
        bound = 1;
        mc = cubic_min(xt, xf, xd, tt, tf, td);
        mq = quad_min(xt, xf, xd, tt, tf);
        newt = (fabs(mc - xt) < fabs(mq - xt)) ? mc : mc + 0.5 * (mq - mc);
    } else if (dsign) {
        brackt = 1;
        bound = 0;
        mc = cubic_min(xt, xf, xd, tt, tf, td);
        mq = quad_min_secant(xt, xd, tt, td);
        newt = (fabs(mc - tt) > fabs(mq - tt)) ? mc : mq;
    } else if (fabs(td) < fabs(xd)) {
        bound = 1;
        mc = cubic_min_bounded(xt, xf, xd, tt, tf, td, tmin, tmax);
        mq = quad_min_secant(xt, xd, tt, td);
        if (brackt) newt = (fabs(tt - mc) < fabs(tt - mq)) ? mc : mq;
        else        newt = (fabs(tt - mc) > fabs(tt - mq)) ? mc : mq;
    } else {
        bound = 0;
        if (brackt)       newt = cubic_min(tt, tf, td, yt, yf, yd);
        else if (xt < tt) newt = tmax;
        else              newt = tmin;
    }
    {
        // LB:664-684 as value selects (pointer-style conditional copies end up in scratch)
        const bool higher = xf < tf;
        const bool y_from_x = !higher && dsign;
        const double nyt = higher ? tt : (y_from_x ? xt : yt);
        const double nyf = higher ? tf : (y_from_x ? xf : yf);
        const double nyd = higher ? td : (y_from_x ? xd : yd);
        const double nxt = higher ? xt : tt;
        const double nxf = higher ? xf : tf;
        const double nxd = higher ? xd : td;
        xt = nxt; xf = nxf; xd = nxd;
        yt = nyt; yf = nyf; yd = nyd;
    }
    if (tmax < newt) newt = tmax;
    if (newt < tmin) newt = tmin;
    if (brackt && bound) {
        mq = xt + 0.66 * (yt - xt);
        if (xt < yt) { if (mq < newt) newt = mq; }
        else         { if (newt < mq) newt = mq; }
    }
    tt = newt;
    return 0;
}

// ---- one line search as a sequence of trips --------------------------------------------------------------------------
// The text below restates, statement for statement, the line search inside k_optimize's iteration loop (vigo_solver.hip);
// the axis-per-lane instantiation runs it from here.

struct LsParams {   // lbfgs_parameter_t: min_step, max_step, f_dec_coeff, s_curv_coeff, xtol, max_linesearch
    double stpmin, stpmax, ftol, gtol, xtol;
    int max_linesearch;
};

struct LsState {
    double dginit, finit, dgtest;                 // of the search: ls_begin / ls_first_begin
    int count, brackt, stage1, uinfo;             // the rest: ls_begin, or ls_first_reject once the first trial is rejected
    double width, prev_width;
    double xt, xf, xd, yt, yf, yd;                // best point and other end of the interval: step, f, f'
    double stmin, stmax;                          // of the trial under way: ls_setup
};

// LB:744-760 (the two tests), the part of LB:762-781 every trial needs.  Not 0: the search ends before its first trial.
VIGO_LS_FN int ls_first_begin(const LsParams& P, LsState& S, double step, double fx, double dginit) {
    int ls = 0;
    S.dginit = dginit;
    if (step <= 0.) ls = LBERR_INVALIDPARAMETERS;
    else if (0 < dginit) ls = LBERR_INCREASEGRADIENT;
    S.finit = fx;
    S.dgtest = P.ftol * dginit;
    S.count = 0;
    return ls;
}
// ... and the rest of LB:762-781: the state of a search that has not tried anything yet
VIGO_LS_FN void ls_init_state(const LsParams& P, LsState& S) {
    S.brackt = 0; S.stage1 = 1; S.uinfo = 0;
    S.width = P.stpmax - P.stpmin;
    S.prev_width = 2.0 * S.width;
    S.xt = S.yt = 0.;
    S.xf = S.yf = S.finit;
    S.xd = S.yd = S.dginit;
}
VIGO_LS_FN int ls_begin(const LsParams& P, LsState& S, double step, double fx, double dginit) {
    const int ls = ls_first_begin(P, S, step, fx, dginit);
    ls_init_state(P, S);
    return ls;
}

// LB:787-795: the ends of the interval the trial step has to lie in (`step` as it stands BEFORE the clamps)
VIGO_LS_FN void ls_interval(LsState& S, double step) {
    if (S.brackt) {
        S.stmin = S.xt <= S.yt ? S.xt : S.yt;
        S.stmax = S.xt >= S.yt ? S.xt : S.yt;
    } else {
        S.stmin = S.xt;
        S.stmax = step + 4.0 * (step - S.xt);
    }
}
// LB:797-799
VIGO_LS_FN void ls_clamp(const LsParams& P, double& step) {
    if (step < P.stpmin) step = P.stpmin;
    if (P.stpmax < step) step = P.stpmax;
}
// LB:787-811, any trial: interval ends, clamps, and the fall-back to the best step so far
VIGO_LS_FN void ls_setup(const LsParams& P, LsState& S, double& step) {
    ls_interval(S, step);
    ls_clamp(P, step);
    if ((S.brackt && ((step <= S.stmin || S.stmax <= step) || P.max_linesearch <= S.count + 1 || S.uinfo != 0)) ||
        (S.brackt && (S.stmax - S.stmin <= P.xtol * S.stmax))) {
        step = S.xt;
    }
}
// the first trial: brackt = 0 leaves the clamps.  The caller keeps the step as it was for ls_first_reject.
VIGO_LS_FN void ls_first_setup(const LsParams& P, double& step) { ls_clamp(P, step); }

// LB:830: the sufficient-decrease bound of the trial at `step`
VIGO_LS_FN double ls_ftest1(const LsState& S, double step) { return S.finit + step * S.dgtest; }

// LB:832-866 after the evaluation (fx, dg) at `step`, S.count already counting this trial: six exits tested in order,
// the first that holds wins.  Evaluated as one select chain in reverse order (six exec-mask branches cost more issue
// slots than the compares).  0: the search goes on.
VIGO_LS_FN int ls_exit_code(const LsParams& P, const LsState& S, double step, double fx, double dg, double ftest1) {
    int code = 0;
    if (fx <= ftest1 && fabs(dg) <= P.gtol * (-S.dginit)) code = S.count;                              // LB:862-866 (count >= 1)
    if (P.max_linesearch <= S.count) code = LBERR_MAXIMUMLINESEARCH;                                   // LB:857-860
    if (S.brackt && (S.stmax - S.stmin) <= P.xtol * S.stmax) code = LBERR_WIDTHTOOSMALL;               // LB:852-855
    if (step == P.stpmin && (ftest1 < fx || S.dgtest <= dg)) code = LBERR_MINIMUMSTEP;                 // LB:847-850
    if (step == P.stpmax && fx <= ftest1 && dg <= S.dgtest) code = LBERR_MAXIMUMSTEP;                  // LB:842-845
    if (S.brackt && ((step <= S.stmin || S.stmax <= step) || S.uinfo != 0)) code = LBERR_ROUNDING_ERROR;   // LB:837-840
    return code;
}
// the first trial (S.count == 1): the four exits that can fire without a bracket, in the same order
VIGO_LS_FN int ls_first_exit_code(const LsParams& P, const LsState& S, double step, double fx, double dg, double ftest1) {
    int code = 0;
    if (fx <= ftest1 && fabs(dg) <= P.gtol * (-S.dginit)) code = 1;
    if (P.max_linesearch <= 1) code = LBERR_MAXIMUMLINESEARCH;
    if (step == P.stpmin && (ftest1 < fx || S.dgtest <= dg)) code = LBERR_MINIMUMSTEP;
    if (step == P.stpmax && fx <= ftest1 && dg <= S.dgtest) code = LBERR_MAXIMUMSTEP;
    return code;
}
// the first trial is rejected: the state ls_begin and ls_setup would have handed to ls_update.  step0 is the step the
// search was entered with, before ls_first_setup's clamps.
VIGO_LS_FN void ls_first_reject(const LsParams& P, LsState& S, double step0) {
    ls_init_state(P, S);
    ls_interval(S, step0);
}

// LB:868-931 after a trial that did not end the search: the stage switch, the interval update on the function or, while
// stage 1 holds and the decrease is insufficient, on the modified function (one call site, operands selected here), and
// the bisection guard.  `step` receives the next trial step, still to go through ls_setup.
VIGO_LS_FN void ls_update(const LsParams& P, LsState& S, double& step, double fx, double dg, double ftest1) {
    const double cmin = P.ftol <= P.gtol ? P.ftol : P.gtol;
    if (S.stage1 && fx <= ftest1 && cmin * S.dginit <= dg) S.stage1 = 0;

    const bool mod = S.stage1 && ftest1 < fx && fx <= S.xf;
    double axf = mod ? S.xf - S.xt * S.dgtest : S.xf, axd = mod ? S.xd - S.dgtest : S.xd;
    double ayf = mod ? S.yf - S.yt * S.dgtest : S.yf, ayd = mod ? S.yd - S.dgtest : S.yd;
    const double atf = mod ? fx - step * S.dgtest : fx, atd = mod ? dg - S.dgtest : dg;
    S.uinfo = trial_interval(S.xt, axf, axd, S.yt, ayf, ayd, step, atf, atd, S.stmin, S.stmax, S.brackt);
    S.xf = mod ? axf + S.xt * S.dgtest : axf;
    S.yf = mod ? ayf + S.yt * S.dgtest : ayf;
    S.xd = mod ? axd + S.dgtest : axd;
    S.yd = mod ? ayd + S.dgtest : ayd;

    if (S.brackt) {
        if (0.66 * S.prev_width <= fabs(S.yt - S.xt)) step = S.xt + 0.5 * (S.yt - S.xt);
        S.prev_width = S.width;
        S.width = fabs(S.yt - S.xt);
    }
}

}  // namespace
}  // namespace vigo
