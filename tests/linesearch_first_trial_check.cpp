// linesearch_first_trial_check: csrc/vigo_linesearch.hpp on the CPU — the first-trial form of a Moré–Thuente trip held to
// the generic form, bit for bit, from the same state (tests/test_linesearch_first_trial.py builds and runs it; host
// compiler, -O2 -ffp-contract=off).  For every input the two forms run side by side:
//
//   generic:      ls_begin        ls_setup        [fx, dg]  ls_exit_code                          ls_update  ls_setup
//   first trial:  ls_first_begin  ls_first_setup  [fx, dg]  ls_first_exit_code  ls_first_reject   ls_update  ls_setup
//
// and then, from the state each holds, one more generic trip on [fx2, dg2].  Compared with == on the bit patterns: the
// code of the begin, the step after the set-up, ftest1, the exit code, every field of the state handed to the second
// trip (after ls_first_reject, and again after ls_update and ls_setup), the second trip's exit code, step and state.
// Exits 1 at the first difference.  Prints "name value" lines: how many inputs went which way.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "vigo_linesearch.hpp"

using namespace vigo;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static double unit() { return (double)(rnd() >> 11) * 0x1p-53; }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
static double from_bits(uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; }
static bool same(double a, double b) { return bits(a) == bits(b); }

static bool same_state(const LsState& a, const LsState& b) {
    return same(a.dginit, b.dginit) && same(a.finit, b.finit) && same(a.dgtest, b.dgtest) && a.count == b.count &&
           a.brackt == b.brackt && a.stage1 == b.stage1 && a.uinfo == b.uinfo && same(a.width, b.width) &&
           same(a.prev_width, b.prev_width) && same(a.xt, b.xt) && same(a.xf, b.xf) && same(a.xd, b.xd) &&
           same(a.yt, b.yt) && same(a.yf, b.yf) && same(a.yd, b.yd) && same(a.stmin, b.stmin) && same(a.stmax, b.stmax);
}

static const double kInf = std::numeric_limits<double>::infinity();
static double special() {
    static const double tab[] = {0.0, -0.0, kInf, -kInf, std::numeric_limits<double>::quiet_NaN(),
                                 -std::numeric_limits<double>::quiet_NaN(), 4.9406564584124654e-324, -4.9406564584124654e-324,
                                 2.2250738585072009e-308, -1.1125369292536007e-308, 1.7976931348623157e308, -1.7976931348623157e308};
    const uint64_t r = rnd();
    if ((r & 15) == 0) return from_bits(0x7FF0000000000001ull | (rnd() & 0x800FFFFFFFFFFFFFull));   // a NaN with a payload
    return tab[(r >> 8) % (sizeof tab / sizeof tab[0])];
}
// a double with a sign chosen by the caller and a magnitude spread over 2^+-span
static double mag(int span) { return (1.0 + unit()) * std::ldexp(1.0, (int)(rnd() % (2 * span + 1)) - span); }

static long long n_cases, n_begin_error, n_accept, n_maxls, n_minstep, n_maxstep, n_rejected, n_second_exit, n_second_on,
    n_clamped_lo, n_clamped_hi, n_special, n_mod, n_bracketed;

static int fail(const char* what, const LsParams& P, double step, double finit, double dginit, double fx, double dg) {
    std::printf("ok 0\nMISMATCH %s: stpmin %a stpmax %a ftol %a gtol %a xtol %a max_linesearch %d step %a finit %a dginit %a fx %a dg %a\n",
                what, P.stpmin, P.stpmax, P.ftol, P.gtol, P.xtol, P.max_linesearch, step, finit, dginit, fx, dg);
    return 1;
}

static int one(const LsParams& P, double step_in, double finit, double dginit, double fx, double dg, double fx2, double dg2) {
    ++n_cases;
    LsState G{}, F{};
    double sg = step_in, sf = step_in;
    const int bg = ls_begin(P, G, sg, finit, dginit);
    const int bf = ls_first_begin(P, F, sf, finit, dginit);
    if (bg != bf) return fail("begin", P, step_in, finit, dginit, fx, dg);
    if (bg != 0) { ++n_begin_error; return 0; }
    const double step0 = sf;
    ls_setup(P, G, sg);
    ls_first_setup(P, sf);
    if (!same(sg, sf)) return fail("step after the set-up", P, step_in, finit, dginit, fx, dg);
    if (sg == P.stpmin && !(step_in == P.stpmin)) ++n_clamped_lo;
    if (sg == P.stpmax && !(step_in == P.stpmax)) ++n_clamped_hi;
    const double tg = ls_ftest1(G, sg), tf = ls_ftest1(F, sf);
    if (!same(tg, tf)) return fail("ftest1", P, step_in, finit, dginit, fx, dg);
    ++G.count; ++F.count;
    const int cg = ls_exit_code(P, G, sg, fx, dg, tg);
    const int cf = ls_first_exit_code(P, F, sf, fx, dg, tf);
    if (cg != cf) return fail("exit code", P, step_in, finit, dginit, fx, dg);
    if (cg != 0) {
        if (cg == 1) ++n_accept;
        else if (cg == LBERR_MAXIMUMLINESEARCH) ++n_maxls;
        else if (cg == LBERR_MINIMUMSTEP) ++n_minstep;
        else if (cg == LBERR_MAXIMUMSTEP) ++n_maxstep;
        else return fail("an exit that needs a bracket", P, step_in, finit, dginit, fx, dg);
        return 0;
    }
    ++n_rejected;
    ls_first_reject(P, F, step0);
    if (!same_state(G, F)) return fail("state handed to the update", P, step_in, finit, dginit, fx, dg);
    if (G.stage1 && tg < fx && fx <= G.xf) ++n_mod;
    ls_update(P, G, sg, fx, dg, tg);
    ls_update(P, F, sf, fx, dg, tf);
    ls_setup(P, G, sg);
    ls_setup(P, F, sf);
    if (!same_state(G, F) || !same(sg, sf)) return fail("state handed to the second trip", P, step_in, finit, dginit, fx, dg);
    if (G.brackt) ++n_bracketed;
    // the second trip
    const double tg2 = ls_ftest1(G, sg), tf2 = ls_ftest1(F, sf);
    ++G.count; ++F.count;
    const int cg2 = ls_exit_code(P, G, sg, fx2, dg2, tg2);
    const int cf2 = ls_exit_code(P, F, sf, fx2, dg2, tf2);
    if (cg2 != cf2 || !same(tg2, tf2)) return fail("second trip's exit code", P, step_in, finit, dginit, fx, dg);
    if (cg2 != 0) { ++n_second_exit; return 0; }
    ++n_second_on;
    ls_update(P, G, sg, fx2, dg2, tg2);
    ls_update(P, F, sf, fx2, dg2, tf2);
    ls_setup(P, G, sg);
    ls_setup(P, F, sf);
    if (!same_state(G, F) || !same(sg, sf)) return fail("second trip's result", P, step_in, finit, dginit, fx, dg);
    return 0;
}

int main() {
    const double stpmins[] = {1e-20, 1e-3, 1.5, 0.0};
    const double stpmaxs[] = {1e20, 0.5, 1e-2, 3.0};
    const double ftols[] = {1e-4, 0.3}, gtols[] = {0.9, 0.31}, xtols[] = {1e-16, 0.5, 0.9};
    const int maxls[] = {40, 1, 2, 40};
    const long long kCases = 4000000;
    for (long long i = 0; i < kCases; ++i) {
        const uint64_t r = rnd();
        const int tol = (int)((r >> 4) & 1);
        LsParams P{stpmins[r & 3], stpmaxs[(r >> 2) & 3], ftols[tol], gtols[tol], xtols[(r >> 5) % 3], maxls[(r >> 8) & 3]};
        if (P.stpmax < P.stpmin) P.stpmax = P.stpmin * 4;
        // the step: random, at either limit, one ulp either side of it, outside (the clamp lands on the limit)
        double step;
        switch ((r >> 12) % 8) {
            case 0: step = P.stpmin; break;
            case 1: step = P.stpmax; break;
            case 2: step = P.stpmin * (unit() < 0.5 ? 0.25 : 1.0 + 0x1p-52); break;
            case 3: step = P.stpmax * (unit() < 0.5 ? 4.0 : 1.0 - 0x1p-53); break;
            case 4: step = (unit() < 0.1 ? -1.0 : 1.0) * mag(80); break;
            default: step = mag(6); break;
        }
        // the search: a descent direction mostly; the trial mostly near what a quadratic along it would give
        double dginit = -mag((r >> 16) & 1 ? 4 : 40), finit = (unit() < 0.2 ? -1.0 : 1.0) * mag(10);
        if (unit() < 0.03) dginit = -dginit;
        const double curv = mag(3);
        auto trial = [&](double s, double& f, double& g) {
            f = finit + s * dginit + 0.5 * curv * s * s * (unit() < 0.3 ? mag(3) : 1.0);
            g = dginit + curv * s * (unit() < 0.3 ? mag(3) : 1.0);
            if (unit() < 0.15) f = finit + s * (P.ftol * dginit) * (unit() < 0.5 ? 1.0 : 1.0 + 0x1p-52);   // at the decrease bound
            if (unit() < 0.1) g = P.ftol * dginit;                                                          // dg == dgtest
        };
        double sc = step;
        if (sc < P.stpmin) sc = P.stpmin;
        if (P.stpmax < sc) sc = P.stpmax;
        double fx, dg, fx2, dg2;
        trial(sc, fx, dg);
        trial(sc * unit(), fx2, dg2);
        bool sp = false;
        if ((r >> 20) % 8 == 0) {   // zeros of both signs, infinities, NaN, denormals, the largest doubles
            const uint64_t w = rnd();
            if (w & 1) fx = special();
            if (w & 2) dg = special();
            if (w & 4) finit = special();
            if (w & 8) dginit = special();
            if (w & 16) fx2 = special();
            if (w & 32) dg2 = special();
            sp = (w & 15) != 0;
        }
        if (sp) ++n_special;
        if (one(P, step, finit, dginit, fx, dg, fx2, dg2)) return 1;
    }
    std::printf("ok 1\ncases %lld\nspecial_values %lld\nbegin_errors %lld\naccepted %lld\nmax_linesearch %lld\nminimum_step %lld\n"
                "maximum_step %lld\nrejected %lld\nmodified_function %lld\nbracketed %lld\nclamped_to_stpmin %lld\nclamped_to_stpmax %lld\n"
                "second_trip_exits %lld\nsecond_trip_goes_on %lld\n",
                n_cases, n_special, n_begin_error, n_accept, n_maxls, n_minstep, n_maxstep, n_rejected, n_mod, n_bracketed,
                n_clamped_lo, n_clamped_hi, n_second_exit, n_second_on);
    return 0;
}
