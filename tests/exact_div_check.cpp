// exact_div_check: csrc/vigo_exact_div.hpp on the CPU, against the operations its two rules stand in for.
// Built by tests/test_exact_div.py with the host compiler at -O2 -ffp-contract=off; prints its figures, one
// "name value" per line, and exits 1 with a message at the first broken contract.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vigo_exact_div.hpp"

using vigo::ConstDiv;
using vigo::ConvFilter;

static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, sizeof u); return u; }
static double from_bits(uint64_t u) { double x; memcpy(&x, &u, sizeof x); return x; }
static double make(int sign, int biased_exp, uint64_t mant) {
    return from_bits(((uint64_t)sign << 63) | ((uint64_t)biased_exp << 52) | (mant & 0xfffffffffffffull));
}
static const uint64_t kOnes = 0xfffffffffffffull;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static double rnd_unit() { return (double)(rnd() >> 11) * 0x1p-53; }
// sign and significand random, binary exponent uniform in [lo, hi)
static double rnd_exp(int lo, int hi) { return make(rnd() & 1, 1023 + lo + (int)(rnd() % (uint64_t)(hi - lo)), rnd()); }

[[noreturn]] static void fail(const char* what, double a, double b, double c) {
    printf("FAILED %s: %a %a %a\n", what, a, b, c);
    exit(1);
}

// the stencil's excess() (vigo_solver.hip, limits 1.0)
static double excess(double v) { return v > 1.0 ? v - 1.0 : (v < -1.0 ? v + 1.0 : 0.0); }

// ---- the division ------------------------------------------------------------------------------------------------------
static long n_div = 0, n_fallback = 0, n_exact = 0, n_chain = 0;

static void check_div(const ConstDiv& cd, double a) {
    const double d = cd.d, ref = a / d;
    const bool d_ok = vigo::exact_div_in_range(d);
    ++n_div;
    // usable is exactly: d in range and |a| < 2^500 (false for NaN and infinity)
    if (cd.usable(a) != (d_ok && fabs(a) < 0x1p500)) fail("usable", a, d, 0);
    if (cd.usable2(a) != (d_ok && fabs(a) < 0x1p500 && fabs(a) < 0x1p498 * fabs(d))) fail("usable2", a, d, 0);
    if (!cd.usable(a)) { ++n_fallback; return; }       // the caller divides: nothing to compare
    const double q = cd.quotient(a);
    // the chain of the velocity stencil: one test of the first dividend answers for the second, 2 excess(quotient)
    if (cd.usable2(a)) {
        ++n_chain;
        const double b = 2.0 * excess(q);
        if (!cd.usable(b)) fail("usable2(a) without usable(2 excess(quotient(a)))", a, d, b);
        if (bits(cd.quotient(b)) != bits((2.0 * excess(ref)) / d)) fail("the second quotient of the chain", a, d, b);
    }
    // first site: through excess() for EVERY usable dividend
    if (bits(excess(q)) != bits(excess(ref))) fail("excess(quotient) != excess(a / d)", a, d, q);
    // second site and the contract proper: the bits of a / d for +0 and for |a| >= 2^-500
    if (bits(a) == 0 || fabs(a) >= 0x1p-500) {
        ++n_exact;
        if (bits(q) != bits(ref)) fail("quotient != a / d", a, d, q);
    }
}

static void special_dividends(const ConstDiv& cd) {
    const double d = cd.d;
    for (int s = 0; s < 2; ++s) {
        check_div(cd, make(s, 0, 0));                                  // +-0
        check_div(cd, make(s, 2047, 0));                               // +-inf
        check_div(cd, make(s, 2047, 1));                               // NaNs
        check_div(cd, make(s, 2047, 0x8000000000000ull));
        check_div(cd, make(s, 0, 1));                                  // denormals: least, greatest, random
        check_div(cd, make(s, 0, kOnes));
        for (int i = 0; i < 200; ++i) check_div(cd, make(s, 0, rnd()));
        for (int e = 1; e < 2047; ++e) {                               // all-ones significands, powers of two
            check_div(cd, make(s, e, kOnes));
            check_div(cd, make(s, e, 0));
            check_div(cd, make(s, e, kOnes - 1));
        }
        // quotients at and next to the limit of excess(): a = +-d stepped by a few ulps, and the products nearest d * 1
        for (int k = -8; k <= 8; ++k) {
            const double a = from_bits(bits(fabs(d)) + (uint64_t)(int64_t)k);
            check_div(cd, s ? -a : a);
        }
        // the dividends of the second site next to its floor: 2 (v - 1) for the v just above 1
        for (int k = 1; k <= 8; ++k) check_div(cd, (s ? -2.0 : 2.0) * (from_bits(bits(1.0) + (uint64_t)k) - 1.0));
    }
}

static void divisions() {
    std::vector<double> fixed = {0.2, 0.1, 1.0 / 3.0, 0.05, 1.0, 0x1p400, 0x1p-400, 0x1p520, 0x1p-520, 1e-300, 1e-160, 1e8,
                                 make(0, 1023, kOnes), make(0, 1020, kOnes), make(0, 1023 - 499, kOnes), -0.2, 3.0};
    long in_range_random = 0, in_range_random_fallback = 0;
    auto run = [&](double d, long n_random) {
        const ConstDiv cd = vigo::make_const_div(d);
        const bool d_ok = vigo::exact_div_in_range(d);
        if (d_ok ? bits(cd.r) != bits(1.0 / d) || cd.lim != 0x1p500 || !(cd.lim2 > 0.0 && cd.lim2 <= cd.lim) : cd.r == cd.r || cd.lim != 0.0 || cd.lim2 != 0.0) fail("make_const_div", d, cd.r, cd.lim);
        special_dividends(cd);
        // exponents over the whole range, the field uniform: denormals, infinities and NaNs among them
        for (long i = 0; i < n_random / 4; ++i) check_div(cd, make(rnd() & 1, (int)(rnd() % 2048), rnd()));
        // the in-range dividends (the share that may take the fallback is capped on these)
        for (long i = 0; i < n_random - n_random / 4; ++i) {
            const long before = n_fallback;
            check_div(cd, rnd_exp(-500, 500));
            if (d_ok) { ++in_range_random; in_range_random_fallback += n_fallback - before; }
            else if (n_fallback == before) fail("a divisor out of range did not take the division", d, 0, 0);
        }
    };
    for (double d : fixed) run(d, 500000);
    for (int i = 0; i < 48; ++i) run(rnd_exp(-500, 500), 100000);
    for (int i = 0; i < 8; ++i) run(make(rnd() & 1, 1023 - 500 + (int)(rnd() % 1000), kOnes - (rnd() & 3)), 100000);
    printf("divisions %ld\n", n_div);
    printf("divisions_compared_bitwise %ld\n", n_exact);
    printf("divisions_fallback %ld\n", n_fallback);
    printf("division_chains %ld\n", n_chain);
    printf("in_range_random %ld\n", in_range_random);
    printf("in_range_random_fallback %ld\n", in_range_random_fallback);
}

// ---- the convergence filter ---------------------------------------------------------------------------------------------
static long n_conv = 0, n_decided_yes = 0, n_decided_no = 0;

// returns the filter's answer after holding it against the reference
static int check_conv(double G, double X, double eps) {
    const ConvFilter F = vigo::make_conv_filter(eps);
    const int f = vigo::conv_filter(G, X, F);
    const bool ref = vigo::conv_reference(G, X, eps);
    ++n_conv;
    if (f < -1 || f > 1) fail("conv_filter's value", G, X, eps);
    if (f >= 0 && (f != 0) != ref) fail("conv_filter decides against the reference", G, X, eps);
    if (vigo::conv_test(G, X, eps, F) != ref) fail("conv_test", G, X, eps);
    // what must never be decided by the filter
    const bool g_ok = G >= 0x1p-500 && G < 0x1p500, x_ok = X >= 0x1p-500 && X < 0x1p500;
    if (f >= 0 && !(g_ok && x_ok && eps >= 0.0)) fail("conv_filter decided outside its range", G, X, eps);
    if (f >= 0 && eps != 0.0 && !(eps >= 0x1p-500 && eps < 0x1p500)) fail("conv_filter decided on an eps out of range", G, X, eps);
    // g_epsilon = 0, the fixed-work mode: decided, "not converged", for every G and X in range
    if (eps == 0.0 && g_ok && x_ok && f != 0) fail("eps = 0 is not 'not converged'", G, X, eps);
    n_decided_yes += f == 1;
    n_decided_no += f == 0;
    return f;
}

static void filter() {
    const double nan = __builtin_nan("");
    // 1. random, everything the filter is meant to decide: the share it leaves to the reference is capped
    long n_random = 0, random_undecided = 0;
    for (long i = 0; i < 2000000; ++i) {           // exponents over the whole admitted range
        ++n_random;
        random_undecided += check_conv(fabs(rnd_exp(-500, 500)), fabs(rnd_exp(-500, 500)), fabs(rnd_exp(-250, 250))) < 0;
    }
    long near_yes = 0, near_no = 0;
    for (long i = 0; i < 2000000; ++i) {           // a solver's magnitudes, G within e^+-3 of the threshold
        const double X = 0.25 * exp(10.6 * rnd_unit()), eps = 1e-4 * exp(9.2 * rnd_unit());
        const double G = (X > 1.0 ? X : 1.0) * eps * eps * exp(6.0 * rnd_unit() - 3.0);
        const int f = check_conv(G, X, eps);
        ++n_random;
        random_undecided += f < 0;
        near_yes += f == 1;
        near_no += f == 0;
    }
    if (near_yes < 500000 || near_no < 500000) fail("the near-threshold family is one-sided", (double)near_yes, (double)near_no, 0);
    // 2. adversarial: G on the threshold and k ulps off it — around 0 (where only the reference may decide) and around
    // the edges of the guard band, 2^-40 relative = 4096 ulps or 2048 next to a power of two
    const double eps_list[] = {0.0, -0.0, -0.01, 0.01, 0.5, 1.0, 1e3, 1e-200, 1e200, 0x1p-250, 0x1p250, 0x1.fffffffffffffp249, 0x1p-251, nan};
    std::vector<double> xs = {1.0, 0.5, 2.0, 0.999, 1.001, 37.25, 1e4, 0x1p-500, 0x1p-501, 0x1.fffffffffffffp499, 0x1p500, 0.0, nan, INFINITY, -1.0};
    for (int k = -4; k <= 4; ++k) xs.push_back(from_bits(bits(1.0) + (uint64_t)(int64_t)k));   // X around 1
    for (int i = 0; i < 40; ++i) xs.push_back(0.25 * exp(10.6 * rnd_unit()));
    long band_undecided = 0, band_decided = 0;
    for (double eps : eps_list)
        for (double X : xs) {
            const double c = (X > 1.0 ? X : 1.0) * eps * eps;
            if (c == c && c > 0x1p-1000 && c < 0x1p1000) {
                auto at = [&](long k) {
                    const int f = check_conv(from_bits(bits(c) + (uint64_t)(int64_t)k), X, eps);
                    (f < 0 ? band_undecided : band_decided) += 1;
                };
                for (long k = -80; k <= 80; ++k) at(k);
                for (long k = 1900; k <= 2200; ++k) { at(k); at(-k); }
                for (long k = 3950; k <= 4250; ++k) { at(k); at(-k); }
                for (long k = 8000; k <= 8200; k += 7) { at(k); at(-k); }
            }
            const double gs[] = {0.0, -0.0, from_bits(1), from_bits(kOnes), 0x1p-1022, 0x1p-501, 0x1p-500, 0x1p500, 0x1.fffffffffffffp499,
                                 INFINITY, nan, -1.0, 1.0, c, 1e-30, 1e30};
            for (double G : gs) check_conv(G, X, eps);
        }
    if (band_undecided == 0 || band_decided == 0) fail("the band family is one-sided", (double)band_undecided, (double)band_decided, 0);
    printf("filter_cases %ld\n", n_conv);
    printf("filter_decided_converged %ld\n", n_decided_yes);
    printf("filter_decided_not_converged %ld\n", n_decided_no);
    printf("filter_random %ld\n", n_random);
    printf("filter_random_undecided %ld\n", random_undecided);
    printf("filter_band_undecided %ld\n", band_undecided);
    printf("filter_band_decided %ld\n", band_decided);
}

int main() {
    divisions();
    filter();
    printf("ok 1\n");
    return 0;
}
