"""-m "not gpu": csrc/vigo_exact_div.hpp on the CPU (tests/exact_div_check.cpp, the host compiler at -O2
-ffp-contract=off): the text the axis-per-lane solve kernel uses for its divisions by ts_ctrl and in front of its
convergence test, against the operations it stands in for.

Division: for each divisor (0.2, 0.1, 1/3, 0.05, 1, 2^+-400, 2^+-520, 1e-300, 1e-160, 1e8, all-ones significands, a
negative one, 56 random ones) the dividends are random with the exponent field uniform over all 2048 values, random with
exponents in [-500, 500), every exponent with an all-ones significand, +-0, denormals, +-inf, NaNs, the divisor itself
stepped by a few ulps (quotients at the limit of the stencil's excess()) and the smallest dividends of the second site.
The program exits 1 at the first dividend for which `usable` is not exactly "divisor in range and |a| < 2^500", for
which excess(quotient) differs in a bit from excess(a / d) (every usable dividend: the first site's contract), or for
which the quotient differs in a bit from a / d (+0 and |a| >= 2^-500: the contract proper, the second site's), or for
which `usable2` holds and the second dividend of the stencil's chain, 2 excess(quotient), is not usable or its quotient
differs in a bit from (2 excess(a / d)) / d.

Filter: the program exits 1 at the first (G, X, eps) for which conv_filter decides and the reference expression says
otherwise, or decides where it must not (G, X outside [2^-500, 2^500), a negative, NaN or out-of-range eps), or does
not say "not converged" for eps = 0 with G and X in range.

The caps below are on what the REFERENCE alone fixes, not measurements of the helper: a dividend drawn with its exponent
in [-500, 500) is below 2^500 by construction, so NONE may take the division when the divisor is in range; a random
(G, X, eps) lies inside the guard band of 2^-40 relative with a probability of about 2^-39 per unit of log-width of the
family (e^+-3 around the threshold for the narrow one: 3e-13 per case), so one case in 10^5 is a generous ceiling that a
filter which never decides misses by five orders of magnitude."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exact_div") / "exact_div_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(HERE, "exact_div_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}


def test_division_by_a_constant_has_the_bits_of_the_division(figures):
    assert figures["ok"] == 1
    assert figures["divisions"] >= 10**7
    assert figures["divisions_compared_bitwise"] >= 6 * 10**6
    assert figures["divisions_fallback"] > 10**5              # NaN, inf, 2^500 and above, divisors out of range: all ran
    assert figures["division_chains"] >= 5 * 10**6             # usable2: the second dividend made of the first quotient
    assert figures["in_range_random"] >= 5 * 10**6
    assert figures["in_range_random_fallback"] == 0           # the cap: see the module's docstring


def test_convergence_filter_decides_as_the_reference_or_not_at_all(figures):
    assert figures["ok"] == 1
    assert figures["filter_random"] >= 4 * 10**6
    assert figures["filter_random_undecided"] * 10**5 <= figures["filter_random"]     # the cap: see the module's docstring
    assert figures["filter_decided_converged"] > 10**6 and figures["filter_decided_not_converged"] > 10**6
    assert figures["filter_band_undecided"] > 0 and figures["filter_band_decided"] > 0
