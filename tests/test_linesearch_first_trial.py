"""-m "not gpu": csrc/vigo_linesearch.hpp on the CPU (tests/linesearch_first_trial_check.cpp, the host compiler at -O2
-ffp-contract=off): the first-trial form of a Moré–Thuente trip, which the axis-per-lane solve kernel takes on the first
trial of every line search, against the generic form from the same state.

Four million inputs: steps random, at `stpmin` / `stpmax`, one ulp beside them and outside them (the clamp lands on the
limit); `min_step` in {1e-20, 1e-3, 1.5, 0}, `max_step` in {1e20, 0.5, 1e-2, 3}; (ftol, gtol) the defaults and (0.3, 0.31);
`xtol` in {1e-16, 0.5, 0.9}; `max_linesearch` in {1, 2, 40}; trials near a quadratic along a descent direction, at the
decrease bound to the ulp and with dg == dgtest; one input in eight with zeros of both signs, infinities, NaNs (with
payloads), denormals and the largest doubles in fx, dg, finit, dginit.  The program exits 1 at the first input for which
a bit differs in: the begin's code, the step after the set-up, ftest1, the exit code, any field of the state handed to
the update and to the second trip, the second trip's exit code, step or state.

The floors below only say that every path was walked; they follow from the input mix (a quarter of the inputs have
max_linesearch = 1, a quarter of the steps sit on or are clamped to a limit), not from the code under test."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("linesearch") / "linesearch_first_trial_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(HERE, "linesearch_first_trial_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (line.split() for line in r.stdout.splitlines())}


def test_first_trial_form_has_the_bits_of_the_generic_trip(figures):
    assert figures["ok"] == 1
    assert figures["cases"] >= 4 * 10**6
    assert figures["special_values"] >= 2 * 10**5


def test_every_exit_and_the_hand_over_were_walked(figures):
    for exit_name in ("accepted", "max_linesearch", "minimum_step", "maximum_step", "begin_errors"):
        assert figures[exit_name] >= 10**5, exit_name
    assert figures["rejected"] >= 10**6                       # first trials handed over to the generic code
    assert figures["clamped_to_stpmin"] >= 10**5 and figures["clamped_to_stpmax"] >= 10**5
    assert figures["modified_function"] >= 10**4 and figures["bracketed"] >= 10**5
    assert figures["second_trip_exits"] >= 10**5 and figures["second_trip_goes_on"] >= 10**5
