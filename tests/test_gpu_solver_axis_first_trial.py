"""-m gpu: the axis-per-lane level kernel's line search (k_optimize, D == 1; csrc/vigo_linesearch.hpp), variant by variant
through the exits a FIRST trial can take and through the hand-over of a rejected first trial to the generic trips.

The kernel takes its Moré–Thuente search from csrc/vigo_linesearch.hpp with the set-up of a trial moved to the end of the
trial before it, so the first trial of every search runs text of its own; tests/test_linesearch_first_trial.py holds that
text to the generic trip on the CPU.  Here every comparison is `==` against the emulation-mode oracle on status,
iterations, evaluations, x, control points and fx.  Every batch is LEVEL, has at most 8 trajectories and N in
{7, 9, 16, 32} control points, so the dispatch takes the axis kernel.

`case(world, name, N)` builds a variant's parameters and batch and `oracle_says(name, N, e)` states, on the oracle's
results alone, what the variant is there for: its exit occurs, and at least one line search of the batch has its first
trial rejected and goes on (a solve whose evaluations outnumber 1 + iterations).  The second is not asked of the variants
whose first trial ends the solve by construction (max_linesearch = 1, a step limit the first step lies beyond,
equal control points) or whose clamp puts the first trial on the limit (min_step = 1e-3: the first step 1 / |g| of these
batches lies below it; min_step = 1e-4 is the variant whose exit fires on the trial AFTER a rejected first one).  Neither
needs a device: tests/test_solver_axis_first_trial_cases.py runs them on the CPU and holds the table VACUOUS below — the
(variant, N) pairs for which the oracle itself does not show both, at most one variant in ten of a shape — to them.
"""
import numpy as np
import pytest

import test_gpu_solver_axis_pair_sums as PS
import test_gpu_solver_axis_warmup as W
from gpu_util import is_level
from trajectory_planner_amd import synth

pytestmark = pytest.mark.gpu

LB_ALREADY_MINIMIZED = 2
LBERR_ROUNDING_ERROR, LBERR_MINIMUMSTEP, LBERR_MAXIMUMSTEP, LBERR_MAXIMUMLINESEARCH, LBERR_MAXIMUMITERATION = -1008, -1007, -1006, -1005, -1004
LBERR_WIDTHTOOSMALL = -1003
SIZES = [7, 9, 16, 32]
_BRACKETING = dict(f_dec_coeff=0.3, s_curv_coeff=0.31)   # profiles/README.md, round 5: the settings whose searches bracket


def noisy_batch(world, N, scale=1.0, seed=None):
    """eight level trajectories with noise on x and y: far enough from a minimum that first trials get rejected"""
    b = synth.make_bspline_batch(world, 8, N, seed or 9795 + N, start_range=3.0)
    ctrl = (b.ctrl + np.random.default_rng(11).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]) * scale
    return PS.no_guides(ctrl)


def _plain(**kw):
    return lambda world, N: (PS.params(**{"max_iterations": 50, "g_epsilon": 0.0, **kw}), noisy_batch(world, N))


def _guided(kind):
    return lambda world, N: (PS.params(max_iterations=50, g_epsilon=0.0, uncertain_factor=1.7), PS.guided_batch(world, N, *PS.GUIDES[kind]))


def _nan(world, N):
    nb = noisy_batch(world, N)
    ctrl = nb.ctrl.copy()
    ctrl[2, N // 2, 1] = np.nan
    return PS.params(max_iterations=17, g_epsilon=0.0), PS.no_guides(ctrl)


def _equal_points(world, N):
    ctrl = np.zeros((3, N, 3))
    ctrl[:, :, 0] = np.array([0.5, -1.25, 0.0])[:, None]
    ctrl[:, :, 1] = np.array([-0.75, 2.0, -0.0])[:, None]
    ctrl[:, :, 2] = 1.0
    return PS.params(max_iterations=50), PS.no_guides(ctrl)


# With one to three free points (N <= 9) most solves are at their minimum to the last bit before the 50th iteration and end in
# a search that cannot improve: the batches of these seeds hold a solve that reaches the cap (found with the oracle alone)
_CAP_SEED = {7: 9803, 9: 9810}

# name -> (builder, the status at least one solve must end with (None: see oracle_says), must a first trial be rejected?)
VARIANTS = {
    "max_linesearch=1": (_plain(max_linesearch=1), LBERR_MAXIMUMLINESEARCH, False),     # (the first rejection ends the solve)
    "max_linesearch=2": (_plain(max_linesearch=2), LBERR_ROUNDING_ERROR, True),
    "max_step=0.5": (_plain(max_step=0.5), LBERR_MAXIMUMSTEP, True),
    "max_step=1e-9": (_plain(max_step=1e-9), LBERR_MAXIMUMSTEP, False),                 # below the first step 1 / |g|
    "min_step=1e-3": (_plain(min_step=1e-3), LBERR_MINIMUMSTEP, False),                 # (the clamp puts the first trial there)
    "min_step=1e-4": (_plain(min_step=1e-4), LBERR_MINIMUMSTEP, True),                  # below 1 / |g|: the SECOND trial lands there
    "min_step=4": (_plain(min_step=4.0), LBERR_MINIMUMSTEP, False),                     # above every first step
    "xtol=0.5,bracketing": (_plain(xtol=0.5, **_BRACKETING), LBERR_WIDTHTOOSMALL, True),
    "xtol=0.9,bracketing": (_plain(xtol=0.9, **_BRACKETING), LBERR_WIDTHTOOSMALL, True),
    "max_iterations=1": (_plain(max_iterations=1), LBERR_MAXIMUMITERATION, True),
    "max_iterations=2": (_plain(max_iterations=2), LBERR_MAXIMUMITERATION, True),
    "max_iterations=17": (_plain(max_iterations=17), LBERR_MAXIMUMITERATION, True),
    "max_iterations=50": (lambda world, N: (PS.params(max_iterations=50, g_epsilon=0.0), noisy_batch(world, N, seed=_CAP_SEED.get(N))),
                          LBERR_MAXIMUMITERATION, True),
    "guides=none": (_guided("none"), None, True),
    "guides=one_pair": (_guided("one_pair"), None, True),
    "guides=one_more_than_the_registers": (_guided("one_more_than_the_registers"), None, True),
    "scale=1e-120": (lambda world, N: (PS.params(max_iterations=17, g_epsilon=0.0), noisy_batch(world, N, 1e-120)), None, True),
    "scale=1e120": (lambda world, N: (PS.params(max_iterations=17, g_epsilon=0.0), noisy_batch(world, N, 1e120)), None, True),
    "nan_coordinate": (_nan, None, True),
    "equal_points": (_equal_points, LB_ALREADY_MINIMIZED, False),                       # (no search at all)
}

# (variant, N) for which the oracle ITSELF does not show what oracle_says asks: the case still runs and is compared, the
# assertion on the oracle is the opposite one (so a new seed that fills the case in fails it, and the entry goes).  None.
VACUOUS = set()


def case(world, name, N):
    P, b = VARIANTS[name][0](world, N)
    assert is_level(b.ctrl).all() and b.B <= 8 and b.N == N
    return P, b


def rejected_first_trials(e):
    """per solve: evaluations beyond the start point's and one per iteration begun (`iters` counts the iteration whose
    search ended the solve too): each is a trial that followed a rejected one"""
    return e["evals"] - 1 - e["iters"]


def shows(name, N, e):
    """does the oracle's result show what the variant is there for?"""
    _, expect, goes_on = VARIANTS[name]
    if expect is not None:
        ok = bool((e["status"] == expect).any())
    elif name.startswith("guides="):
        ok = bool((e["iters"] >= 6).all())
    elif name.startswith("scale="):
        x2 = (e["x"][:, :, :2] ** 2).sum()
        ok = bool((x2 < 1e-200 or x2 > 1e200) and (e["iters"] >= 1).any())
    else:   # nan_coordinate
        ok = bool(np.isnan(e["fx"][2]) and e["status"][2] < 0 and (np.delete(e["iters"], 2) >= 6).any())
    if goes_on:
        ok = ok and bool((rejected_first_trials(e) > 0).any())
    return ok


def oracle_says(name, N, e):
    if (name, N) in VACUOUS:
        assert not shows(name, N, e), f"{name}, N = {N}: listed as vacuous, and the oracle shows the exit and a rejected first trial"
    else:
        assert shows(name, N, e), f"{name}, N = {N}: the oracle does not show the variant's exit and a rejected first trial that goes on"


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("N", SIZES)
def test_first_trial_variants_match_the_oracle(vigo_handle, small_world, N, name):
    P, b = case(small_world, name, N)
    _, e = W.assert_axis_equals_oracle(vigo_handle, P, b, f"{b.B} x {N}, {name}")
    oracle_says(name, N, e)
