"""-m gpu: the paired reductions of the axis-per-lane level kernel (k_optimize, D == 1; csrc/vigo_solver.hip: pair_tree32,
pack_xy, ys_yy_axis).

The evaluation reduces its six sums as three pairs — [distance cost | x . x], [smoothness | feasibility], [g . d | g . g] —
and the update reduces ys and yy as one: the lower half of the wave carries one sum of a pair through the 32-lane tree,
the upper half the other, where both halves used to run the same tree on the same operands.  Each half runs the tree it
ran before on the operands it had before, so nothing may change: every comparison is `==` against the emulation-mode
oracle on status, iterations, evaluations, x, control points and fx.  tests/test_axis_pair_tree.py holds the tree itself
against a 64-lane model on the CPU.

Every batch is LEVEL, has at most 8 trajectories and is no larger than the device has SIMDs, so the dispatch takes the
axis kernel.  The `*_case` functions build the inputs and assert, on the inputs and on the oracle's results alone, that a
case is about what its name says; they need no device.
"""
import numpy as np
import pytest

import test_gpu_solver_axis_warmup as W
from gpu_util import is_level
from trajectory_planner_amd import synth
from trajectory_planner_amd.vigo import default_params

pytestmark = pytest.mark.gpu
LB_ALREADY_MINIMIZED = 2
K_GUIDE_REGS = 2          # LaneProblem<T, 1>::kGuideRegs: the pairs of a point held in registers
# one free point; rows (16 lanes) and halves (32) part full and full
SIZES = [7, 8, 9, 16, 17, 31, 32]
# the first trip; the first update (ys, yy); the warm-up two-loops and the first steady one; the steady state
CAPS = [1, 2, 17, 50]
# pairs on ONE control point of each trajectory, unknown flag
GUIDES = {"none": (0, 0), "one_pair": (1, 0), "one_more_than_the_registers": (K_GUIDE_REGS + 1, 0), "unknown_flags": (K_GUIDE_REGS + 1, 1)}


def params(**kw):
    P = default_params()
    for k, v in kw.items():
        setattr(P, k, v)
    return P


def no_guides(ctrl):
    return synth.Batch(ctrl, *W.NO_GUIDES(ctrl.shape[0], ctrl.shape[1]))


def guided_batch(world, N, n_pairs, unk):
    """four level trajectories of N control points; trajectory t carries n_pairs guide pairs on one free control point.
    In order (tests/test_gpu_solver_axis.py::guided_batch): a pair whose plane passes through the point (the cubic branch
    at its edge), one behind its guide point (the quadratic branch), one in the middle of the cubic band with its
    direction tilted out of the plane.  The first two sit in registers, the third is read from memory."""
    b = synth.make_bspline_batch(world, 4, N, 9500 + N, start_range=3.0)
    dth = default_params().dthresh
    pv, off = [], [0]
    for t in range(b.B):
        for p in range(N):
            if n_pairs and p == 3 + (2 * t) % (N - 6):
                c = b.ctrl[t, p]
                th = 0.7 + 1.1 * t
                u = np.array([np.cos(th), np.sin(th), 0.0])
                w = np.array([0.8 * np.cos(th + 0.4), 0.8 * np.sin(th + 0.4), 0.6])
                pairs = [np.concatenate([c, u]), np.concatenate([c + 0.35 * u, u]), np.concatenate([c - 0.5 * dth * w + [0, 0, 0.1], w])]
                pv += pairs[:n_pairs]
            off.append(len(pv))
    pv = np.array(pv, dtype=np.float64).reshape(-1, 6)
    return synth.Batch(b.ctrl, np.array(off, dtype=np.int32), pv, np.full(len(pv), unk, dtype=np.uint8))


_first_cost = {}


def first_cost(world, N, kind):
    """fx of the oracle's first evaluation (g_epsilon so large that the solve stops there)"""
    if (N, kind) not in _first_cost:
        e = W.oracle(params(g_epsilon=1e300, uncertain_factor=1.7), guided_batch(world, N, *GUIDES[kind]))
        assert (e["evals"] == 1).all()
        _first_cost[(N, kind)] = e["fx"]
    return _first_cost[(N, kind)]


def shape_case(world, N, kind, cap):
    n_pairs, unk = GUIDES[kind]
    b = guided_batch(world, N, n_pairs, unk)
    assert is_level(b.ctrl).all() and b.B <= 8 and np.diff(b.guide_off).max() == n_pairs
    # each kind of guides is felt by the cost: every pair added adds to it, and the unknown flag scales it
    if kind == "one_pair":
        assert (first_cost(world, N, kind) > first_cost(world, N, "none")).all()
    if kind == "one_more_than_the_registers":
        assert (first_cost(world, N, kind) > first_cost(world, N, "one_pair")).all()
    if kind == "unknown_flags":
        assert (first_cost(world, N, kind) > first_cost(world, N, "one_more_than_the_registers")).all()
    return params(max_iterations=cap, g_epsilon=0.0, uncertain_factor=1.7), b


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("kind", list(GUIDES))
@pytest.mark.parametrize("N", SIZES)
def test_sizes_guides_and_depths_match_the_oracle(vigo_handle, small_world, N, kind, cap):
    P, b = shape_case(small_world, N, kind, cap)
    _, e = W.assert_axis_equals_oracle(vigo_handle, P, b, f"4 x {N}, guides {kind}, {cap} iterations")
    # One to three free points (N <= 9) are at their minimum to the last bit well before 17 or 50 iterations, and the solve
    # ends there with a line search that cannot improve: those cases are about the update and the two-loop of a wave that is
    # nearly empty, and every solve of theirs must have run at least six iterations of it.
    at_cap = (e["iters"] == cap).any()
    at_minimum = N <= 9 and (e["status"] < 0).all() and (e["iters"] >= 6).all()
    assert at_cap or at_minimum, "no solve of the batch got as far as the cap"


def scaled_case(world, N, scale):
    """eight trajectories with noise on x and y, scaled: the costs go with the square of the scale and above, g . d and
    g . g with its square, x . x with its square while ys and yy follow the steps taken — the two sums of a pair lie
    far apart and a sum that came out of the wrong half could not hide in rounding"""
    b = synth.make_bspline_batch(world, 8, N, 9600 + N, start_range=3.0)
    ctrl = (b.ctrl + np.random.default_rng(7).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]) * scale
    nb = no_guides(ctrl)
    assert is_level(nb.ctrl).all()
    return nb


@pytest.mark.parametrize("cap", [2, 17])
@pytest.mark.parametrize("N", [9, 32])
@pytest.mark.parametrize("scale", [1e-120, 1e120])
def test_scaled_batches_match_the_oracle(vigo_handle, small_world, scale, N, cap):
    b = scaled_case(small_world, N, scale)
    _, e = W.assert_axis_equals_oracle(vigo_handle, params(max_iterations=cap, g_epsilon=0.0), b, f"8 x {N}, scale {scale}, {cap} iterations")
    assert (e["iters"] >= 1).any(), "every solve of the batch stopped in its first line search"
    x2 = (e["x"][:, :, :2] ** 2).sum()
    assert (x2 < 1e-200 or x2 > 1e200) and not (np.isfinite(e["fx"]) & (e["fx"] > 1e-150) & (e["fx"] < 1e150)).any()


def nan_case(world):
    b = synth.make_bspline_batch(world, 6, 17, 9700, start_range=3.0)
    ctrl = b.ctrl + np.random.default_rng(17).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]
    ctrl[2, 8, 1] = np.nan
    return params(max_iterations=17, g_epsilon=0.0), no_guides(ctrl)


def test_nan_coordinate_matches_the_oracle(vigo_handle, small_world):
    P, b = nan_case(small_world)
    _, e = W.assert_axis_equals_oracle(vigo_handle, P, b, "NaN y coordinate")
    assert np.isnan(e["fx"][2]) and e["status"][2] < 0
    assert (np.delete(e["iters"], 2) == 17).any(), "no solve beside the NaN one got as far as the cap"


def equal_points_case():
    """all control points of a trajectory in one place: every stencil term and the gradient are exact zeros (a partial of
    +-0 in every lane of both halves), and the first convergence test ends the solve"""
    ctrl = np.zeros((3, 16, 3))
    ctrl[:, :, 0] = np.array([0.5, -1.25, 0.0])[:, None]
    ctrl[:, :, 1] = np.array([-0.75, 2.0, -0.0])[:, None]
    ctrl[:, :, 2] = 1.0
    return params(max_iterations=50), no_guides(ctrl)


def test_equal_control_points_are_already_minimized(vigo_handle):
    P, b = equal_points_case()
    g, e = W.assert_axis_equals_oracle(vigo_handle, P, b, "equal control points")
    assert (e["status"] == LB_ALREADY_MINIMIZED).all() and (e["iters"] == 0).all() and (e["evals"] == 1).all() and (e["fx"] == 0.0).all()
    assert np.array_equal(g["ctrl"], b.ctrl)


@pytest.mark.parametrize("N,scale", [(8, 1e-154), (10, 1e-160)])
def test_zero_ys_matches_the_oracle(vigo_handle, small_world, N, scale):
    """the construction of tests/test_gpu_solver_axis.py::test_zero_ys_takes_the_non_finite_path: the products of ys
    underflow to zero while yy's do not have to, and the two-loop coefficients leave the finite range"""
    b = synth.make_bspline_batch(small_world, 6, N, 8800, start_range=3.0)
    nb = no_guides((b.ctrl + np.random.default_rng(9).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]) * scale)
    _, e = W.assert_axis_equals_oracle(vigo_handle, params(max_iterations=60, g_epsilon=0.0), nb, f"scale {scale}", np.full((6, 4), 1e5))
    poisoned = ~np.isfinite(e["ctrl"]).all(1).all(1)
    assert poisoned.any() and (e["iters"][poisoned] >= 2).all(), "no two-loop coefficient left the finite range"
