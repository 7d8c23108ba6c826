"""-m gpu: the warm-up two-loops of the axis-per-lane level kernel (k_optimize, D == 1): the iterations whose history is
not yet full (k = 1 .. 15 with the default memory of 16).

They divide by ys with Markstein's sequence on the stored reciprocal, as the steady-state two-loop does, and share its
one fallback: a two-loop that saw a dividend outside 2^+-500, a reciprocal that is NaN or a NaN in d is repeated from
d = -g with true divisions.  The emulation-mode oracle always divides, so every comparison here is `==` on status,
iterations, evaluations, x, control points and fx.  Every batch is LEVEL and no larger than the device has SIMDs, so the
dispatch takes the axis kernel.
"""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from gpu_util import batch_to_dev, emulation, is_level, simd_count
from trajectory_planner_amd import synth
from trajectory_planner_amd.vigo import default_params

pytestmark = pytest.mark.gpu
OUT = ("status", "iters", "evals", "x", "ctrl", "fx")
NO_GUIDES = lambda B, N: (np.zeros(B * N + 1, dtype=np.int32), np.zeros((0, 6)), np.zeros(0, dtype=np.uint8))


def solve(v, P, b, weights=None):
    v.set_params(P)
    r = v.optimize(**batch_to_dev(b, v.device, weights))
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in OUT}


def oracle(P, b, weights=None):
    with emulation(b.N):
        return ol.optimize_batch(P, b, weights) if weights is not None else ol.optimize_batch(P, b)


def assert_axis_equals_oracle(v, P, b, what, weights=None):
    assert is_level(b.ctrl).all() and b.B <= simd_count(), f"{what}: not a batch for the axis kernel"
    g, e = solve(v, P, b, weights), oracle(P, b, weights)
    for k in OUT:
        assert np.array_equal(g[k], e[k], equal_nan=True), f"{what}: {k} differs from the emulation-mode oracle"
    return g, e


def depth_batch(world, N, guides):
    """six level trajectories; guides: the pairs synth gives the control points that start inside an obstacle"""
    b = synth.make_bspline_batch(world, 6, N, 9100 + N, start_range=3.0, guide2_prob=0.9)
    if guides:
        assert b.guide_off[-1] > 0, "no control point of this batch carries a guide pair"
        return b
    return synth.Batch(b.ctrl, *NO_GUIDES(b.B, b.N))


def concat(a, b):
    """two batches without obstacles as one: a's trajectories first"""
    return synth.Batch(np.concatenate([a.ctrl, b.ctrl]), np.concatenate([a.guide_off, b.guide_off[1:] + a.guide_off[-1]]).astype(np.int32),
                       np.concatenate([a.guide_pv, b.guide_pv]), np.concatenate([a.guide_unk, b.guide_unk]))


# ---- 1. every warm-up depth -------------------------------------------------------------------------------------------
# the solve ends inside each warm-up depth (two-loops of 1 .. 14 pairs), at the last warm-up iteration (15), at the first
# steady one (16) and just past it
@pytest.mark.parametrize("max_iterations", [1, 2, 3, 8, 15, 16, 17, 20])
@pytest.mark.parametrize("guides", [0, 1])
@pytest.mark.parametrize("N", [8, 20, 32])
def test_every_warmup_depth_matches_the_oracle(vigo_handle, small_world, N, guides, max_iterations):
    b = depth_batch(small_world, N, guides)
    P = default_params()
    P.max_iterations = max_iterations
    P.g_epsilon = 0.0
    _, e = assert_axis_equals_oracle(vigo_handle, P, b, f"6 x {N}, guides {guides}, {max_iterations} iterations")
    assert (e["iters"] == max_iterations).any(), "no solve of the batch got as far as the cap"


# ---- 2. warm-up fallback ----------------------------------------------------------------------------------------------
_scaled = {}


def scaled_batch(world, scale):
    """the batch of test_gpu_solver.py::test_two_loop_division_fallback_is_exact with the noise on x and y only (level):
    control points scaled by 1e-25 keep the dividends (~ scale^2) within 2^+-500, 1e-80 and 1e-120 put them far below"""
    if scale not in _scaled:
        b = synth.make_bspline_batch(world, 40, 32, 4711, start_range=3.0)
        ctrl = (b.ctrl + np.random.default_rng(3).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]) * scale
        _scaled[scale] = synth.Batch(ctrl, *NO_GUIDES(b.B, b.N))
    return _scaled[scale]


@pytest.mark.parametrize("max_iterations", [3, 8, 15])
@pytest.mark.parametrize("scale", [1e-25, 1e-80, 1e-120])
def test_warmup_division_fallback_is_exact(vigo_handle, small_world, scale, max_iterations):
    """only warm-up two-loops run: on Markstein's sequence at 1e-25, through the fallback at 1e-80 and 1e-120"""
    P = default_params()
    P.max_iterations = max_iterations
    P.g_epsilon = 0.0
    _, e = assert_axis_equals_oracle(vigo_handle, P, scaled_batch(small_world, scale), f"scale {scale}, {max_iterations} iterations")
    assert (e["iters"] == max_iterations).any(), "every solve of the batch stopped before the cap"
    assert (e["iters"] <= 15).all()


def test_steady_path_reports_into_the_shared_fallback(vigo_handle, small_world):
    """40 iterations at 1e-80: the steady-state two-loop sees the dividends below 2^-500 and hands over to the one
    true-division recursion the warm-up path uses"""
    P = default_params()
    P.max_iterations = 40
    P.g_epsilon = 0.0
    _, e = assert_axis_equals_oracle(vigo_handle, P, scaled_batch(small_world, 1e-80), "scale 1e-80, 40 iterations")
    assert (e["iters"] > 20).any(), "the history never filled up"


# ---- 3. non-finite coefficients in the warm-up --------------------------------------------------------------------------
def test_nan_coordinate_in_the_warmup(vigo_handle, small_world):
    b = synth.make_bspline_batch(small_world, 8, 20, 9300, start_range=3.0)
    ctrl = b.ctrl + np.random.default_rng(13).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]
    ctrl[5, 9, 0] = np.nan
    nb = synth.Batch(ctrl, *NO_GUIDES(b.B, b.N))
    P = default_params()
    P.max_iterations = 10
    P.g_epsilon = 0.0
    _, e = assert_axis_equals_oracle(vigo_handle, P, nb, "NaN x coordinate")
    assert (np.delete(e["iters"], 5) == 10).any(), "no solve beside the NaN one got as far as the cap"


@pytest.mark.parametrize("N,scale", [(8, 1e-154), (10, 1e-160)])
def test_zero_ys_in_the_warmup(vigo_handle, small_world, N, scale):
    """the construction of test_gpu_solver_axis.py::test_zero_ys_takes_the_non_finite_path, stopped after six iterations"""
    b = synth.make_bspline_batch(small_world, 6, N, 8800, start_range=3.0)
    ctrl = (b.ctrl + np.random.default_rng(9).normal(0, 0.05, size=b.ctrl.shape) * [1, 1, 0]) * scale
    nb = synth.Batch(ctrl, *NO_GUIDES(b.B, b.N))
    P = default_params()
    P.max_iterations = 6
    P.g_epsilon = 0.0
    _, e = assert_axis_equals_oracle(vigo_handle, P, nb, f"scale {scale}", np.full((6, 4), 1e5))
    assert (e["iters"] >= 5).any(), "every solve of the batch stopped at its first line search"


# ---- 4. same answer whatever the dispatch -------------------------------------------------------------------------------
def test_warmup_result_does_not_depend_on_the_dispatch(vigo_handle, small_world):
    """The six trajectories of case 1 at N = 32 on a wave each (the axis kernel), and at the head of a batch of more
    trajectories than the device has SIMDs (two per wave, the D = 2 instantiation, which divides for real)."""
    b = depth_batch(small_world, 32, 1)
    P = default_params()
    P.max_iterations = 12
    P.g_epsilon = 0.0
    g, _ = assert_axis_equals_oracle(vigo_handle, P, b, "6 x 32, 12 iterations")
    big = concat(b, synth.make_bspline_batch(small_world, simd_count() + 64 - b.B, 32, 9400, start_range=3.0))
    assert big.B > simd_count() and is_level(big.ctrl).all()
    gb = solve(vigo_handle, P, big)
    for k in OUT:
        assert np.array_equal(gb[k][:b.B], g[k], equal_nan=True), f"{k} depends on the size of the batch"
