"""-m gpu: k_optimize_fused (vigo_solver.hip), the ONE launch of a vigo_optimize call that used to be the axis-per-lane
launch followed by the general one: fp64 reference order, N <= 32, no obstacle list, no z planning, at most one
trajectory per SIMD.  Workgroup b classifies trajectory b once; a level one runs the axis body on the whole wave, any
other the general body alone on lanes 0 .. 31, with an LDS layout for one trajectory.

Everything is compared with `==` against the emulation-mode oracle (status, iterations, evaluations, x, control points,
fx), which knows nothing of launches or layouts.  A result must not depend on the trajectories it shares a batch with, nor
on its place in it: every trajectory of a mixed batch equals the same trajectory solved alone and in the reversed batch.
"""
import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import emulation, is_level, simd_count
from test_gpu_solver_axis import OUT, assert_equals_oracle, guided_batch, solve, take
from trajectory_planner_amd import synth
from trajectory_planner_amd.vigo import default_params

pytestmark = pytest.mark.gpu


def band_edge(z0):
    """(the last z that the level rule accepts beside z0, the first it refuses), z > z0"""
    lvl = lambda z: bool(is_level(np.array([[[0.0, 0.0, z0], [0.0, 0.0, z]]]))[0])
    z = z0 + 2.0 ** -40 * max(1.0, abs(z0))
    while lvl(z):
        z = np.nextafter(z, np.inf)
    while not lvl(np.nextafter(z, -np.inf)):
        z = np.nextafter(z, -np.inf)
    return np.nextafter(z, -np.inf), z


def jitter(b, which, seed):
    """vertical structure far beyond the level band on the trajectories `which`"""
    which = np.asarray(which, dtype=np.int64)
    b.ctrl[which, :, 2] += np.random.default_rng(seed).normal(0.0, 0.03, size=(len(which), b.N))
    return b


# composition -> the trajectories of a batch of B that are NOT level (None: the band-edge pair, built apart)
COMPOSITIONS = {
    "all_level": lambda B: [],
    "none_level": lambda B: list(range(B)),
    "alternating": lambda B: list(range(1, B, 2)),
    "alternating_from_0": lambda B: list(range(0, B, 2)),
    "only_first": lambda B: [0],
    "only_last": lambda B: [B - 1],
    "band_edge": None,
}


def composed(world, B, N, name, seed):
    """(batch, the level flags it must have).  band_edge: trajectory 0 has one free control point raised to the last z the
    level rule accepts, trajectory 1 (B >= 2) the same point at the first z it refuses; the rest stay level."""
    b = synth.make_bspline_batch(world, B, N, seed, start_range=3.0)
    assert is_level(b.ctrl).all()
    if name == "band_edge":
        want = np.ones(B, dtype=bool)
        for t in range(min(B, 2)):
            b.ctrl[t, :, 2] = b.ctrl[t, 0, 2]
            b.ctrl[t, N // 2, 2] = band_edge(b.ctrl[t, 0, 2])[t]
            want[t] = t == 0
    else:
        out = COMPOSITIONS[name](B)
        jitter(b, out, seed + 1)
        want = np.ones(B, dtype=bool)
        want[out] = False
    level = is_level(b.ctrl)
    assert np.array_equal(level, want), name
    return b, level


def assert_independent_of_the_batch(v, P, b, g, what):
    """every trajectory alone, and the batch in reversed order"""
    for i in range(b.B):
        gi = solve(v, P, take(b, [i]))
        for k in OUT:
            assert np.array_equal(gi[k][0], g[k][i], equal_nan=True), f"{what}, trajectory {i}: {k} depends on the batch it is solved in"
    gr = solve(v, P, take(b, np.arange(b.B)[::-1]))
    for k in OUT:
        assert np.array_equal(gr[k][::-1], g[k], equal_nan=True), f"{what}: {k} depends on the order of the batch"


@pytest.mark.parametrize("N", [7, 8, 13, 32])       # one free point; two; an odd count; all 32 lanes of a half in use
@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_compositions_match_the_oracle_and_the_solve_alone(vigo_handle, small_world, B, N):
    P = default_params()
    P.max_iterations = 50
    for name in COMPOSITIONS:
        b, level = composed(small_world, B, N, name, 9100 + 100 * N + 10 * B)
        mixed = name not in ("all_level", "none_level") and B >= 2
        if mixed:
            assert level.any() and (~level).any(), name      # both classes, by the rule on the input alone
        g, _ = assert_equals_oracle(vigo_handle, P, b, f"{B} x {N}, {name}")
        assert np.array_equal(g["ctrl"][level, :, 2], b.ctrl[level, :, 2])          # the level rule: z as it was loaded
        if mixed:
            assert_independent_of_the_batch(vigo_handle, P, b, g, f"{B} x {N}, {name}")


@pytest.mark.parametrize("max_iterations", [1, 50])
@pytest.mark.parametrize("mem_size", [1, 2, 3, 16])     # 1, 2: every pair in registers, no ring slot in LDS; 3: one slot
@pytest.mark.parametrize("N", [8, 32])
def test_history_lengths_match_the_oracle(vigo_handle, small_world, N, mem_size, max_iterations):
    b, level = composed(small_world, 3, N, "alternating", 9500 + N)
    assert level.any() and (~level).any()
    P = default_params()
    P.mem_size = mem_size
    P.max_iterations = max_iterations
    P.g_epsilon = 0.0                                   # never converged: the iteration cap or a line-search exit
    what = f"3 x {N}, mem_size {mem_size}, max_iterations {max_iterations}"
    g, _ = assert_equals_oracle(vigo_handle, P, b, what)
    assert (g["status"] != 0).all() and (g["iters"] >= 1).all()
    assert_independent_of_the_batch(vigo_handle, P, b, g, what)


@pytest.mark.parametrize("not_level", [(1,), (0, 2)], ids=["guides_on_2_level_1_not", "guides_on_1_level_2_not"])
@pytest.mark.parametrize("n_pairs", [0, 1, 3])          # none; one; one more than the two that sit in registers
def test_guide_pairs_match_the_oracle(vigo_handle, small_world, n_pairs, not_level):
    b = jitter(guided_batch(small_world, n_pairs, 1), not_level, 9600)
    level = is_level(b.ctrl)
    assert level.any() and (~level).any() and not level[list(not_level)].any()
    assert np.diff(b.guide_off).reshape(3, b.N).max(1).tolist() == [n_pairs] * 3       # pairs on both classes
    P = default_params()
    P.max_iterations = 50
    P.uncertain_factor = 1.7
    g, _ = assert_equals_oracle(vigo_handle, P, b, f"{n_pairs} guide pairs")
    assert_independent_of_the_batch(vigo_handle, P, b, g, f"{n_pairs} guide pairs")


def test_per_trajectory_weights_match_the_oracle(vigo_handle, small_world):
    b = jitter(synth.make_bspline_batch(small_world, 5, 20, 9700, start_range=3.0, guide2_prob=0.9), [1, 3], 9701)
    level = is_level(b.ctrl)
    assert level.tolist() == [True, False, True, False, True]
    w = np.random.default_rng(5).choice([0.5, 1.0, 2.0, 8.0], size=(b.B, 4))
    P = default_params()
    P.max_iterations = 50
    g, _ = assert_equals_oracle(vigo_handle, P, b, "per-trajectory weights", w)
    for i in range(b.B):
        gi = solve(vigo_handle, P, take(b, [i]), w[i:i + 1])
        for k in OUT:
            assert np.array_equal(gi[k][0], g[k][i]), f"trajectory {i}: {k} depends on the batch it is solved in"


def test_nan_coordinate_between_two_level_trajectories(vigo_handle, small_world):
    b = jitter(synth.make_bspline_batch(small_world, 3, 13, 9800, start_range=3.0), [1], 9801)
    b.ctrl[1, 6, 0] = np.nan
    assert is_level(b.ctrl).tolist() == [True, False, True]
    P = default_params()
    P.max_iterations = 50
    g, e = assert_equals_oracle(vigo_handle, P, b, "NaN x coordinate in the trajectory that is not level")
    assert np.isnan(e["fx"][1]) and e["status"][1] < 0 and (e["iters"][[0, 2]] > 0).all()
    assert np.isfinite(g["ctrl"][[0, 2]]).all()
    assert_independent_of_the_batch(vigo_handle, P, b, g, "NaN x coordinate")


@pytest.mark.parametrize("extra", [0, 1], ids=["one_trajectory_per_simd", "one_more"])
def test_the_last_fused_batch_and_the_first_that_is_not(vigo_handle, small_world, extra):
    """B = SIMD count: the largest batch of the fused launch; one more: two trajectories per wave, the D = 2 kernel and
    the general one.  The same answers either way."""
    B = simd_count() + extra
    b = jitter(synth.make_bspline_batch(small_world, B, 7, 9900, start_range=3.0), np.arange(1, B, 2), 9901)
    level = is_level(b.ctrl)
    assert np.array_equal(level, np.arange(B) % 2 == 0)
    P = default_params()
    P.max_iterations = 50
    g = solve(vigo_handle, P, b)
    with emulation(7):
        e = ol.optimize_batch(P, b)
    for k in OUT:
        assert np.array_equal(g[k], e[k], equal_nan=True), f"{B} x 7: {k} differs from the emulation-mode oracle"
    assert np.array_equal(g["ctrl"][level, :, 2], b.ctrl[level, :, 2])
