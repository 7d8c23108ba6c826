"""-m gpu: the axis-per-lane level kernel (vigo_solver.hip, D == 1) across the solver's parameter range.

That kernel reads the constants its iteration loop uses ONCE, at entry, into registers (HotConst) instead of at every
use site from DevConst in memory.  Every case here changes one of those constants to a value that decides a branch the
defaults do not take, on level batches the kernel takes (fp64 reference order, no obstacle list, B <= simd_count), and
compares control points, x, status, fx, iterations and evaluations with `==` against the emulation-mode oracle.  The
last test changes the parameters between two solves on one handle: the constants are read from the device copy at every
launch, never kept from an earlier one.
"""
import numpy as np
import pytest

import oracle_lib as ol
from gpu_util import emulation, is_level, simd_count
from test_gpu_solver_axis import OUT, assert_equals_oracle
from trajectory_planner_amd import synth
from trajectory_planner_amd.vigo import default_params

pytestmark = pytest.mark.gpu

LBERR_ROUNDING_ERROR, LBERR_MINIMUMSTEP, LBERR_MAXIMUMSTEP, LBERR_MAXIMUMLINESEARCH, LBERR_MAXIMUMITERATION = -1008, -1007, -1006, -1005, -1004
LBERR_WIDTHTOOSMALL = -1003
SHAPES = [(3, 8), (3, 32), (64, 8), (64, 32)]


def with_guides(b, n_pairs, unk):
    """b with its guide lists replaced: trajectory t carries n_pairs pairs on ONE free control point (3 + t mod (N - 6)),
    all known or all unknown.  In order: a pair whose plane passes through the control point (dist = 0, e == dthresh:
    the cubic branch wins), one in the no-penalty band (dist = 1.5 dthresh), one behind its guide point (dist < 0: the
    quadratic branch), one too far (dist = 2.5 dthresh: never scaled), one in the middle of the cubic band with its
    direction tilted out of the plane.  The kernel keeps the first two pairs of a point in registers and reads the rest
    from memory.  Distances are laid out for the DEFAULT dthresh; a case that changes it moves every pair's branch."""
    B, N = b.B, b.N
    dth = default_params().dthresh
    pv, off = [], [0]
    for t in range(B):
        for p in range(N):
            if p == 3 + t % (N - 6):
                c = b.ctrl[t, p]
                th = 0.7 + 1.1 * t
                u = np.array([np.cos(th), np.sin(th), 0.0])
                w = np.array([0.8 * np.cos(th + 0.4), 0.8 * np.sin(th + 0.4), 0.6])
                pairs = [np.concatenate([c, u]),
                         np.concatenate([c - 1.5 * dth * u, u]),
                         np.concatenate([c + 0.35 * u, u]),
                         np.concatenate([c - 2.5 * dth * u, u]),
                         np.concatenate([c - 0.5 * dth * w + [0, 0, 0.1], w])]
                pv += pairs[:n_pairs]
            off.append(len(pv))
    pv = np.array(pv, dtype=np.float64).reshape(-1, 6)
    return synth.Batch(b.ctrl, np.array(off, dtype=np.int32), pv, np.full(len(pv), unk, dtype=np.uint8))


def _set(**kw):
    def f(P):
        for k, v in kw.items():
            setattr(P, k, v)
    return f


def _double_dthresh(P):
    P.dthresh = 2.0 * P.dthresh


ALL = frozenset(SHAPES)
_WIDTH = dict(f_dec_coeff=0.3, s_curv_coeff=0.31)   # line searches that bracket: the only ones the width test can end


def V(change, guides=None, expect=None, expect_at=ALL, live=ALL, base=None):
    """One variant: `change` sets the parameters; `guides` = constructed guides (pairs per point, unknown) or None for
    the batch's own; at the shapes `expect_at` the oracle must report status `expect` for at least one trajectory; at the
    shapes `live` the oracle's result must DIFFER from its result with `base` (default: the default parameters) on the
    same batch — the changed constant decides something there, so a kernel that held a wrong value for it would fail
    the comparison.  Both sets come from oracle runs of these very batches; a new seed or world that empties one of
    them fails the case instead of leaving it vacuous."""
    return dict(change=change, guides=guides, expect=expect, expect_at=expect_at, live=live, base=base or _set())


VARIANTS = {
    "max_linesearch=1": V(_set(max_linesearch=1), expect=LBERR_MAXIMUMLINESEARCH),
    # (the loop header's test, max_linesearch <= count + 1, sends the second trial back to the best step: LB:837 wins)
    "max_linesearch=2": V(_set(max_linesearch=2), expect=LBERR_ROUNDING_ERROR),
    "max_iterations=1": V(_set(max_iterations=1), expect=LBERR_MAXIMUMITERATION),
    "max_iterations=3": V(_set(max_iterations=3), expect=LBERR_MAXIMUMITERATION),
    # crosses into the full-history two-loop; 3 x 8 converges before the 17th iteration
    "max_iterations=17": V(_set(max_iterations=17), live=ALL - {(3, 8)}),
    "g_epsilon=0": V(_set(g_epsilon=0.0), live=ALL - {(3, 32)}),           # never converged; 3 x 32 hits the cap either way
    "g_epsilon=1": V(_set(g_epsilon=1.0)),
    "g_epsilon=100": V(_set(g_epsilon=100.0), expect=0),                   # converged after an iteration or two
    "g_epsilon=1e300": V(_set(g_epsilon=1e300), expect=2),                 # LBFGS_ALREADY_MINIMIZED
    "max_step=0.5": V(_set(max_step=0.5), expect=LBERR_MAXIMUMSTEP),       # the clamp
    "min_step=1e-3": V(_set(min_step=1e-3), expect=LBERR_MINIMUMSTEP),
    # the width test needs a bracketed search, and with the default f_dec_coeff / s_curv_coeff these batches have
    # almost none: xtol = 0.1 alone changes nothing (kept: it must change nothing on the device either) ...
    "xtol=0.1": V(_set(xtol=0.1), live=frozenset()),
    # ... longer line searches (cmin), which end with LBFGSERR_WIDTHTOOSMALL at the default xtol already ...
    "ftol=0.3,gtol=0.31": V(_set(**_WIDTH), expect=LBERR_WIDTHTOOSMALL, expect_at=ALL - {(3, 8)}),
    # ... and among them the VALUE of xtol decides: a different trajectory than with the default xtol
    "xtol=0.5,ftol=0.3,gtol=0.31": V(_set(xtol=0.5, **_WIDTH), expect=LBERR_WIDTHTOOSMALL, expect_at=ALL - {(3, 8)},
                                     live=frozenset({(64, 8), (64, 32)}), base=_set(**_WIDTH)),
    "xtol=0.9,ftol=0.3,gtol=0.31": V(_set(xtol=0.9, **_WIDTH), expect=LBERR_WIDTHTOOSMALL, expect_at=ALL - {(3, 8)},
                                     live=ALL - {(3, 32)}, base=_set(**_WIDTH)),
    "dthresh*2,known": V(_double_dthresh, (2, 0)),
    "dthresh*2,unknown": V(_double_dthresh, (2, 1)),
    # (the factor scales unknown pairs only: with known pairs it must change nothing)
    "uncertain_factor=3,2pairs,known": V(_set(uncertain_factor=3.0), (2, 0), live=frozenset()),
    "uncertain_factor=3,2pairs,unknown": V(_set(uncertain_factor=3.0), (2, 1)),
    "uncertain_factor=3,5pairs,known": V(_set(uncertain_factor=3.0), (5, 0), live=frozenset()),
    "uncertain_factor=3,5pairs,unknown": V(_set(uncertain_factor=3.0), (5, 1)),
    "ts_ctrl=0.05": V(_set(ts_ctrl=0.05)),
    "ts_ctrl=0.3": V(_set(ts_ctrl=0.3)),
    "mem_size=1": V(_set(mem_size=1)),
    "mem_size=4": V(_set(mem_size=4)),
    "mem_size=16": V(_set(mem_size=16), live=frozenset()),                 # the default
}


def case(world, B, N, name):
    """the variant's parameters, its batch, and the parameters its result is held against where it is `live`"""
    v = VARIANTS[name]
    b = synth.make_bspline_batch(world, B, N, 8900 + 10 * N + B, start_range=3.0)
    if v["guides"] is not None:
        b = with_guides(b, *v["guides"])
    P, P0 = default_params(), default_params()
    P.max_iterations = P0.max_iterations = 50
    v["change"](P)
    v["base"](P0)
    return P, b, P0


def oracle_checks(name, B, N, e, e0):
    """what the oracle's own results must show for the case to mean something (no device result involved)"""
    v = VARIANTS[name]
    if v["expect"] is not None and (B, N) in v["expect_at"]:
        assert (e["status"] == v["expect"]).any(), f"{B} x {N}, {name}: no trajectory ends with status {v['expect']}"
    if (B, N) in v["live"]:
        assert not all(np.array_equal(e[k], e0[k], equal_nan=True) for k in OUT), \
            f"{B} x {N}, {name}: the oracle's result does not depend on what the variant changes"


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("B,N", SHAPES)
def test_parameter_variants_match_the_oracle(vigo_handle, small_world, B, N, name):
    P, b, P0 = case(small_world, B, N, name)
    assert is_level(b.ctrl).all() and b.obs is None and B <= simd_count()     # the axis-per-lane kernel takes it
    _, e = assert_equals_oracle(vigo_handle, P, b, f"{B} x {N}, {name}")
    with emulation(N):
        e0 = ol.optimize_batch(P0, b)
    oracle_checks(name, B, N, e, e0)


def test_set_params_between_two_solves_takes_effect(vigo_handle, small_world):
    b = synth.make_bspline_batch(small_world, 64, 32, 8990, start_range=3.0)
    assert is_level(b.ctrl).all()
    P = default_params()
    P.max_iterations = 50
    P.g_epsilon = 0.01
    g1, _ = assert_equals_oracle(vigo_handle, P, b, "first solve, g_epsilon = 0.01")
    P.g_epsilon = 100.0
    g2, _ = assert_equals_oracle(vigo_handle, P, b, "second solve, g_epsilon = 100")
    assert (g2["iters"] < g1["iters"]).all()                                  # the looser test ends every solve sooner
