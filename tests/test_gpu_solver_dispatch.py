"""-m gpu: every k_optimize / k_cost_grad instantiation the launchers of vigo_solver.hip can select, each checked
against the CPU oracle.

  A  dispatch matrix (fp64, fp64 fast): one case per launch path of plan_optimize (csrc/vigo_solver_plan.hpp) — shape,
     obstacle list or not, one or two waves per SIMD, the axis-per-lane (D = 1) launch, the level (D = 2) launch with
     and without the register-held history, the fast-mode redirect to the obstacle instantiation — solve and
     cost/gradient bit-exact against the emulation-mode oracle.  The restatement of the dispatch rule in
     solver_dispatch_rule.py, which test_solver_plan.py holds to the library's own plan, asserts that each case reaches
     the cell it is named for.
  B  the solve kernel's LDS obstacle table at prediction horizons that hold 0, 1, some, 16 obstacles, an odd
     prediction count and a count of 1, always with more obstacles than fit; a shared obstacle list at B > 1.
  C  fp32 cost/gradient against the fp64 reference-order oracle at the fp32-rounded inputs, under a bound the test
     derives per trajectory, and a check that the bound is far below what a dropped term would change.
  D  the first evaluation of a solve (status LBFGS_ALREADY_MINIMIZED) equals the standalone cost kernel bit for bit,
     in all three modes and at every cell of A and B: for fp32 the only exact check there is.
  E  the largest N vigo_optimize accepts per precision and mem_size, solved with obstacles; N + 1 refused.
"""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from gpu_util import batch_to_dev, emulation, is_level, simd_count
from solver_dispatch_rule import CELLS, LDS, WAVE, cell_batch_size, kernel_name, launches, lds_bytes, obs_table_fit, shape_for
from trajectory_planner_amd import synth
from trajectory_planner_amd.vigo import PREC_F32, PREC_F64, PREC_F64_FAST, VigoError, default_params

pytestmark = pytest.mark.gpu
MODES = {"f64": PREC_F64, "fast": PREC_F64_FAST, "f32": PREC_F32}
OUT = ("status", "iters", "evals", "x", "ctrl", "fx")
U32 = 2.0 ** -24                     # unit roundoff of fp32


# ---- A: the dispatch matrix (CELLS, solver_dispatch_rule.py) ------------------------------------------------------
def cell_params(modes):
    return [pytest.param(m, c, id=f"{m}-{c[0]}") for m in modes for c in CELLS if m in c[1].split()]


def cell_batch(world, cell, simds):
    name, _, N, _, mem, n_obs, flags, _ = cell
    B = cell_batch_size(cell, simds)
    # level and vertically jittered trajectories mixed, so that both launches of a level call have waves to solve
    b = synth.make_bspline_batch(world, B, N, 5000 + N + B + mem, start_range=3.0, n_obs=n_obs, z_jitter=0.02, z_share=0.3)
    P = default_params()
    P.max_iterations = 20
    P.mem_size = mem
    P.plan_in_z = 1 if "plan_in_z" in flags else 0
    P.strict_z = 1 if "strict_z" in flags else 0
    return b, P


def check_cell(mode, cell, b, P, simds):
    name, _, N, _, mem, n_obs, flags, want = cell
    got = launches(mode, N, b.B, mem, n_obs > 0, P.plan_in_z, P.strict_z, simds)
    assert got == want, f"{mode}-{name}: the launch rule now selects {[kernel_name(mode, N, *k) for k in got]}"
    level = is_level(b.ctrl)
    if any(k[2] == 1 for k in want):
        assert level.any() and not level.all(), "some trajectories level and some not"
    if any(k[2] == 2 for k in want):
        tpb = WAVE // shape_for(N)[0]
        wave_level = np.array([level[i:i + tpb].all() for i in range(0, b.B, tpb)])
        assert wave_level.any() and not wave_level.all(), "both launches of the level call must have waves to solve"


def solve(v, P, b, mode, weights=None):
    v.set_params(P)
    v.set_precision(MODES[mode])
    try:
        d = batch_to_dev(b, v.device, weights)
        cost, grad, terms = v.cost_grad(**d)
        r = v.optimize(**d)
        torch.cuda.synchronize()
    finally:
        v.set_precision(PREC_F64)
    return r, (cost.cpu().numpy(), grad.cpu().numpy(), terms.cpu().numpy())


def assert_matches_emulation(v, P, b, mode, what):
    r, (cost, grad, terms) = solve(v, P, b, mode)
    with emulation(b.N, fast=mode == "fast"):
        e = ol.optimize_batch(P, b)
        ce, ge, te = ol.cost_grad_batch(P, b)
    assert np.array_equal(cost, ce) and np.array_equal(grad, ge) and np.array_equal(terms, te), \
        f"{what}: cost/gradient differ from the emulation-mode oracle"
    for k in OUT:
        assert np.array_equal(getattr(r, k).cpu().numpy(), e[k]), f"{what}: {k} differs from the emulation-mode oracle"
    return r, terms


@pytest.mark.parametrize("mode,cell", cell_params(("f64", "fast")))
def test_dispatch_cell_matches_emulation(vigo_handle, small_world, mode, cell):
    simds = simd_count()
    b, P = cell_batch(small_world, cell, simds)
    check_cell(mode, cell, b, P, simds)
    r, terms = assert_matches_emulation(vigo_handle, P, b, mode, f"{mode}-{cell[0]}")
    if cell[5]:
        assert (terms[:, 3] > 0).mean() > 0.3, "too few trajectories meet an obstacle"


# ---- B: the LDS obstacle table -----------------------------------------------------------------------------------
# (case, N, pred_num, ts, obstacles per trajectory / in the shared list, shared list, obstacles the table holds)
TABLE = [
    ("32x1-fit0", 24, 200, 0.05, 3, False, 0),
    ("32x1-fit1", 24, 100, 0.1, 4, False, 1),
    ("32x1-partial", 24, 20, 0.1, 11, False, 8),
    ("32x1-cap16", 24, 8, 0.2, 19, False, 16),
    ("32x1-odd", 24, 21, 0.1, 11, False, 8),
    ("32x1-pred1", 24, 1, 0.1, 19, False, 16),
    ("64x1-fit0", 48, 70, 0.05, 3, False, 0),
    ("64x1-fit1", 48, 40, 0.1, 4, False, 1),
    ("64x1-partial", 48, 20, 0.1, 6, False, 3),
    ("64x1-cap16", 48, 2, 0.2, 19, False, 16),
    ("64x1-odd", 48, 11, 0.1, 8, False, 5),
    ("64x1-pred1", 48, 1, 0.1, 19, False, 16),
    ("64x4-odd", 150, 13, 0.1, 6, False, 4),
    ("32x1-shared", 24, 20, 0.1, 11, True, 8),
    ("64x2-shared", 100, 5, 0.1, 13, True, 11),
]


def table_params(modes):
    return [pytest.param(m, c, id=f"{m}-{c[0]}") for m in modes for c in TABLE]


def table_batch(world, case):
    name, N, pred_num, ts, n_obs, shared, fit = case
    assert obs_table_fit(N, pred_num) == fit and n_obs > fit, name
    B = 33
    b = synth.make_bspline_batch(world, B, N, 7000 + N + pred_num, start_range=3.0, n_obs=n_obs, z_jitter=0.02, z_share=0.3)
    if shared:   # one list for the whole batch (obs_off == NULL): obstacle j is the j-th one generated near path j
        b = synth.Batch(b.ctrl, b.guide_off, b.guide_pv, b.guide_unk, None,
                        np.ascontiguousarray(b.obs[[j * n_obs + j for j in range(n_obs)]]))
    P = default_params()
    P.max_iterations = 20
    P.ts = ts
    P.pred_horizon = (pred_num + 0.5) * ts
    assert int(P.pred_horizon / P.ts) == pred_num
    return b, P


@pytest.mark.parametrize("mode,case", table_params(("f64", "fast")))
def test_obstacle_table_matches_emulation(vigo_handle, small_world, mode, case):
    b, P = table_batch(small_world, case)
    r, terms = assert_matches_emulation(vigo_handle, P, b, mode, f"{mode}-{case[0]}")
    assert (terms[:, 3] > 0).mean() > 0.2, "too few trajectories meet an obstacle"


# ---- D: the first evaluation of a solve is the standalone cost kernel ------------------------------------------
def assert_first_evaluation_is_cost_kernel(v, P, b, mode, what):
    """g_epsilon so large that every solve stops at its first evaluation with LBFGS_ALREADY_MINIMIZED (k_optimize:
    `gnorm / xnorm <= g_epsilon` after trip 0): out_fx then holds f(x0), the control points are stored back as
    loaded.  Solve kernel (LDS obstacle table, D = 2 level build, two-wave build) vs k_cost_grad (all from HBM)."""
    P1 = type(P).from_buffer_copy(P)
    P1.g_epsilon = 1e300
    if mode == "f32":     # control points the fp32 state holds exactly, so "unchanged" is exact
        b = synth.Batch(b.ctrl.astype(np.float32).astype(np.float64), b.guide_off, b.guide_pv, b.guide_unk, b.obs_off, b.obs)
    r, (cost, _, _) = solve(v, P1, b, mode)
    assert (r.status.cpu().numpy() == 2).all(), f"{what}: not every solve stopped at its first evaluation"
    assert (r.iters.cpu().numpy() == 0).all() and (r.evals.cpu().numpy() == 1).all(), what
    fx = r.fx.cpu().numpy()
    bad = np.nonzero(fx != cost)[0]
    assert len(bad) == 0, (f"{what}: f(x0) of the solve differs from vigo_cost_grad on {len(bad)} trajectories, e.g. "
                           f"#{bad[0]}: {fx[bad[0]]!r} vs {cost[bad[0]]!r}")
    assert np.array_equal(r.ctrl.cpu().numpy(), b.ctrl), f"{what}: control points changed"


@pytest.mark.parametrize("mode,cell", cell_params(("f64", "fast", "f32")))
def test_first_evaluation_of_each_cell_is_the_cost_kernel(vigo_handle, small_world, mode, cell):
    simds = simd_count()
    b, P = cell_batch(small_world, cell, simds)
    check_cell(mode, cell, b, P, simds)
    assert_first_evaluation_is_cost_kernel(vigo_handle, P, b, mode, f"{mode}-{cell[0]}")


@pytest.mark.parametrize("mode,case", table_params(("f64", "fast", "f32")))
def test_first_evaluation_with_obstacle_table_is_the_cost_kernel(vigo_handle, small_world, mode, case):
    b, P = table_batch(small_world, case)
    assert_first_evaluation_is_cost_kernel(vigo_handle, P, b, mode, f"{mode}-{case[0]}")


# ---- C: fp32 against the fp64 reference-order oracle -------------------------------------------------------------
def f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32).astype(np.float64)


def fp32_problem(world, N, plan_in_z, B=48):
    """fp32-representable inputs: 20 obstacles per path (more than the table holds), 3 - 5 guide pairs on the points
    that have two, unknown-space guides with uncertain_factor != 1, per-trajectory weights; with plan_in_z, paths
    near either height limit so that the height term is active."""
    rng = np.random.default_rng(N + 1000 * plan_in_z)
    b = synth.make_bspline_batch(world, B, N, 600 + N, start_range=3.0, n_obs=20, guide2_prob=0.9, z_jitter=0.03, z_share=0.5)
    pv, unk, off = [], [], [0]
    for i, c in enumerate(np.diff(b.guide_off)):
        p, u = b.guide_pv[b.guide_off[i]:b.guide_off[i + 1]], b.guide_unk[b.guide_off[i]:b.guide_off[i + 1]]
        if c == 2:
            k = 1 + i % 3
            p = np.concatenate([p, p[[0, 1, 0][:k]] + rng.normal(0, 0.05, size=(k, 6)) * [1, 1, 1, 0, 0, 0]])
            u = np.concatenate([u, [1, 0, 1][:k]])
        pv.append(p)
        unk.append(u)
        off.append(off[-1] + len(p))
    ctrl, obs = b.ctrl.copy(), b.obs.copy()
    last = b.obs_off[1:] - 1                # the last obstacle of each path starts 0.3 m beside its middle point
    obs[last, :2] = ctrl[:, N // 2, :2] + 0.3
    obs[last, 3:5] = rng.uniform(-0.2, 0.2, size=(B, 2))
    if plan_in_z:
        ctrl[0::2, :, 2] -= 0.28            # z ~ 0.72: inside the band of min_height (0.7 + 0.2)
        ctrl[1::2, :, 2] += 0.26            # z ~ 1.26: inside the band of max_height (1.3 - 0.2)
    nb = synth.Batch(f32(ctrl), np.array(off, dtype=np.int32), f32(np.concatenate(pv)),
                     np.concatenate(unk).astype(np.uint8), b.obs_off, f32(obs))
    assert np.diff(nb.guide_off).max() >= 5 and np.diff(nb.obs_off).min() == 20
    P = default_params()
    P.plan_in_z = plan_in_z
    P.uncertain_factor, P.dthresh, P.dist_thresh_dynamic = 1.7, 0.6, 0.7
    P.pred_horizon = 2.05                   # pred_num 20 with the fp32 ts
    for f in ("dthresh", "dist_thresh_dynamic", "ts_ctrl", "ts", "uncertain_factor", "min_height", "max_height"):
        setattr(P, f, float(np.float32(getattr(P, f))))     # the parameters the kernel casts to fp32, as it sees them
    return nb, f32(rng.uniform(0.5, 4.0, size=(B, 4))), P


FP32_SAFETY = 16
FP32_PROBES = 4


def fp32_bound(P, b, w):
    """Per trajectory: a bound on |fp32 kernel - fp64 oracle| for each un-weighted term and for the weighted gradient.

    Every fp32 quantity of the kernel (stencil differences, guide distances, obstacle offsets, norms, penalties) is a
    short expression of inputs; evaluated in fp32 it equals the exact expression at inputs moved by a few units of
    fp32 roundoff u, and is then rounded once more.  The first part is measured: the largest change of the fp64
    oracle when every input (control points, guide pairs, obstacles) is scaled by (1 +- u) with random signs,
    over FP32_PROBES draws.  The second part: every term is a sum of non-negative per-point penalties, each rounded
    to fp32 before the fp64 sum, so it is at most u * term; for the gradient, u * sum_k |w_k grad term_k| (the four
    weighted parts are rounded before they are added).  The bound is FP32_SAFETY x (both parts): the factor covers the
    few roundings per quantity and a probe that misses the worst direction."""
    c0, g0, t0 = ol.cost_grad_batch(P, b, w)
    rng = np.random.default_rng(11)
    sgn = lambda a: 1.0 + U32 * rng.choice([-1.0, 1.0], size=a.shape)
    dt, dg = np.zeros_like(t0), np.zeros(b.B)
    for _ in range(FP32_PROBES):
        pb = synth.Batch(b.ctrl * sgn(b.ctrl), b.guide_off, b.guide_pv * sgn(b.guide_pv), b.guide_unk, b.obs_off,
                         None if b.obs is None else b.obs * sgn(b.obs))
        _, g, t = ol.cost_grad_batch(P, pb, w)
        dt = np.maximum(dt, np.abs(t - t0))
        dg = np.maximum(dg, np.abs(g - g0).reshape(b.B, -1).max(1))
    gsum = sum(np.abs(w[:, k, None, None] * ol.cost_grad_batch(P, b, np.eye(4)[[k] * b.B])[1]) for k in range(4))
    tb = FP32_SAFETY * (dt + U32 * np.abs(t0))
    gb = FP32_SAFETY * (dg + U32 * gsum.reshape(b.B, -1).max(1))
    return c0, g0, t0, tb, gb


def drop_one(b, what):
    """the batch with one guide pair per trajectory (the last pair of its point with the most) or its last obstacle
    removed"""
    B, N = b.B, b.N
    if what == "obstacle":
        keep = np.ones(len(b.obs), dtype=bool)
        keep[b.obs_off[1:] - 1] = False
        return synth.Batch(b.ctrl, b.guide_off, b.guide_pv, b.guide_unk, b.obs_off - np.arange(B + 1, dtype=np.int32),
                           np.ascontiguousarray(b.obs[keep]))
    cnt = np.diff(b.guide_off).reshape(B, N)
    keep = np.ones(len(b.guide_pv), dtype=bool)
    for i in range(B):
        if cnt[i].max() > 0:
            keep[b.guide_off[i * N + int(np.argmax(cnt[i])) + 1] - 1] = False
    kept = np.concatenate([[0], np.cumsum(keep)])
    return synth.Batch(b.ctrl, kept[b.guide_off].astype(np.int32), np.ascontiguousarray(b.guide_pv[keep]),
                       np.ascontiguousarray(b.guide_unk[keep]), b.obs_off, b.obs)


def assert_fp32_cost_grad(v, P, b, w, what):
    c0, g0, t0, tb, gb = fp32_bound(P, b, w)
    v.set_params(P)
    v.set_precision(PREC_F32)
    try:
        cost, grad, terms = v.cost_grad(**batch_to_dev(b, v.device, w))
        cost, grad, terms = cost.cpu().numpy(), grad.cpu().numpy(), terms.cpu().numpy()
    finally:
        v.set_precision(PREC_F64)
    et = np.abs(terms - t0)
    eg = np.abs(grad - g0).reshape(b.B, -1).max(1)
    print(f"\n[{what}] fp32 vs fp64 oracle, error / bound: terms max {(et / np.maximum(tb, 1e-300)).max(0).round(3)}, "
          f"gradient max {(eg / gb).max():.3f}; bound / term median {np.median(tb / np.maximum(t0, 1e-300), 0)}")
    for k, name in enumerate(("distance", "smoothness", "feasibility", "dynamic")):
        bad = np.nonzero(et[:, k] > tb[:, k])[0]
        assert len(bad) == 0, f"{what}: {name} term outside its bound on {len(bad)} trajectories, e.g. #{bad[0]}: " \
                              f"{terms[bad[0], k]!r} vs {t0[bad[0], k]!r} (bound {tb[bad[0], k]:.3e})"
    bad = np.nonzero(eg > gb)[0]
    assert len(bad) == 0, f"{what}: gradient outside its bound on {len(bad)} trajectories (worst {(eg / gb).max():.2f} x)"
    assert (np.abs(cost - c0) <= (w * tb).sum(1) * (1 + 1e-12)).all(), f"{what}: cost outside the bound"
    return t0, tb


def sensitivity_margins(P, b, w, t0, tb):
    """the oracle's change of the affected term when one guide pair / one obstacle / the height term is dropped,
    over the bound, for the trajectories where it changes (the height term is part of the distance term with
    plan_in_z; without it, the guide pairs' costs are the same)"""
    out = {}
    for what, k, P1, b1 in (("guide pair", 0, P, drop_one(b, "guide")), ("obstacle", 3, P, drop_one(b, "obstacle")),
                            ("height term", 0, None, b)):
        if P1 is None:
            if not P.plan_in_z:
                continue
            P1 = type(P).from_buffer_copy(P)
            P1.plan_in_z = 0
        _, _, t1 = ol.cost_grad_batch(P1, b1, w)
        ch = np.abs(t1[:, k] - t0[:, k])
        nz = ch > 0
        assert nz.sum() >= b.B // 4, f"dropping one {what} changes too few trajectories ({nz.sum()})"
        out[what] = (ch[nz] / tb[nz, k]).min()
    return out


@pytest.mark.parametrize("plan_in_z", [0, 1])
@pytest.mark.parametrize("N", [7, 20, 32, 33, 64, 65, 128, 129, 200, 256])
def test_fp32_cost_grad_within_derived_bound(vigo_handle, small_world, N, plan_in_z):
    b, w, P = fp32_problem(small_world, N, plan_in_z)
    t0, tb = assert_fp32_cost_grad(vigo_handle, P, b, w, f"fp32 N={N} plan_in_z={plan_in_z}")
    margins = sensitivity_margins(P, b, w, t0, tb)
    print(f"    smallest change / bound when one is dropped: {({k: f'{m:.3g}' for k, m in margins.items()})}")
    for what, m in margins.items():
        assert m >= 10, f"dropping one {what} changes the oracle by only {m:.2f} x the fp32 bound"


# ---- E: the largest N per precision and history length ---------------------------------------------------------
@pytest.mark.parametrize("mem", [16, 8, 1])
@pytest.mark.parametrize("mode", ["f64", "fast", "f32"])
def test_largest_accepted_n_solves(vigo_handle, small_world, mode, mem):
    v = vigo_handle
    P = default_params()
    P.max_iterations = 20
    P.mem_size = mem
    v.set_params(P)
    v.set_precision(MODES[mode])
    try:
        def accepted(N, B=0):
            try:
                v.optimize(torch.zeros(B, N, 3, dtype=torch.float64, device=v.device))
                return True
            except VigoError as e:
                assert "failed (-4)" in str(e), str(e)      # VIGO_ERR_UNSUPPORTED_N, refused on the host
                return False
        ok = [N for N in range(7, 258) if accepted(N)]
        nmax = ok[-1]
        assert ok == list(range(7, nmax + 1)) and nmax <= 256
        assert nmax == max(N for N in range(7, 257) if lds_bytes(mode, N, mem) <= LDS), "the ABI's limit moved"
        if mode != "f32" and mem == 16:
            assert nmax == 216          # include/vigo.h
        assert not accepted(nmax + 1, B=2)
    finally:
        v.set_precision(PREC_F64)
    b = synth.make_bspline_batch(small_world, 3, nmax, 9000 + nmax + mem, start_range=3.0, n_obs=18)
    what = f"{mode} N={nmax} mem_size={mem}"
    assert_first_evaluation_is_cost_kernel(v, P, b, mode, what)
    if mode != "f32":
        assert_matches_emulation(v, P, b, mode, what)
        return
    # fp32: cost/gradient under the derived bound, and the solve against the fp64 reference-order oracle
    bb, w, P32 = fp32_problem(small_world, nmax, 0, B=3)
    P32.mem_size, P32.max_iterations = mem, 20
    assert_fp32_cost_grad(v, P32, bb, w, what)
    r, (c0, _, _) = solve(v, P32, bb, mode, w)
    ref = ol.optimize_batch(P32, bb, w)
    got = r.ctrl.cpu().numpy()
    rel = np.abs(got - ref["ctrl"]).reshape(3, -1).max(1) / np.abs(ref["ctrl"]).reshape(3, -1).max(1)
    print(f"\n[{what}] fp32 end point vs fp64 oracle: max rel {rel.max():.2e}")
    assert np.isfinite(got).all() and (r.fx.cpu().numpy() <= c0).all() and np.median(rel) < 5e-2
