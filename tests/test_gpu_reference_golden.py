"""The HIP kernels against the numbers of the COMPILED reference (tests/golden/bspline_ref.npz: the verbatim
bspline.cpp / bsplineTraj.cpp over oracle/ref_shim, recorded by tests/golden/make_golden.py), not through the oracle.
Reads the fixture only: no reference source, no oracle/_ref library.  Bounds are the ones the existing tests hold
against the reference-order oracle: cost / terms 1e-13 relative and gradient 1e-12 of its largest entry
(test_gpu_solver.test_cost_grad_matches_oracle_all_terms), control points 1e-4 relative and equal statuses on >= 97 % at
50 iterations, the objective at 200 (test_optimize_matches_oracle), fp32 inside test_gpu_solver_dispatch.fp32_bound,
values / flags / indices of the spline and gate kernels exact, the fit at test_gpu_fit's 1e-10."""
import os

import numpy as np
import pytest
import torch

import bspline_ref_cases as brc
from gpu_util import batch_to_dev, rel_err_per_traj, to_dev
from test_gpu_solver_dispatch import fp32_bound
from test_prologue_restatement import collision_segments
from trajectory_planner_amd.vigo import PREC_F32, PREC_F64, PREC_F64_FAST

pytestmark = pytest.mark.gpu
FIX = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bspline_ref.npz")))
TOL, FIT_TOL = 1e-4, 1e-10


@pytest.mark.parametrize("mode", ["f64", "fast"])
def test_cost_grad_matches_the_reference(vigo_handle, mode):
    v = vigo_handle
    worst_c = worst_t = worst_g = 0.0
    v.set_precision(PREC_F64 if mode == "f64" else PREC_F64_FAST)
    try:
        for k, g in brc.groups(FIX, "cg"):
            v.set_params(brc.params(g["P"]))
            b = brc.batch_of(g)
            cost, grad, terms = (t.cpu().numpy() for t in v.cost_grad(**batch_to_dev(b, v.device, b.weights)))
            rc, rt, rg = FIX[f"cg{k}_cost"], FIX[f"cg{k}_terms"], FIX[f"cg{k}_grad"]
            ec = np.abs(cost - rc) / np.abs(rc)
            et = np.abs(terms - rt) / np.maximum(np.abs(rt), 1e-300)
            eg = np.abs(grad - rg).reshape(b.B, -1).max(1) / np.abs(rg).reshape(b.B, -1).max(1)
            print(f"\n[{mode} group {k} N={b.N} B={b.B}] vs compiled reference: cost {ec.max():.2e} terms {et.max():.2e} gradient {eg.max():.2e}")
            worst_c, worst_t, worst_g = max(worst_c, ec.max()), max(worst_t, et.max()), max(worst_g, eg.max())
            assert ec.max() <= 1e-13 and et.max() <= 1e-13, (k, ec.max(), et.max())
            assert eg.max() <= 1e-12, (k, eg.max())
    finally:
        v.set_precision(PREC_F64)
    print(f"\n[{mode}] worst over all groups: cost {worst_c:.2e} terms {worst_t:.2e} gradient {worst_g:.2e}")


def test_cost_grad_fp32_inside_the_derived_bound_of_the_reference(vigo_handle):
    v = vigo_handle
    for k, g in brc.groups(FIX, "cg"):
        P = brc.params(g["P"])
        b = brc.batch_of(g)
        # the parameters stay fp64 here (the fixture IS the reference at these values); the kernel rounds them to fp32,
        # a relative change of at most u in each — the same size as the input perturbation fp32_bound probes, which its
        # factor of 16 covers (observed: at most 0.1 of the bound)
        _, _, _, tb, gb = fp32_bound(P, b, b.weights)
        v.set_params(P)
        v.set_precision(PREC_F32)
        try:
            cost, grad, terms = (t.cpu().numpy() for t in v.cost_grad(**batch_to_dev(b, v.device, b.weights)))
        finally:
            v.set_precision(PREC_F64)
        et = np.abs(terms - FIX[f"cg{k}_terms"])
        eg = np.abs(grad - FIX[f"cg{k}_grad"]).reshape(b.B, -1).max(1)
        print(f"\n[f32 group {k} N={b.N}] error / bound: terms {(et / np.maximum(tb, 1e-300)).max():.3f} gradient {(eg / np.maximum(gb, 1e-300)).max():.3f}")
        assert (et <= tb).all(), (k, (et / np.maximum(tb, 1e-300)).max())
        assert (eg <= gb).all(), (k, (eg / np.maximum(gb, 1e-300)).max())
        assert (np.abs(cost - FIX[f"cg{k}_cost"]) <= (b.weights * tb).sum(1) * (1 + 1e-12)).all(), k


def test_optimize_matches_the_reference_solves(vigo_handle):
    v = vigo_handle
    rel50, same50, frel200, shapes = [], [], [], set()
    for k, g in brc.groups(FIX, "og"):
        P = brc.params(g["P"])
        P.max_iterations = iters = int(FIX[f"og{k}_iters"])
        v.set_params(P)
        b = brc.batch_of(g)
        r = v.optimize(**batch_to_dev(b, v.device, b.weights))
        ctrl, status, fx = r.ctrl.cpu().numpy(), r.status.cpu().numpy(), r.fx.cpu().numpy()
        level = (not P.plan_in_z) and bool((np.ptp(b.ctrl[:, :, 2], axis=1) == 0).all())
        if iters <= 50:
            rel = rel_err_per_traj(ctrl, FIX[f"og{k}_ctrl_out"])
            print(f"\n[group {k} N={b.N} level={level} it={iters}] control points vs compiled reference: max rel {rel.max():.2e}; "
                  f"status {status.tolist()} / {FIX[f'og{k}_status'].tolist()}")
            rel50 += rel.tolist()
            same50 += (status == FIX[f"og{k}_status"]).tolist()
            shapes.add((b.N, level))
        else:
            f = np.abs(fx - FIX[f"og{k}_fx"]) / np.abs(FIX[f"og{k}_fx"])
            print(f"\n[group {k} N={b.N} it={iters}] objective vs compiled reference: rel {f.tolist()}")
            frel200 += f.tolist()
    print(f"\n50 iterations: worst control-point error {max(rel50):.2e}, equal statuses {np.mean(same50) * 100:.1f} %; "
          f"200 iterations: objective median {np.median(frel200):.2e}")
    # both sides of every dispatch boundary, the level-rule instantiation and the general one
    assert shapes >= {(n, l) for n in (32, 33, 64, 65, 128, 129) for l in (True, False)}, shapes
    assert max(rel50) <= TOL, max(rel50)
    assert np.mean(same50) >= 0.97
    assert np.median(frel200) < 1e-3


def test_bspline_eval_equals_the_reference(vigo_handle):
    v = vigo_handle
    for N in brc.SPLINE_NS:
        c = to_dev(FIX[f"sp{N}_ctrl"][None], v.device)
        t = to_dev(FIX[f"sp{N}_t"], v.device)
        for dv in range(3):
            got = v.bspline_eval(c, t, deriv=dv).cpu().numpy()[0]
            assert np.array_equal(got, FIX[f"sp{N}_val"][:, dv]), (N, dv, np.abs(got - FIX[f"sp{N}_val"][:, dv]).max())


def test_gates_equal_the_reference(vigo_handle):
    v = vigo_handle
    v.set_grid(to_dev(FIX["world_vox"], v.device), FIX["world_origin"], float(FIX["world_res"]))
    dt = float(FIX["world_res"]) / brc.GATE_MAX_VEL / 2.0
    for N in brc.GATE_NS:
        cs, obs = FIX[f"gt{N}_ctrl"], FIX[f"gt{N}_obs"]
        B, n_obs = cs.shape[0], obs.shape[1]
        c = to_dev(cs, v.device)
        flag, first = (t.cpu().numpy() for t in v.traj_collision(c, dt))
        assert np.array_equal(flag, FIX[f"gt{N}_flag"]), N
        assert np.array_equal(first[flag != 0], FIX[f"gt{N}_first"][flag != 0]), N
        dyn = v.traj_dynamic_collision(c, dt, to_dev((np.arange(B + 1) * n_obs).astype(np.int32), v.device),
                                       to_dev(obs.reshape(B * n_obs, 9), v.device)).cpu().numpy()
        assert np.array_equal(dyn, FIX[f"gt{N}_dyn"]), N
        pt, line = (t.cpu().numpy() for t in v.ctrl_occupancy(c))
        want, pos = FIX[f"gt{N}_seg0"], 0
        for b in range(B):
            n = int(want[pos])
            got = collision_segments(N, lambda i: pt[b][i], lambda i: line[b][i])          # findCollisionSeg over the kernel's two flags
            assert [x for sg in got for x in sg] == want[pos + 1:pos + 1 + 2 * n].tolist(), (N, b)
            pos += 1 + 2 * n


def test_bspline_fit_matches_the_reference(vigo_handle):
    v = vigo_handle
    for K in (4, 9, 30):
        got = v.bspline_fit(to_dev(FIX[f"fit{K}_pts"], v.device), to_dev(FIX[f"fit{K}_cond"], v.device), ts=0.2).cpu().numpy()
        ref = FIX[f"fit{K}_ctrl"]
        err = rel_err_per_traj(got, ref)
        print(f"\n[fit K={K}] vs compiled reference: max rel {err.max():.2e}")
        assert err.max() <= FIT_TOL, (K, err.max())
