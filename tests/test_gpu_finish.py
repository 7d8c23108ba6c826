"""-m gpu: vigo_traj_finish (csrc/vigo_finish.hip) on every case of tests/finish_cases.py against the host twin and the
literal restatement of the rule — factor, maxima, counts, positions, velocities and statuses BIT FOR BIT, the sentinel
rows of INVALID_N and the tail beyond out_n included; a trajectory alone against the same trajectory inside the mixed
batch; the clock-table slots of the handle next to the gates' one; the whole-call refusals.  Small shapes only."""
import ctypes as C

import numpy as np
import pytest
import torch

import finish_cases as fc
import gate_cases as gc
from gpu_util import to_dev
from test_finish_core import assert_same, run_host, u64
from trajectory_planner_amd.vigo import VigoError, default_params

pytestmark = pytest.mark.gpu

CASES = fc.cases()


def _params(ts_ctrl, ts):
    P = default_params()
    P.ts_ctrl, P.ts = ts_ctrl, ts
    P.pred_horizon = max(P.pred_horizon, ts)       # vigo_set_params wants pred_horizon / ts in [1, 1e5]; the stage does not read it
    return P


def run_device(v, case, S_cap, ctrl=None, n_pts="case", limits=None):
    d = v.device
    ctrl = case.ctrl if ctrl is None else ctrl
    n_pts = case.n_pts if isinstance(n_pts, str) else n_pts
    limits = case.limits if limits is None else limits
    B = ctrl.shape[0]
    out = (torch.full((B, S_cap, 3), fc.SENTINEL, dtype=torch.float64, device=d), torch.full((B, S_cap, 3), fc.SENTINEL, dtype=torch.float64, device=d))
    r = v.traj_finish(to_dev(ctrl, d), to_dev(limits, d), case.dt, S_cap, n_pts=to_dev(n_pts, d), out=out)
    torch.cuda.synchronize()
    return {k: (None if t is None else t.cpu().numpy()) for k, t in r.items()}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_kernel_equals_host_twin_and_restatement(vigo_handle, case):
    v = vigo_handle
    v.set_params(_params(case.ts_ctrl, case.ts))
    e = fc.expected(case)
    got = run_device(v, case, e["S_cap"])
    assert_same(case, got, e, "kernel against the restatement")
    assert_same(case, got, run_host(case, e), "kernel against the host twin")


def test_alone_equals_inside_the_mixed_batch(vigo_handle):
    v = vigo_handle
    case = fc.by_name("count:mixed_in_64")
    v.set_params(_params(case.ts_ctrl, case.ts))
    e = fc.expected(case)
    S = e["S_cap"]
    batch = run_device(v, case, S)
    for b in range(case.B):
        row = case.row(b)[None]                                   # B = 1, Ns = n
        alone = run_device(v, case, S, ctrl=row, n_pts=None, limits=case.limits[b:b + 1])
        for k in ("factor", "max", "pos", "vel"):
            assert np.array_equal(u64(alone[k][0]), u64(batch[k][b])), (b, k)
        assert alone["n"][0] == batch["n"][b] and alone["status"][0] == batch["status"][b] == fc.OK


def test_clock_slots_live_next_to_the_gates_table(vigo_handle):
    """two calls with different sample_dt on one handle, a gate call between them: every result is what a fresh call gives"""
    v = vigo_handle
    g = gc.first_hit_cases()[0]
    case = fc.by_name("batch:3")
    assert g.ts_ctrl == case.ts_ctrl
    v.set_params(_params(case.ts_ctrl, case.ts))
    v.set_grid(to_dev(g.world.voxels, v.device), g.world.origin, g.world.res)
    gate = lambda: tuple(t.cpu().numpy() for t in v.traj_collision(to_dev(g.ctrl, v.device), g.dt))
    flag0, first0 = gate()
    ref_flag, ref_first = gc.oracle_static(g)
    assert np.array_equal(flag0, ref_flag) and np.array_equal(first0, ref_first)
    e = fc.expected(case)
    first_call = run_device(v, case, e["S_cap"])
    assert_same(case, first_call, e, "first call")
    flag1, first1 = gate()
    assert np.array_equal(flag1, flag0) and np.array_equal(first1, first0)
    other = fc.FinishCase("slots:other_dt", case.ts_ctrl, case.ts, 0.037, case.ctrl, case.limits, case.n_pts)
    e2 = fc.expected(other)
    assert_same(other, run_device(v, other, e2["S_cap"]), e2, "second call, another sample_dt")
    flag2, first2 = gate()
    assert np.array_equal(flag2, flag0) and np.array_equal(first2, first0)
    assert_same(case, run_device(v, case, e["S_cap"]), e, "third call, the first sample_dt again")


def test_optional_outputs_and_empty_batch(vigo_handle):
    v = vigo_handle
    case = fc.by_name("batch:3")
    v.set_params(_params(case.ts_ctrl, case.ts))
    e = fc.expected(case)
    d = v.device
    r = v.traj_finish(to_dev(case.ctrl, d), to_dev(case.limits, d), case.dt, e["S_cap"], n_pts=to_dev(case.n_pts, d), want_max=False, want_vel=False)
    assert r["max"] is None and r["vel"] is None
    assert np.array_equal(u64(r["factor"].cpu().numpy()), u64(e["factor"])) and np.array_equal(r["n"].cpu().numpy(), e["n"])
    n = e["n"]
    for b in range(case.B):
        assert np.array_equal(u64(r["pos"][b, :n[b]].cpu().numpy()), u64(e["pos"][b, :n[b]]))
    empty = v.traj_finish(torch.zeros(0, 9, 3, dtype=torch.float64, device=d), torch.zeros(0, 2, dtype=torch.float64, device=d), 0.1, 4)
    assert empty["factor"].shape == (0,)


def test_whole_call_refusals(vigo_handle):
    v = vigo_handle
    d = v.device
    case = fc.by_name("batch:3")
    ctrl, lim, npts = to_dev(case.ctrl, d), to_dev(case.limits, d), to_dev(case.n_pts, d)
    for bad in (0.0, -0.1, float("inf"), float("nan")):
        with pytest.raises(VigoError, match=r"\(-1\)"):
            v.traj_finish(ctrl, lim, bad, 40, n_pts=npts)
    with pytest.raises(VigoError, match=r"\(-1\)"):
        v.traj_finish(ctrl, lim, 0.1, 0, n_pts=npts)
    for Ns in (6, 257):
        with pytest.raises(VigoError, match=r"\(-4\)"):
            v.traj_finish(torch.zeros(1, Ns, 3, dtype=torch.float64, device=d), torch.ones(1, 2, dtype=torch.float64, device=d), 0.1, 8)
    # a NULL required pointer with B > 0, straight through the C ABI
    f = torch.zeros(3, dtype=torch.float64, device=d)
    n, st = torch.zeros(3, dtype=torch.int32, device=d), torch.zeros(3, dtype=torch.int32, device=d)
    pos = torch.zeros(3, 40, 3, dtype=torch.float64, device=d)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [v._h, 3, case.Ns, p(npts), p(ctrl), p(lim), 0.1, 40, p(f), None, p(n), p(pos), None, p(st)]
    for k in (4, 5, 8, 10, 11, 13):
        broken = list(args)
        broken[k] = None
        assert v._lib.vigo_traj_finish(*broken) == -1, k
    assert v._lib.vigo_traj_finish(*args) == 0
    assert v._lib.vigo_traj_finish(None, *args[1:]) == -1
    torch.cuda.synchronize()
