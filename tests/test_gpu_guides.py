"""-m gpu: vigo_guide_assign (csrc/vigo_guides.hip) against its host twin — csrc/vigo_guide_core.hpp with vigo_atan2,
compiled for the host (vigo_host_guide_core, mode 1) — bit for bit: offsets, pairs (compared as uint64: the NaNs of a zero
diff must match too), the unknown flags against vigo_guides_unknown, statuses, on every workload of tests/guide_cases.py;
a trajectory's pairs must not depend on its batch.  Then the entry's error contract, and bsplineTraj::makePlanBatch under
setDeviceGuides(0 | 1 | 2) through vigo_host_plan_batch, with the prologue timings."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guide_cases as gc
import plan_batch as pb
from gpu_util import to_dev
from trajectory_planner_amd import _lib, synth
from trajectory_planner_amd.vigo import GUIDE_DEFERRED, GUIDE_OK

pytestmark = pytest.mark.gpu


def _pad(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.size else np.zeros((4,) + a.shape[1:], dtype=dtype)      # (an empty tensor has no device pointer)


def _dev_assign(v, w, pair_cap=None, want_unknown=True):
    cap = gc.pair_count(w) + 8 if pair_cap is None else pair_cap
    d = v.device
    off, pv, unk, st = v.guide_assign(to_dev(w.ctrl, d), to_dev(w.seg_off, d), to_dev(_pad(w.seg, np.int32), d), to_dev(w.path_off, d),
                                      to_dev(_pad(w.path, np.float64), d), cap, want_unknown=want_unknown)
    torch.cuda.synchronize()
    off = off.cpu().numpy()
    g = int(off[-1])
    return off, pv.cpu().numpy()[:g], (unk.cpu().numpy()[:g] if want_unknown else None), st.cpu().numpy(), pv


def _equal_twin(v, lib, w, label):
    """the kernel == mode 1 with the shipped capacity; returns the twin's outputs"""
    v.set_grid(to_dev(w.vox, v.device), w.origin, w.res)
    rc, off, pv, unk, st, _ = gc.core(lib, w, 1, path_cap=gc.capacity())
    assert rc == 0
    d_off, d_pv, d_unk, d_st, pv_dev = _dev_assign(v, w)
    assert np.array_equal(d_st, st), label
    assert np.array_equal(d_off, off), label
    assert d_pv.shape == pv.shape and np.array_equal(gc.bits(d_pv), gc.bits(pv)), \
        (label, int((gc.bits(d_pv) != gc.bits(pv)).any(axis=1).sum()), len(pv))
    assert np.array_equal(d_unk, unk), label
    if len(pv):
        ref_unk = v.guides_unknown(pv_dev[:len(pv)].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(d_unk, ref_unk.cpu().numpy()), label
    print(f"\n{label}: {w.B} trajectories, {len(w.seg)} segments, {len(pv)} pairs, {int((st == GUIDE_DEFERRED).sum())} deferred: device == twin")
    return off, pv, st


def test_crafted_cases_equal_the_twin(vigo_handle):
    v, lib = vigo_handle, gc.host_lib()
    w, names = gc.crafted_workload(long_path=gc.capacity() + 44)
    off, pv, st = _equal_twin(v, lib, w, "crafted")
    long_b = names.index("a path longer than the device buffer")
    assert st[long_b] == GUIDE_DEFERRED and off[long_b * w.N] == off[(long_b + 1) * w.N]
    assert (np.delete(st, long_b) == GUIDE_OK).all()
    assert np.isnan(pv).any() and (w.vox & 2).any()               # the zero diff is in; unknown voxels exist
    # a path of exactly the capacity is taken
    w2, _ = gc.crafted_workload(long_path=gc.capacity())
    _, _, st2 = _equal_twin(v, lib, w2, "crafted, the long path at the capacity")
    assert (st2 == GUIDE_OK).all()


@pytest.mark.parametrize("seed", [None, synth.SEED_BASE + 77])
def test_pipeline_prologue_equals_the_twin_and_does_not_depend_on_the_batch(vigo_handle, seed):
    v, lib = vigo_handle, gc.host_lib()
    w, _, _ = gc.pipeline_workload(lib, seed)
    assert len(w.seg) >= 400
    off, pv, st = _equal_twin(v, lib, w, w.name)
    assert (st == GUIDE_DEFERRED).mean() <= 0.02
    # shuffled: every trajectory keeps its pairs
    perm = np.random.default_rng(5).permutation(w.B)
    ws = w.subset(perm)
    s_off, s_pv, _, s_st, _ = _dev_assign(v, ws)
    for k, b in enumerate(perm):
        a, c = ws.pairs_of(s_off, k), w.pairs_of(off, b)
        assert s_st[k] == st[b] and np.array_equal(gc.bits(s_pv[a]), gc.bits(pv[c])), (k, b)
        assert np.array_equal(np.diff(s_off[k * w.N:(k + 1) * w.N + 1]), np.diff(off[b * w.N:(b + 1) * w.N + 1])), (k, b)
    # alone: the trajectories with the most pairs, the longest path, the first and the last with segments
    n_pairs = off[w.N::w.N] - off[:-1:w.N]
    with_seg = np.nonzero(np.diff(w.seg_off) > 0)[0]
    longest = int(np.searchsorted(w.seg_off, np.argmax(np.diff(w.path_off)), side="right") - 1)
    for b in sorted({int(np.argmax(n_pairs)), longest, int(with_seg[0]), int(with_seg[-1])}):
        w1 = w.subset([b])
        o1, p1, _, s1, _ = _dev_assign(v, w1)
        assert s1[0] == st[b] and np.array_equal(gc.bits(p1), gc.bits(pv[w.pairs_of(off, b)])), b


def test_error_contract_writes_nothing(vigo_handle):
    v = vigo_handle
    lib = _lib.load()
    d = v.device
    w, _ = gc.crafted_workload()
    cap = gc.pair_count(w) + 8
    t = dict(ctrl=to_dev(w.ctrl, d), seg_off=to_dev(w.seg_off, d), seg=to_dev(w.seg, d), path_off=to_dev(w.path_off, d), path=to_dev(w.path, d))
    off = torch.full((w.B * w.N + 1,), 77, dtype=torch.int32, device=d)
    pv = torch.full((cap, 6), 77.0, dtype=torch.float64, device=d)
    unk = torch.full((cap,), 77, dtype=torch.uint8, device=d)
    st = torch.full((w.B,), 77, dtype=torch.int32, device=d)
    p = lambda x: C.c_void_p(x.data_ptr())

    def call(h=v._h, B=w.B, N=w.N, ctrl=p(t["ctrl"]), seg_off=p(t["seg_off"]), seg=p(t["seg"]), path_off=p(t["path_off"]), path=p(t["path"]),
             pair_cap=cap, off=p(off), pv=p(pv), unk=p(unk), st=p(st)):
        return lib.vigo_guide_assign(h, B, N, ctrl, seg_off, seg, path_off, path, pair_cap, off, pv, unk, st)

    INVALID, NO_GRID = -1, -5
    assert call() == NO_GRID                                      # before a grid
    v.set_grid(to_dev(w.vox, d), w.origin, w.res)
    assert call(h=None) == INVALID
    assert call(B=-1) == INVALID and call(N=0) == INVALID and call(pair_cap=-1) == INVALID
    for k in ("ctrl", "seg_off", "seg", "path_off", "path", "off", "pv", "st"):
        assert call(**{k: None}) == INVALID, k
    bad = w.seg_off.copy()
    bad[3], bad[4] = bad[4], bad[3] - 1                           # offsets that decrease
    assert bad[4] < bad[3]
    assert call(seg_off=p(to_dev(bad, d))) == INVALID
    bad = w.path_off.copy()
    bad[2] = bad[1] - 1
    assert call(path_off=p(to_dev(bad, d))) == INVALID
    bad = w.seg.copy()
    bad[1] = (-1, 0)                                              # a line collision whose own ends are not control points
    assert call(seg=p(to_dev(bad, d))) == INVALID
    total = gc.pair_count(w) - 8                                  # (the long path's trajectory is deferred: its 8 pairs are not counted)
    assert call(pair_cap=total - 1) == INVALID                    # pair_cap too small
    assert call(B=0) == 0 and call(B=0, ctrl=None, seg_off=None, seg=None, path_off=None, path=None, off=None, pv=None, unk=None, st=None) == 0
    torch.cuda.synchronize()
    assert (off == 77).all() and (pv == 77.0).all() and (unk == 77).all() and (st == 77).all()
    assert call(pair_cap=total) == 0 and call(unk=None) == 0      # and the good call works, with exactly enough room
    torch.cuda.synchronize()
    assert int(off[-1]) == total and (st != 77).all()


# ---- the facade ----------------------------------------------------------------------------------------------------
def _plan(P, astar, reps):
    """slot 0: the untouched default, once, first; then `reps` rounds over slots 1, 2, 3: deviceGuides 0, 1, 2"""
    from test_gpu_astar import _facade_paths, _facade_world
    vox, origin = _facade_world()
    slots = [(0, 16384, pb.UNTOUCHED)] + [((pb.ASTAR if astar else 0) | guides << 1, 16384, pb.BY_CALL) for guides in (0, 1, 2)]
    r = pb.plan_batch(SimpleNamespace(voxels=vox, origin=origin, res=0.1), *pb.uniform_paths(_facade_paths(P)), slots, [0] + [1, 2, 3] * reps,
                      outputs=("ok", "solver", "ncp", "ctrl", "guides"), ncp_cap=64, room=64 * P)
    return dict(prologue_ms=r["slot_seconds"][:, :, 0] * 1e3, total_ms=r["slot_seconds"][:, :, 2] * 1e3, counts=pb.stat(r, "guidesDecided", "guidesHost"),
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_guides", "guides")})


def test_make_plan_batch_under_the_three_settings():
    """slots: 0 = a run before any setter is touched, 1 / 2 / 3 = setDeviceGuides(0 / 1 / 2)"""
    P = 1024
    r = _plan(P, astar=0, reps=1)
    dev, host = r["counts"][:, 0], r["counts"][:, 1]
    print(f"\ntrajectories with guides: device / workers' twin: setting 1 {dev[2]} / {host[2]}, setting 2 {dev[3]} / {host[3]}")
    assert dev[0] == host[0] == dev[1] == host[1] == 0            # setting 0 never enters the new path
    assert dev[3] == 0 and host[3] > P // 10
    assert dev[2] + host[2] == host[3] and dev[2] >= 0.98 * (dev[2] + host[2])
    for k in ("ok", "solver", "ncp", "n_guides"):
        assert np.array_equal(r[k][2], r[k][3]), f"{k}: settings 1 and 2 differ"
        assert np.array_equal(r[k][0], r[k][1]), f"{k}: setting 0 differs from the untouched default"
    for k in ("ctrl", "guides"):
        assert np.array_equal(gc.bits(r[k][2]), gc.bits(r[k][3])), f"{k}: settings 1 and 2 differ"
        assert np.array_equal(gc.bits(r[k][0]), gc.bits(r[k][1])), f"{k}: setting 0 differs from the untouched default"
    assert r["ok"][0].sum() >= P * 8 // 10 and (r["n_guides"][0] > 0).sum() >= P // 10
    # reported, not gated: settings 1 against 0 (a few-ulp change in a guide is amplified by 200 L-BFGS iterations)
    same_ok = (r["ok"][1] == r["ok"][2]).mean()
    same_ng = (r["n_guides"][1] == r["n_guides"][2]).mean()
    n = np.minimum(r["ncp"][1], r["ncp"][2])
    close = tot = 0
    for t in range(P):
        dlt = np.abs(r["ctrl"][1][t, :n[t]] - r["ctrl"][2][t, :n[t]]).max(axis=1)
        close += int((dlt <= 1e-4).sum())
        tot += int(n[t])
    print(f"setting 1 against setting 0: ok flags agree on {same_ok * 100:.2f} %, guide counts on {same_ng * 100:.2f} %, "
          f"{close / tot * 100:.3f} % of {tot} control points within 1e-4")


def test_prologue_timings_are_reported():
    """the prologue's wall time per 1024 planners under settings 0 and 1, with the device A* off and on: the median of 5
    alternating repetitions (profiles/README.md holds a run of this)"""
    for astar in (0, 1):
        r = _plan(1024, astar=astar, reps=5)
        med = np.median(r["prologue_ms"][1:], axis=1)
        medt = np.median(r["total_ms"][1:], axis=1)
        print(f"\ndevice A* {'on' if astar else 'off'}: prologue ms per 1024 planners, median of 5: setting 0 {med[0]:.2f}, setting 1 {med[1]:.2f}, "
              f"setting 2 {med[2]:.2f} (all runs: {np.round(r['prologue_ms'][1:], 2).tolist()}); makePlanBatch {medt[0]:.1f} / {medt[1]:.1f} / {medt[2]:.1f} ms")
        assert (r["prologue_ms"][1:] > 0).all()
        for k in ("ok", "n_guides"):
            assert np.array_equal(r[k][2], r[k][3])
