"""-m gpu: vigo_collision_segs and vigo_path_search (csrc/vigo_pathsearch.hip) against their host twin —
csrc/vigo_pathsearch_core.hpp around the device's search core under the shipped capacities (vigo_host_path_search_core)
— bit for bit on every workload of tests/pathsearch_cases.py: statuses, seg_off, seg, path_off, path (as uint64),
counts; a trajectory alone equals itself inside the batch.  The outputs chain into vigo_guide_assign as device tensors.
Then the error contract, and bsplineTraj::makePlanBatch under setDevicePrologue(true) against the parent's behaviour
(setDeviceGuides(1), host A*) through vigo_host_plan_batch, with the prologue timings printed: the ok flags,
collision segments, A* paths, control points, guides and solver statuses are compared on every planner."""
import ctypes as C

import numpy as np
import pytest
import torch

import guide_cases as gc
import pathsearch_cases as pc
import plan_batch as pb
from gpu_util import to_dev
from trajectory_planner_amd import _lib, synth
from trajectory_planner_amd.vigo import GUIDE_OK, PATHS_DEFERRED, PATHS_FAILED, PATHS_OK

pytestmark = pytest.mark.gpu
CAP = 512                                                         # search_path_cap of these tests


def _dev_search(v, w, **kw):
    d = v.device
    so = None if w.seg_off is None else to_dev(w.seg_off, d)
    sg = None if w.seg is None else to_dev(np.ascontiguousarray(w.seg, dtype=np.int32), d)
    sc, pcap = pc.caps(w, CAP)
    out = v.path_search(to_dev(w.ctrl, d), w.res, w.pool, w.cfg[1], w.cfg[2], seg_off=so, seg=sg, not_check_ratio=w.ncr, search_path_cap=CAP,
                        seg_cap=kw.pop("seg_cap", sc), point_cap=kw.pop("point_cap", pcap), **kw)
    torch.cuda.synchronize()
    st, seg_off, seg, path_off, path, counts = [None if t is None else t.cpu().numpy() for t in out]
    S = int(seg_off[w.B])
    return pc.Result(0, st, seg_off, seg[:S], path_off[:S + 1], path[:path_off[S]], counts), out


def _equal_twin(v, lib, w, label):
    v.set_grid(to_dev(w.vox, v.device), w.origin, w.res)
    t = pc.twin(lib, w, cap=pc.shipped(), search_path_cap=CAP)
    assert t.rc == 0
    r, dev = _dev_search(v, w)
    assert pc.same(r, t) and np.array_equal(r.counts, t.counts), label
    # counts against statuses: a deferred trajectory with segments has an undecided search; all decided -> not deferred
    undecided = r.counts[:, 1] < r.counts[:, 0]
    assert (undecided[(r.status == PATHS_DEFERRED) & (r.counts[:, 0] > 0)]).all() and (r.status[~undecided & (r.counts[:, 0] > 0)] != PATHS_DEFERRED).all()
    assert (np.diff(r.seg_off)[r.status != PATHS_OK] == 0).all()
    if w.seg_off is None:
        rc, seg_off, seg, st = pc.twin_segments(lib, w)
        d_off, d_seg, d_st = v.collision_segs(to_dev(w.ctrl, v.device), w.ncr)
        torch.cuda.synchronize()
        assert rc == 0 and np.array_equal(d_off.cpu().numpy(), seg_off) and np.array_equal(d_seg.cpu().numpy()[:len(seg)], seg)
        assert np.array_equal(d_st.cpu().numpy(), st), label
    print(f"\n{label}: {w.B} trajectories, {len(r.seg)} segments, {len(r.path)} path points; ok / failed / deferred "
          f"{[int((r.status == k).sum()) for k in (0, 1, 2)]}; {int(r.counts[:, 0].sum())} searches, {int(r.counts[:, 1].sum())} decided: device == twin")
    return r, dev


def test_crafted_cases_equal_the_twin(vigo_handle):
    v, lib = vigo_handle, pc.host_lib()
    seen = set()
    for name, w in pc.crafted_workloads():
        for ncr in ((0.0, 0.3) if w.seg_off is None else (0.0,)):
            w.ncr = ncr
            r, _ = _equal_twin(v, lib, w, f"{name}, not_check_ratio {ncr}")
            seen.add(int(r.status[0]))
    assert seen == {PATHS_OK, PATHS_FAILED, PATHS_DEFERRED}
    for N in (120, 60):
        _equal_twin(v, lib, pc.zigzag_workload(N), f"zigzag, {N} control points")


@pytest.mark.parametrize("seed", [None, synth.SEED_BASE + 77])
def test_pipeline_batch_equals_the_twin_chains_into_guide_assign_and_does_not_depend_on_the_batch(vigo_handle, seed):
    v, lib = vigo_handle, pc.host_lib()
    w = pc.pipeline_workload(seed)
    r, dev = _equal_twin(v, lib, w, w.name)
    assert len(r.seg) >= 400 and (r.status == PATHS_DEFERRED).mean() <= 0.02
    # chaining: the device tensors as they are -> vigo_guide_assign == vigo_guide_assign on the host pipeline's lists
    gw, _, _ = gc.pipeline_workload(gc.host_lib(), seed)
    cap = gc.pair_count(gw) + 8
    d = v.device
    ctrl = to_dev(w.ctrl, d)
    off1, pv1, _, st1 = v.guide_assign(ctrl, dev[1], dev[2], dev[3], dev[4], cap)
    off2, pv2, _, st2 = v.guide_assign(ctrl, to_dev(gw.seg_off, d), to_dev(gw.seg, d), to_dev(gw.path_off, d), to_dev(gw.path, d), cap)
    torch.cuda.synchronize()
    off1, pv1, st1, off2, pv2, st2 = [t.cpu().numpy() for t in (off1, pv1, st1, off2, pv2, st2)]
    both = (r.status == PATHS_OK) & (st1 == GUIDE_OK) & (st2 == GUIDE_OK)
    assert both.mean() >= 0.96
    for b in np.nonzero(both)[0]:
        a, c = gw.pairs_of(off1, b), gw.pairs_of(off2, b)
        assert np.array_equal(np.diff(off1[b * w.N:(b + 1) * w.N + 1]), np.diff(off2[b * w.N:(b + 1) * w.N + 1])), b
        assert np.array_equal(gc.bits(pv1[a]), gc.bits(pv2[c])), b
    # alone: the trajectory with the most segments, the most path points, a deferred one, the first and the last
    n_seg = np.diff(r.seg_off)
    pts = np.array([r.path_off[r.seg_off[b + 1]] - r.path_off[r.seg_off[b]] for b in range(w.B)])
    picks = {int(np.argmax(n_seg)), int(np.argmax(pts)), 0, w.B - 1}
    if (r.status == PATHS_DEFERRED).any():
        picks.add(int(np.nonzero(r.status == PATHS_DEFERRED)[0][0]))
    for b in sorted(picks):
        r1, _ = _dev_search(v, w.subset([b]))
        a, c = r1.of(0), r.of(b)
        assert a[0] == c[0] and np.array_equal(a[1], c[1]) and len(a[2]) == len(c[2]) and np.array_equal(r1.counts[0], r.counts[b]), b
        assert all(np.array_equal(pc.bits(x), pc.bits(y)) for x, y in zip(a[2], c[2])), b


def test_error_contract_writes_nothing(vigo_handle):
    v = vigo_handle
    lib = _lib.load()
    d = v.device
    w = dict(pc.crafted_workloads())["a supplied list that differs from the scanned one"]
    B, N = 3, w.N
    ctrl = to_dev(np.ascontiguousarray(np.tile(w.ctrl, (B, 1, 1))), d)
    seg_off = np.array([0, 2, 2, 4], dtype=np.int32)
    seg = np.array([[13, 19], [20, 22], [13, 19], [20, 22]], dtype=np.int32)
    t_so, t_sg = to_dev(seg_off, d), to_dev(seg, d)
    seg_cap, point_cap = 8, 8 * (CAP + 1)
    st = torch.full((B,), 77, dtype=torch.int32, device=d)
    o_so = torch.full((B + 1,), 77, dtype=torch.int32, device=d)
    o_sg = torch.full((seg_cap, 2), 77, dtype=torch.int32, device=d)
    o_po = torch.full((seg_cap + 1,), 77, dtype=torch.int32, device=d)
    o_pa = torch.full((point_cap, 3), 77.0, dtype=torch.float64, device=d)
    o_ct = torch.full((B, 2), 77, dtype=torch.int32, device=d)
    p = lambda x: C.c_void_p(x.data_ptr())
    pool = (C.c_int32 * 3)(*w.pool)

    def call(h=v._h, B=B, N=N, ctrl=p(ctrl), so=p(t_so), sg=p(t_sg), ncr=0.0, step=0.1, pool=pool, max_exp=100000, cap=CAP, seg_cap=seg_cap,
             point_cap=point_cap, st=p(st), o_so=p(o_so), o_sg=p(o_sg), o_po=p(o_po), o_pa=p(o_pa), o_ct=p(o_ct)):
        return lib.vigo_path_search(h, B, N, ctrl, so, sg, ncr, step, pool, 0.7, 1.3, max_exp, cap, seg_cap, point_cap, st, o_so, o_sg, o_po, o_pa, o_ct)

    def segs(h=v._h, B=B, N=N, ctrl=p(ctrl), ncr=0.0, seg_cap=seg_cap, o_so=p(o_so), o_sg=p(o_sg), st=p(st)):
        return lib.vigo_collision_segs(h, B, N, ctrl, ncr, o_so, o_sg, seg_cap, st)

    INVALID, NO_GRID, UNSUPPORTED = -1, -5, -6
    assert call() == NO_GRID and segs() == NO_GRID                # before a grid
    v.set_grid(to_dev(w.vox, d), w.origin, w.res)
    assert call(h=None) == INVALID and segs(h=None) == INVALID
    assert call(B=-1) == INVALID and call(N=6) == INVALID and segs(B=-1) == INVALID and segs(N=6) == INVALID
    for k in ("ctrl", "st", "o_so", "o_sg", "o_po", "o_pa"):
        assert call(**{k: None}) == INVALID, k
    for k in ("ctrl", "st", "o_so", "o_sg"):
        assert segs(**{k: None}) == INVALID, k
    assert call(so=None) == INVALID and call(sg=None) == INVALID  # a list is offsets AND segments
    bad = seg_off.copy()
    bad[2] = 1                                                    # offsets that decrease
    assert call(so=p(to_dev(bad, d))) == INVALID
    bad = seg_off.copy()
    bad[0] = -1
    assert call(so=p(to_dev(bad, d))) == INVALID
    for row in ((13, N), (-1, 19)):                               # a segment end that is not a control point
        bad = seg.copy()
        bad[2] = row
        assert call(sg=p(to_dev(bad, d))) == INVALID, row
    assert call(seg_cap=3) == INVALID and call(seg_cap=-1) == INVALID          # seg_cap too small
    assert call(point_cap=10) == INVALID and call(point_cap=-1) == INVALID     # point_cap too small
    assert call(pool=None) == INVALID and call(pool=(C.c_int32 * 3)(16, 2, 8)) == INVALID
    assert call(pool=(C.c_int32 * 3)(16, 16, 2000)) == UNSUPPORTED
    for step in (0.0, -0.1, float("nan"), float("inf")):
        assert call(step=step) == INVALID, step
    assert call(cap=1) == INVALID and call(max_exp=-1) == INVALID
    for ncr in (-0.1, 1.5, float("nan")):
        assert call(so=None, sg=None, ncr=ncr) == INVALID and segs(ncr=ncr) == INVALID, ncr
    assert segs(seg_cap=2) == INVALID and segs(seg_cap=-1) == INVALID          # (three trajectories with one segment each)
    assert call(B=0) == 0 and segs(B=0) == 0
    assert call(B=0, ctrl=None, so=None, sg=None, st=None, o_so=None, o_sg=None, o_po=None, o_pa=None, o_ct=None) == 0
    torch.cuda.synchronize()
    for t in (st, o_so, o_sg, o_po, o_ct):
        assert (t == 77).all()
    assert (o_pa == 77.0).all()
    assert call(seg_cap=4) == 0                                   # and the good call works, with exactly enough segments
    torch.cuda.synchronize()
    assert st.tolist() == [PATHS_OK] * 3 and o_so.tolist() == [0, 2, 2, 4] and o_sg[:4].tolist() == seg.tolist() and int(o_po[4]) > 8
    total = int(o_po[4])
    assert call(point_cap=total - 1) == INVALID and call(point_cap=total, o_ct=None) == 0
    assert segs(seg_cap=3) == 0
    torch.cuda.synchronize()
    assert o_so.tolist() == [0, 1, 2, 3] and o_sg[:3].tolist() == [[14, 17]] * 3


# ---- the facade ----------------------------------------------------------------------------------------------------
def _pipeline_paths(P, N=32, seed=11):
    """P straight jittered paths of N - 2 poses with free ends on the pipeline world (synth.make_pipeline_batch's candidates,
    plannable or not)"""
    world = synth.make_pipeline_world()
    rng = np.random.default_rng(seed)
    K = N - 2
    s = np.arange(K) * synth.CTRL_SPACING
    out = []
    while sum(len(x) for x in out) < P:
        M = 2 * P
        start = np.concatenate([rng.uniform(-8.0, 8.0, size=(M, 2)), np.full((M, 1), 1.0)], axis=1)
        heading = rng.uniform(0.0, 2 * np.pi, size=M)
        dirv = np.stack([np.cos(heading), np.sin(heading), np.zeros(M)], axis=1)
        lat = np.stack([-np.sin(heading), np.cos(heading), np.zeros(M)], axis=1)
        pts = start[:, None, :] + s[None, :, None] * dirv[:, None, :] + rng.normal(0.0, 0.05, size=(M, K, 1)) * lat[:, None, :]
        out.append(pts[(synth.lookup(world, pts[:, 0], 0) == 0) & (synth.lookup(world, pts[:, -1], 0) == 0)])
    return world, np.ascontiguousarray(np.concatenate(out)[:P])


def _plan(P, slots, budget=16384, reps=1):
    """`reps` rounds over the slots of `slots` (bit k: slot k runs): 0 deviceGuides = 1 (the reference point of slot 1), 1
    devicePrologue, 2 deviceAstar + deviceGuides = 1 (the device pieces without the chain), 3 the host prologue"""
    world, pts = _pipeline_paths(P)
    masks = (pb.GUIDES1, pb.PROLOGUE, pb.ASTAR | pb.GUIDES1, 0)
    r = pb.plan_batch(world, *pb.uniform_paths(pts), [(m, budget, pb.BY_CALL) for m in masks], [s for s in range(4) if (slots >> s) & 1] * reps,
                      outputs=("ok", "solver", "ncp", "ctrl", "segs", "paths", "guides"), ncp_cap=64)
    ms = r["slot_seconds"] * 1e3
    return dict(prologue_ms=ms[:, :, 0], chain_ms=ms[:, :, 1], total_ms=ms[:, :, 2], counts=pb.stat(r, "prologueDecided", "prologueHost"),
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_seg", "segs", "n_path_pts", "paths", "n_guides", "guides")})


def _same_plans(r, label, device_share):
    """slot 1 (setDevicePrologue(true)) against slot 0 (the parent's behaviour: setDeviceGuides(1), host A*)"""
    P = r["ok"].shape[1]
    dev, host = int(r["counts"][1, 0]), int(r["counts"][1, 1])
    print(f"\n{label}: {dev} planners decided by the device chain, {host} by the host steps; {int(r['ok'][0].sum())} of {P} planned, "
          f"{int((r['n_path_pts'][0] > 0).sum())} with A* paths; prologue {np.median(r['prologue_ms'][0]):.2f} ms (parent) / "
          f"{np.median(r['prologue_ms'][1]):.2f} ms (device prologue, chain {np.median(r['chain_ms'][1]):.2f} ms)")
    assert r["counts"][0].tolist() == [0, 0] and dev + host == P
    searched = int((r["n_path_pts"][0] > 0).sum())                # (at least: a planner whose first search fails has no path either)
    if device_share:
        assert dev >= device_share * P, label
    else:                                                         # starved searches: only planners without a search are the device's
        assert host >= searched and dev <= P - searched, label
    for k in ("ok", "solver", "ncp", "n_guides"):
        assert np.array_equal(r[k][0], r[k][1]), f"{label}: {k} differs"
    for k in ("ctrl", "guides"):
        assert np.array_equal(gc.bits(r[k][0]), gc.bits(r[k][1])), f"{label}: {k} differs"
    # collisionSeg_ and astarPaths_ of EVERY planner, those whose path search failed included (the host leaves the scanned
    # segments and the paths found before the failure there)
    for k in ("n_seg", "n_path_pts"):
        assert np.array_equal(r[k][0], r[k][1]), f"{label}: {k} differs"
    S, W = int(r["n_seg"][0].sum()), int(r["n_path_pts"][0].sum())
    assert np.array_equal(r["segs"][0][:S], r["segs"][1][:S]), f"{label}: collision segments differ"
    assert np.array_equal(gc.bits(r["paths"][0][:W]), gc.bits(r["paths"][1][:W])), f"{label}: A* paths differ"
    unprepared = (r["ok"][0] == 0) & (r["n_guides"][0] == 0)
    print(f"{label}: {S} collision segments and {W} path points identical; {int(unprepared.sum())} planners without guides "
          f"(failed path search), {int((unprepared & (r['n_seg'][0] > 0)).sum())} of them with segments left")
    assert r["ok"][0].sum() >= P // 2 and (r["n_path_pts"][0] > 0).sum() >= P // 10, label


def test_make_plan_batch_with_the_device_prologue_is_the_same_plan():
    _same_plans(_plan(1024, slots=0b0011), "1024 planners of the pipeline world", 0.98)


def test_make_plan_batch_with_everything_deferred():
    """max_expansions 0: every search comes back VIGO_ASTAR_DEFERRED, so every planner with a collision segment runs the host steps"""
    _same_plans(_plan(256, slots=0b0011, budget=0), "256 planners, max_expansions 0", 0)


def test_prologue_timings_are_reported(vigo_handle):
    """the prologue of one 1024-planner makePlanBatch on the pipeline world, median of 5 alternating repetitions after a
    warm-up round: host, the parent's device pieces, the device prologue — and vigo_path_search alone under HIP events
    (profiles/README.md, "Device prologue", holds a run of this)"""
    r = _plan(1024, slots=0b1110, reps=6)
    med = np.median(r["prologue_ms"][:, 1:], axis=1)
    print(f"\nprologue ms per 1024 planners, median of 5 after a warm-up: host {med[3]:.2f}, setDeviceAstar + setDeviceGuides(1) {med[2]:.2f}, "
          f"setDevicePrologue {med[1]:.2f} (its device chains {np.median(r['chain_ms'][1, 1:]):.2f}); all runs {np.round(r['prologue_ms'][1:], 2).tolist()}")
    assert (r["prologue_ms"][1:] > 0).all()
    v = vigo_handle
    w = pc.pipeline_workload()
    v.set_grid(to_dev(w.vox, v.device), w.origin, w.res)
    ctrl = to_dev(w.ctrl, v.device)
    ms = []
    for k in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v.path_search(ctrl, w.res, w.pool, w.cfg[1], w.cfg[2], max_expansions=16384, search_path_cap=128, seg_cap=8 * w.B, point_cap=8 * w.B * 129)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(f"vigo_path_search alone, 1024 trajectories of the pipeline batch, HIP events: median of 5 after two warm-up calls {np.median(ms[2:]):.3f} ms "
          f"(all {np.round(ms, 3).tolist()})")
