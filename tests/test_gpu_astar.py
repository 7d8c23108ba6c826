"""-m gpu: vigo_astar_search (csrc/vigo_astar.hip) against the facade's host A* — status, length, every coordinate and
the search's own counts (pops, pushed nodes, heap peak) bit for bit on the crafted cases of tests/astar_cases.py and on
every prologue search of the pipeline batch, with at most 2 % of those deferred — its argument checks, its independence
of the batch, and bsplineTraj::makePlanBatch with setDeviceAstar(true) against the same call with the host A*."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import astar_cases as ac
import plan_batch as pb
from gpu_util import to_dev
from trajectory_planner_amd import _lib, synth
from trajectory_planner_amd.vigo import ASTAR_DEFERRED, ASTAR_FOUND, ASTAR_NOT_FOUND, ASTAR_PATH_TOO_LONG

pytestmark = pytest.mark.gpu


def _dev_search(v, c_or_ends, pool, band, step, **kw):
    ends = np.ascontiguousarray(c_or_ends, dtype=np.float64).reshape(-1, 6)
    st, ln, path, stats = v.astar_search(to_dev(np.ascontiguousarray(ends[:, :3]), v.device), to_dev(np.ascontiguousarray(ends[:, 3:]), v.device), step,
                                         pool, band[0], band[1], **kw)
    torch.cuda.synchronize()
    return st.cpu().numpy(), ln.cpu().numpy(), path.cpu().numpy(), stats.cpu().numpy()


def _capacity():
    max_nodes, max_heap = C.c_int32(0), C.c_int32(0)
    assert _lib.load().vigo_astar_capacity(C.byref(max_nodes), C.byref(max_heap)) == 0
    return max_nodes.value, max_heap.value


def _over_capacity(hstats):
    """the searches the device must defer with an unlimited max_expansions, and the only ones it may: the host search
    pushes more nodes than the table holds, or its open set grows past the heap (vigo_astar_capacity)"""
    max_nodes, max_heap = _capacity()
    hstats = np.asarray(hstats).reshape(-1, 5)
    return (hstats[:, 4] > max_nodes) | (hstats[:, 2] > max_heap)


def test_crafted_cases_equal_the_host_search(vigo_handle):
    v, lib = vigo_handle, ac.host_lib()
    seen = set()
    for c in ac.crafted_cases() + ac.restatement_cases(seeds=range(2), per_seed=6):
        v.set_grid(to_dev(c.vox, v.device), c.origin, c.res)
        host, hs = ac.host_astar(lib, c)
        st, ln, path, stats = _dev_search(v, np.concatenate([c.start, c.end]), c.pool, (c.min_h, c.max_h), c.step, path_cap=512)
        print(f"{c.name}: status {st[0]}, {ln[0]} points, pops / pushed / heap peak {stats[0].tolist()}")
        seen.add(int(st[0]))
        if _over_capacity(hs)[0]:                       # more nodes than the table holds: no result, nothing written
            assert st[0] == ASTAR_DEFERRED and ln[0] == 0 and not path.any(), c.name
            continue
        assert st[0] == (ASTAR_NOT_FOUND if host is None else ASTAR_FOUND), c.name
        if host is not None:
            assert ln[0] == len(host) and np.array_equal(path[0, :ln[0]], host), c.name
        assert stats[0].tolist() == [int(hs[0]), int(hs[4]), int(hs[2])], (c.name, stats[0], hs)
    assert seen == {ASTAR_FOUND, ASTAR_NOT_FOUND, ASTAR_DEFERRED}      # (deferred: "enclosed goal, larger pool" alone)
    # the budgets and the path buffer, on the last grid that holds the detour
    c = next(k for k in ac.crafted_cases() if k.name == "wall: detour")
    v.set_grid(to_dev(c.vox, v.device), c.origin, c.res)
    host, hs = ac.host_astar(lib, c)
    ends = np.concatenate([c.start, c.end])
    st, ln, path, _ = _dev_search(v, ends, c.pool, (c.min_h, c.max_h), c.step, max_expansions=int(hs[0]) - 1)
    assert st[0] == ASTAR_DEFERRED and ln[0] == 0 and not path.any()
    st, ln, path, _ = _dev_search(v, ends, c.pool, (c.min_h, c.max_h), c.step, max_expansions=int(hs[0]))
    assert st[0] == ASTAR_FOUND and np.array_equal(path[0, :ln[0]], host)
    st, ln, path, _ = _dev_search(v, ends, c.pool, (c.min_h, c.max_h), c.step, path_cap=len(host) - 1)
    assert st[0] == ASTAR_PATH_TOO_LONG and ln[0] == len(host) and not path.any()


def test_pipeline_batch_searches_equal_the_host_search_and_do_not_depend_on_the_batch(vigo_handle):
    v, lib = vigo_handle, ac.host_lib()
    world, pool, ends, hlen, hpath, hstats = ac.pipeline_searches(lib)
    band = (float(synth.PIPELINE_CFG[1]), float(synth.PIPELINE_CFG[2]))
    v.set_grid(to_dev(world.voxels, v.device), world.origin, world.res)
    cap = hpath.shape[1]
    st, ln, path, stats = _dev_search(v, ends, pool, band, world.res, path_cap=cap)
    deferred = st == ASTAR_DEFERRED
    print(f"\n{len(ends)} searches: {int((st == ASTAR_FOUND).sum())} found, {int((st == ASTAR_NOT_FOUND).sum())} not found, {int(deferred.sum())} deferred "
          f"({deferred.mean() * 100:.2f} %)")
    assert set(np.unique(st)) <= {ASTAR_FOUND, ASTAR_NOT_FOUND, ASTAR_DEFERRED}
    assert deferred.mean() <= 0.02
    assert np.array_equal(deferred, _over_capacity(hstats))           # deferred for want of room, and only then
    for q in np.nonzero(~deferred)[0]:
        assert st[q] == (ASTAR_FOUND if hlen[q] >= 0 else ASTAR_NOT_FOUND), q
        assert ln[q] == max(int(hlen[q]), 0) and np.array_equal(path[q, :ln[q]], hpath[q, :ln[q]]), q
        assert stats[q].tolist() == [int(hstats[q, 0]), int(hstats[q, 4]), int(hstats[q, 2])], (q, stats[q], hstats[q])
    assert not path[deferred].any()
    # a search alone == the same search inside the whole-batch launch: the longest, the shortest, a deferred one, a few more
    order = np.argsort(hstats[:, 0])
    picks = {int(order[0]), int(order[-1]), int(order[len(order) // 2]), 0, len(ends) - 1}
    if deferred.any():
        picks.add(int(np.nonzero(deferred)[0][0]))
    for q in sorted(picks):
        s1, l1, p1, t1 = _dev_search(v, ends[q], pool, band, world.res, path_cap=cap)
        assert s1[0] == st[q] and l1[0] == ln[q] and np.array_equal(p1[0], path[q]), q
        if st[q] != ASTAR_DEFERRED:
            assert np.array_equal(t1[0], stats[q]), q


def test_argument_checks_write_nothing(vigo_handle):
    v = vigo_handle
    lib = _lib.load()
    d = v.device
    Q = 4
    s = to_dev(np.tile([[-1.0, 0.0, 1.0]], (Q, 1)), d)
    e = to_dev(np.tile([[1.0, 0.0, 1.0]], (Q, 1)), d)
    status = torch.full((Q,), 77, dtype=torch.int32, device=d)
    ln = torch.full((Q,), 77, dtype=torch.int32, device=d)
    path = torch.full((Q, 64, 3), 77.0, dtype=torch.float64, device=d)
    p = lambda t: C.c_void_p(t.data_ptr())
    pool = (C.c_int32 * 3)(40, 40, 40)

    def call(h=v._h, Q=Q, s=p(s), e=p(e), step=0.1, pool=pool, max_exp=1000, path_cap=64, st=p(status), l=p(ln), pa=p(path)):
        return lib.vigo_astar_search(h, Q, s, e, step, pool, 0.7, 1.3, max_exp, path_cap, st, l, pa, None)

    INVALID, NO_GRID, UNSUPPORTED = -1, -5, -6
    assert call() == NO_GRID                                      # before a grid
    v.set_grid(to_dev(np.zeros((48, 48, 24), dtype=np.uint8), d), np.array([-2.4, -2.4, 0.0]), 0.1)
    assert call(h=None) == INVALID
    assert call(Q=-1) == INVALID
    for k in ("s", "e", "st", "l", "pa"):
        assert call(**{k: None}) == INVALID, k
    assert call(pool=None) == INVALID
    assert call(pool=(C.c_int32 * 3)(40, 2, 40)) == INVALID
    assert call(pool=(C.c_int32 * 3)(40, 40, 2000)) == UNSUPPORTED
    for step in (0.0, -0.1, float("nan"), float("inf")):
        assert call(step=step) == INVALID, step
    assert call(path_cap=1) == INVALID
    assert call(max_exp=-1) == INVALID
    assert call(Q=0) == 0 and call(Q=0, s=None, e=None, st=None, l=None, pa=None) == 0
    torch.cuda.synchronize()
    assert (status == 77).all() and (ln == 77).all() and (path == 77.0).all()
    assert call() == 0                                            # and the good call works
    torch.cuda.synchronize()
    assert (status == ASTAR_FOUND).all() and (ln > 1).all()


# ---- the facade ----------------------------------------------------------------------------------------------------
def _facade_world(x0=-0.3, x1=0.3, y0=-0.8, y1=0.8):
    """host/test/test_facade.cpp: a 12.8 m x 12.8 m x 4 m map at 0.1 m with a pillar across the straight paths, and its 1024 paths"""
    n = (128, 128, 40)
    origin = np.array([-6.4, -6.4, -0.5])
    ctr = [origin[a] + (np.arange(n[a]) + 0.5) * 0.1 for a in range(3)]
    X, Y, Z = np.meshgrid(*ctr, indexing="ij")
    vox = np.zeros(n, dtype=np.uint8)
    z0, z1 = -0.5, 3.5
    vox[(X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1) & (Z >= z0) & (Z <= z1)] |= 4
    vox[(X >= x0 - 0.4) & (X <= x1 + 0.4) & (Y >= y0 - 0.4) & (Y <= y1 + 0.4) & (Z >= z0 - 0.15) & (Z <= z1 + 0.15)] |= 1
    return vox, origin


def _facade_paths(P):
    i = np.arange(P)
    y = -2.6 + 5.2 * (i % 97) / 96.0
    tilt = 0.4 * ((i * 37) % 11 - 5) / 5.0
    n = 24                                                        # straight(): int(len / 0.25) segments for len in [6, 6.014)
    t = np.arange(n + 1) / n
    pts = np.zeros((P, n + 1, 3))
    pts[:, :, 0] = -3.0 + 6.0 * t[None, :]
    pts[:, :, 1] = y[:, None] + tilt[:, None] * t[None, :]
    pts[:, :, 2] = 1.0
    return pts


def _plan_twice(P, n_maps=1, budget=16384, reps=1, second_world=None):
    """slot 0: the prologue's A* on the host, slot 1: deviceAstar; alternating, `reps` times"""
    vox, origin = _facade_world()
    r = pb.plan_batch(SimpleNamespace(voxels=vox, origin=origin, res=0.1), *pb.uniform_paths(_facade_paths(P)),
                      [(0, budget, pb.BY_CALL), (pb.ASTAR, budget, pb.BY_CALL)], [0, 1] * reps, outputs=("ok", "solver", "ncp", "ctrl", "guides", "paths"),
                      vox2=_facade_world(**second_world)[0] if second_world else None, n_maps=n_maps, ncp_cap=64, room=64 * P)
    decided, host = pb.stat(r, "astarDecided", "astarHost")[1]
    return dict(device_decided=int(decided), host_run=int(host), prologue_ms=r["slot_seconds"][:, :, 0] * 1e3, total_ms=r["slot_seconds"][:, :, 2] * 1e3,
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_guides", "guides", "n_path_pts", "paths")})


def _same_plans(r, label, device_share, first_world=slice(None)):
    """device_share: the least share of the device-mode call's searches that the DEVICE must have decided (the facade
    falls back to the host A* quietly — no device, no snapshot, a failed launch — and a fallen-back run gives the same
    plan), or 0: none may be"""
    jobs = r["device_decided"] + r["host_run"]
    print(f"\n{label}: {jobs} prologue searches, {r['device_decided']} decided by the device, {r['host_run']} run by the host")
    assert jobs >= (r["n_path_pts"][0] > 0).sum() > 0, label
    if device_share:
        assert r["device_decided"] >= device_share * jobs, label
    else:
        assert r["device_decided"] == 0, label
    for k in ("ok", "solver", "ncp", "n_guides", "n_path_pts", "ctrl", "guides", "paths"):
        assert np.array_equal(r[k][0], r[k][1]), f"{label}: {k} differs between the host A* and the device A*"
    P = r["ok"].shape[1]
    # not a comparison of failures: on test_facade's own map (the planners of first_world) most plans succeed, as there
    ok = r["ok"][0][first_world]
    assert ok.sum() >= len(ok) * 8 // 10 and (r["n_path_pts"][0] > 0).sum() >= P // 10, label
    print(f"\n{label}: {int(r['ok'][0].sum())} of {P} planned, {int((r['n_path_pts'][0] > 0).sum())} with A* paths; prologue host A* "
          f"{np.median(r['prologue_ms'][0]):.2f} ms, device A* {np.median(r['prologue_ms'][1]):.2f} ms; makePlanBatch {np.median(r['total_ms'][0]):.2f} / "
          f"{np.median(r['total_ms'][1]):.2f} ms")


def test_make_plan_batch_with_device_astar_is_the_same_plan():
    _same_plans(_plan_twice(1024, reps=2), "1024 planners", 0.98)


def test_make_plan_batch_with_device_astar_in_groups():
    # the odd planners' map has another pillar (wider, moved): each group's searches have their own answers
    r = _plan_twice(256, n_maps=2, second_world=dict(x0=-0.1, x1=0.6, y0=-1.3, y1=1.1))
    even, odd = slice(0, 256, 2), slice(1, 256, 2)
    _same_plans(r, "256 planners on two different maps", 0.98, first_world=even)
    assert r["ok"][0][odd].sum() > 0
    assert (r["n_path_pts"][0][odd] > 0).sum() > (r["n_path_pts"][0][even] > 0).sum()      # the wider pillar stops more paths


def test_make_plan_batch_with_everything_deferred():
    _same_plans(_plan_twice(256, budget=0), "256 planners, max_expansions 0", 0)
