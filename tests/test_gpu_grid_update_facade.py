"""-m gpu: a map that changes under planners that share it, through vigo_host_map_update_replan (host/src/cabi_host.cpp): 16
bsplineTraj planners on ONE dense map plan by makePlanBatch after the first upload and after each of 4 edits of the map.  The
owner tells the planners of an edit either by a bare ++version (mode 0: the snapshot is replaced whole, as before) or by
markChanged(lo, n) (mode 1: mapAdapter::uploadSnapshot sends the box alone, vigo_update_grid_region_host).  Both must plan
the same, bit for bit, in every round, and mapAdapter::snapshotTotals must show which route ran.

World: 60 x 60 x 20 voxels of 0.1 m with seeded pillars like tests/seed_cases.pillar_world, a band of |y| < 1 m and the
columns of the starts and goals kept free.  The planners cross the band along x, 21 poses each, planner 0 down its middle.
Edit 1 drops a pillar onto planner 0's path and misses the others by 0.1 m and more.

The totals count uploads per HANDLE, and a batch stage runs on the handle of the first planner of its group.  Here every
planner has one control-point count and only planner 0 ever collides, so every group of every stage starts with planner 0
and one handle holds the snapshot: 1 whole snapshot for the first upload, then one upload per edit."""
import ctypes as C
import os

import numpy as np
import pytest

from trajectory_planner_amd import synth

pytestmark = pytest.mark.gpu
LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
ORIGIN, RES = np.array([-3.0, -3.0, 0.0]), 0.1
P, NCP_CAP = 16, 96
PILLAR_EDIT = 1


def world():
    rng = np.random.default_rng(5)
    vox = np.zeros((60, 60, 20), np.uint8)
    for _ in range(25):
        c = rng.integers(3, 57, size=2)
        s = rng.integers(1, 4, size=2)
        vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], :] |= int(rng.choice([1, 3, 3]))
    vox[:, 20:40, :] = 0          # the free band
    vox[:9, :, :] = 0             # starts
    vox[51:, :, :] = 0            # goals
    return vox


def paths():
    ys = np.concatenate([[0.0], 0.3 + 0.08 * np.arange(8), -0.3 - 0.08 * np.arange(7)])   # planner 0 first
    xs = -2.5 + synth.CTRL_SPACING * np.arange(21)
    xyz = np.stack([np.stack([xs, np.full_like(xs, y), np.full_like(xs, 1.0)], axis=1) for y in ys])
    return (21 * np.arange(P + 1)).astype(np.int32), np.ascontiguousarray(xyz.reshape(-1, 3))


def edits():
    """(lo, bytes [n0, n1, n2]): a pillar off the band, THE pillar on planner 0's path (x and y in [-0.2, 0.2)), a cleared block, an unknown block"""
    return [((14, 42, 0), np.full((4, 4, 20), 1, np.uint8)),
            ((28, 28, 0), np.full((4, 4, 20), 1, np.uint8)),
            ((33, 8, 0), np.zeros((12, 14, 20), np.uint8)),
            ((20, 45, 3), np.full((10, 5, 9), 2, np.uint8))]


def replan(mode, mask=0):
    lib = C.CDLL(LIB)
    vox, (off, xyz), ed = world(), paths(), edits()
    E = len(ed)
    lo = np.array([e[0] for e in ed], dtype=np.int32)
    n = np.array([e[1].shape for e in ed], dtype=np.int32)
    eoff = np.concatenate([[0], np.cumsum([e[1].size for e in ed])]).astype(np.int64)
    ebytes = np.concatenate([e[1].reshape(-1) for e in ed])
    cfg = np.ascontiguousarray(synth.PIPELINE_CFG, dtype=np.float64)
    ok, solver, ncp = (np.zeros((E + 1, P), dtype=np.int32) for _ in range(3))
    ctrl, totals, ms = np.zeros((E + 1, P, NCP_CAP, 3)), np.zeros(3, dtype=np.int64), np.zeros(E + 1)
    vp = C.c_void_p
    lib.vigo_host_map_update_replan.restype = C.c_int
    lib.vigo_host_map_update_replan.argtypes = [vp, vp, vp, C.c_double, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int,
                                                vp, vp, vp, vp, vp, vp]
    dims = np.array(vox.shape, dtype=np.int32)
    rc = lib.vigo_host_map_update_replan(vox.ctypes.data, dims.ctypes.data, ORIGIN.ctypes.data, RES, P, off.ctypes.data, xyz.ctypes.data,
                                         cfg.ctypes.data, mask, E, lo.ctypes.data, n.ctypes.data, eoff.ctypes.data, ebytes.ctypes.data, mode, NCP_CAP,
                                         ok.ctypes.data, solver.ctypes.data, ncp.ctypes.data, ctrl.ctypes.data, totals.ctypes.data, ms.ctypes.data)
    assert rc == 0, rc
    return dict(ok=ok, solver=solver, ncp=ncp, ctrl=ctrl, totals=totals.tolist(), ms=ms, voxels=int(sum(e[1].size for e in ed)))


@pytest.fixture(scope="module")
def runs():
    return replan(0), replan(1)


def test_both_routes_plan_the_same_in_every_round(runs):
    full, region = runs
    print(f"\nplanned per round: {full['ok'].sum(1).tolist()}; ms per round, whole snapshots {np.round(full['ms'], 2).tolist()}, "
          f"boxes {np.round(region['ms'], 2).tolist()}")
    for k in ("ok", "solver", "ncp"):
        assert np.array_equal(full[k], region[k]), k
    same = full["ctrl"].view(np.int64) == region["ctrl"].view(np.int64)
    assert same.all(), np.argwhere(~same)[:4].tolist()
    assert full["ok"].sum(1).min() >= 1 and len(set(full["ncp"].reshape(-1).tolist())) == 1


def test_snapshot_totals_show_the_route(runs):
    full, region = runs
    E = len(edits())
    assert full["totals"] == [1 + E, 0, 0]
    assert region["totals"] == [1, E, region["voxels"]]


def test_the_pillar_edit_is_seen(runs):
    for r in runs:
        before, after = r["ctrl"][PILLAR_EDIT], r["ctrl"][PILLAR_EDIT + 1]
        moved = [t for t in range(P) if not np.array_equal(before[t], after[t]) or r["ok"][PILLAR_EDIT][t] != r["ok"][PILLAR_EDIT + 1][t]]
        assert 0 in moved, moved
