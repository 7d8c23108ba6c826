"""-m gpu: bsplineTraj::isCurrTrajValidBatch through vigo_host_validate_batch and vigo_host_map_update_validate
(host/src/cabi_host.cpp): the workload of tests/test_gpu_mixed_facade.py — 48 planners of the small world over ten
control-point counts — held as fitted plans, plus a planner without a device, one that is not initialised and one of more
than 256 control points.  The batch form's flags, first-collision positions (bits) and dynamic flags equal the per-planner
loop's (isCurrTrajValid(pos), hasDynamicCollisionTrajectory); all counts share one device group; the three odd planners take
the host route; the stats add up.  Then a wall written into the shared map, announced by its owner, and removed again."""
import ctypes as C
import os

import numpy as np
import pytest

import mixed_cases as mc
from test_gpu_mixed_facade import POSES
from trajectory_planner_amd import synth

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e33
N_WORKLOAD = 48
NO_DEVICE, NOT_INIT = 5, 9


def _lib():
    lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so"))
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    lib.vigo_host_validate_batch.restype = C.c_int
    lib.vigo_host_validate_batch.argtypes = [C.c_void_p, ip, dp, C.c_double, C.c_int, ip, dp, dp, C.c_int, C.c_int, ip, dp, ip, dp, ip, ip, lp, lp, C.c_int, dp]
    lib.vigo_host_map_update_validate.restype = C.c_int
    lib.vigo_host_map_update_validate.argtypes = [C.c_void_p, ip, dp, C.c_double, C.c_int, ip, dp, dp, C.c_int, ip, ip, lp, C.c_void_p, C.c_int, ip, dp, ip,
                                                  lp, lp]
    return lib, dp, ip, lp


def validate_batch(world, path_off, xyz, no_device=-1, not_init=-1, obs_off=None, obs=None, cfg=synth.PIPELINE_CFG, reps=0):
    lib, dp, ip, lp = _lib()
    n = len(path_off) - 1
    vox, origin = np.ascontiguousarray(world.voxels), np.ascontiguousarray(world.origin, dtype=np.float64)
    cfg, off, xyz = np.ascontiguousarray(cfg, dtype=np.float64), np.ascontiguousarray(path_off, dtype=np.int32), np.ascontiguousarray(xyz)
    valid, dyn, ncp = np.full((2, n), -1, dtype=np.int32), np.full((2, n), -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    pos = np.full((2, n, 3), SENTINEL)
    stats, totals, ms = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros((max(reps, 1), 2))
    ooff = None if obs_off is None else np.ascontiguousarray(obs_off, dtype=np.int32)
    ob = None if obs is None else np.ascontiguousarray(obs, dtype=np.float64)
    rc = lib.vigo_host_validate_batch(vox.ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), origin.ctypes.data_as(dp), float(world.res), n,
                                      off.ctypes.data_as(ip), xyz.ctypes.data_as(dp), cfg.ctypes.data_as(dp), no_device, not_init,
                                      None if ooff is None else ooff.ctypes.data_as(ip), None if ob is None else ob.ctypes.data_as(dp),
                                      valid.ctypes.data_as(ip), pos.ctypes.data_as(dp), dyn.ctypes.data_as(ip), ncp.ctypes.data_as(ip),
                                      stats.ctypes.data_as(lp), totals.ctypes.data_as(lp), reps, ms.ctypes.data_as(dp))
    assert rc == 0, rc
    return dict(valid=valid, pos=pos, dyn=dyn, ncp=ncp, stats=stats, totals=totals, ms=ms)


def map_update_validate(world, path_off, xyz, edits, mode=1, cfg=synth.PIPELINE_CFG):
    """edits: [(lo, bytes [n0, n1, n2])] -> per round (0: before any edit) both routes' outputs"""
    lib, dp, ip, lp = _lib()
    n, E = len(path_off) - 1, len(edits)
    vox, origin = np.ascontiguousarray(world.voxels), np.ascontiguousarray(world.origin, dtype=np.float64)
    cfg, off, xyz = np.ascontiguousarray(cfg, dtype=np.float64), np.ascontiguousarray(path_off, dtype=np.int32), np.ascontiguousarray(xyz)
    lo = np.ascontiguousarray([e[0] for e in edits], dtype=np.int32).reshape(E, 3)
    en = np.ascontiguousarray([e[1].shape for e in edits], dtype=np.int32).reshape(E, 3)
    eoff = np.concatenate([[0], np.cumsum([e[1].size for e in edits])]).astype(np.int64)
    data = np.ascontiguousarray(np.concatenate([e[1].reshape(-1) for e in edits]), dtype=np.uint8)
    valid, dyn = np.full((E + 1, 2, n), -1, dtype=np.int32), np.full((E + 1, 2, n), -1, dtype=np.int32)
    pos = np.full((E + 1, 2, n, 3), SENTINEL)
    stats, totals = np.zeros((E + 1, 3), dtype=np.int64), np.zeros(3, dtype=np.int64)
    rc = lib.vigo_host_map_update_validate(vox.ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), origin.ctypes.data_as(dp), float(world.res), n,
                                           off.ctypes.data_as(ip), xyz.ctypes.data_as(dp), cfg.ctypes.data_as(dp), E, lo.ctypes.data_as(ip),
                                           en.ctypes.data_as(ip), eoff.ctypes.data_as(lp), data.ctypes.data_as(C.c_void_p), mode,
                                           valid.ctypes.data_as(ip), pos.ctypes.data_as(dp), dyn.ctypes.data_as(ip), stats.ctypes.data_as(lp),
                                           totals.ctypes.data_as(lp))
    assert rc == 0, rc
    return dict(valid=valid, pos=pos, dyn=dyn, stats=stats, totals=totals)


def long_path(world, poses=260, radius=4.0, z=1.0):
    """a pose list that fits more than VIGO_MAX_CTRL_POINTS control points: part of a circle inside the map whose last
    pose is free (updatePath refuses an occupied goal)"""
    for k in range(720):
        a = np.deg2rad(k * 0.5) + np.arange(poses) * (0.09 / radius)
        pts = np.stack([radius * np.cos(a), radius * np.sin(a), np.full(poses, z)], axis=1)
        if synth.lookup(world, pts[-1:], 0)[0] == 0:
            return pts
    raise AssertionError("no free goal on the circle")


def workload(world):
    poses = [POSES[t % len(POSES)] for t in range(N_WORKLOAD)]
    off, xyz = mc.pose_lists(world, poses)
    return off, xyz


def same_routes(r, label):
    assert np.array_equal(r["valid"][..., 0, :], r["valid"][..., 1, :]), f"{label}: the flags differ: {r['valid'].tolist()}"
    assert np.array_equal(r["dyn"][..., 0, :], r["dyn"][..., 1, :]), f"{label}: the dynamic flags differ: {r['dyn'].tolist()}"
    a, b = np.ascontiguousarray(r["pos"][..., 0, :, :]).view(np.int64), np.ascontiguousarray(r["pos"][..., 1, :, :]).view(np.int64)
    assert np.array_equal(a, b), f"{label}: first-collision positions differ at {np.argwhere(a != b)[:4].tolist()}"


def test_the_batch_form_equals_the_per_planner_loop(small_world):
    off, xyz = workload(small_world)
    extra = long_path(small_world)
    off = np.concatenate([off, [off[-1] + len(extra)]]).astype(np.int32)
    xyz = np.concatenate([xyz, extra])
    n = N_WORKLOAD + 1
    # obstacles: every third planner one on its own middle pose (a hit), every third one far away, the others none
    lists = []
    for t in range(n):
        mid = xyz[(off[t] + off[t + 1]) // 2]
        lists.append([[mid[0], mid[1], mid[2], 0, 0, 0, 0.6, 0.6, 1.0]] if t % 3 == 0 else ([[50.0, 50.0, 1.0, 0, 0, 0, 0.6, 0.6, 1.0]] * 2 if t % 3 == 1 else []))
    ooff = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    obs = np.array([o for l in lists for o in l], dtype=np.float64).reshape(-1, 9)
    r = validate_batch(small_world, off, xyz, no_device=NO_DEVICE, not_init=NOT_INIT, obs_off=ooff, obs=obs)
    counts = sorted(set(int(c) for c in r["ncp"][:N_WORKLOAD]) - {0})
    print(f"\n{n} planners, control-point counts {counts} and {int(r['ncp'][-1])}: {int(r['valid'][0].sum())} valid, {int(r['dyn'][0].sum())} inside an obstacle; "
          f"decided / host / groups {r['stats'].tolist()}")
    assert len(counts) >= 10 and r["ncp"][NOT_INIT] == 0 and r["ncp"][-1] > 256
    same_routes(r, "batch form against the loop")
    v = r["valid"][0]
    assert v[NOT_INIT] == 0 and (r["pos"][0, NOT_INIT] == SENTINEL).all()               # not initialised: false, nothing written
    assert 0.2 * n <= v.sum() <= 0.9 * n                                                # both answers occur
    assert ((r["pos"][0] == SENTINEL).all(axis=1) == ((v == 1) | (np.arange(n) == NOT_INIT))).all()   # a position exactly where the answer is false
    # (the planner of 262 points has one too: the dynamic gate takes at most VIGO_MAX_CTRL_POINTS points, false by either route)
    hit = [t for t in range(N_WORKLOAD) if t % 3 == 0 and t not in (NO_DEVICE, NOT_INIT)]
    assert r["dyn"][0][hit].all() and not r["dyn"][0][[t for t in range(n) if t % 3 != 0]].any()
    # one device group for all counts; the planner without a device and the one of more than 256 points took the host route
    assert r["stats"].tolist() == [n - 3, 2, 1] and r["totals"].tolist() == r["stats"].tolist()


def test_a_wall_written_into_the_shared_map_and_removed(small_world):
    off, xyz = workload(small_world)
    first = validate_batch(small_world, off, xyz)
    keep = [t for t in range(N_WORKLOAD) if first["valid"][0, t] == 1]
    assert len(keep) >= 8
    poff = np.concatenate([[0], np.cumsum([off[t + 1] - off[t] for t in keep])]).astype(np.int32)
    pxyz = np.concatenate([xyz[off[t]:off[t + 1]] for t in keep])
    n = len(keep)
    # a 3 x 3 x 3 block of occupied, inflated voxels on the middle pose of three of the longer plans, then the old bytes back
    walled = sorted(range(n), key=lambda k: poff[k] - poff[k + 1])[:3]
    vox = small_world.voxels
    edits, undo = [], []
    for k in walled:
        mid = pxyz[(poff[k] + poff[k + 1]) // 2]
        lo = np.clip(synth.voxel_index(small_world, mid[None])[0] - 1, 0, np.array(vox.shape) - 3)
        edits.append((lo, np.full((3, 3, 3), 5, dtype=np.uint8)))
        undo.append((lo, np.ascontiguousarray(vox[lo[0]:lo[0] + 3, lo[1]:lo[1] + 3, lo[2]:lo[2] + 3])))
    r = map_update_validate(small_world, poff, pxyz, edits + undo[::-1])
    same_routes(r, "after every edit")
    v = r["valid"][:, 0]
    print(f"\n{n} valid plans, walls on {walled}: invalid per round {[np.flatnonzero(x == 0).tolist() for x in v]}; snapshots / region updates / voxels {r['totals'].tolist()}")
    assert v[0].all()
    E = len(walled)
    for e, k in enumerate(walled):
        assert v[e + 1][k] == 0, f"the wall of round {e + 1} lies on plan {k}"
    assert set(walled) <= set(np.flatnonzero(v[E] == 0).tolist())
    assert v[-1].all() and (r["pos"][-1] == SENTINEL).all()                              # after the removal every plan is valid again
    assert (r["stats"][:, 0] == n).all() and (r["stats"][:, 1] == 0).all() and (r["stats"][:, 2] == 1).all()
