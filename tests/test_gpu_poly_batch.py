"""-m gpu: polyTrajOctomap::makePlanBatch (whole trajectories checked by vigo_traj_corridor_check) against each planner's
twin planned alone with makePlan() (host sampling, vigo_box_collision_points, the collisionSegments rule), through
vigo_host_poly_plan_batch_ex: on the maze fixture and on seeded pillar worlds, 32 planners mixing both modes and a path of
more than 11 waypoints (host QP); the reference's shipped degrees (continuity 3, jerk); path shapes the device QP refuses
(continuity 2 at 11 waypoints) and corridors of more than its 1024 boxes, which the batch solves on the host as its solo
twin does.  Every sample of a valid trajectory is re-checked with a numpy box sweep."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
CAP = 4096


def numpy_box_sweep(vox, origin, res, pts, box, step):
    """PO.cpp:547-589 restated: float coordinates, floor(coord * (1/res)) keys, unknown or outside the grid => occupied"""
    nx, ny, nz = vox.shape
    key0 = np.round(origin / res).astype(np.int64)
    p = pts.astype(np.float32).astype(np.float64)
    hit = np.zeros(len(pts), dtype=bool)
    lo = p - np.asarray(box) / 2
    num = ((p + np.asarray(box) / 2) - lo) / step
    n_max = [int(num[:, a].max()) if len(p) else 0 for a in range(3)]
    for i in range(n_max[0] + 1):
        for j in range(n_max[1] + 1):
            for k in range(n_max[2] + 1):
                use = (i <= num[:, 0].astype(np.int64)) & (j <= num[:, 1].astype(np.int64)) & (k <= num[:, 2].astype(np.int64))
                q = np.stack([lo[:, 0] + i * step, lo[:, 1] + j * step, lo[:, 2] + k * step], 1).astype(np.float32)
                idx = np.floor(q.astype(np.float64) * (1.0 / res)).astype(np.int64) - key0
                out = (idx < 0).any(1) | (idx[:, 0] >= nx) | (idx[:, 1] >= ny) | (idx[:, 2] >= nz)
                ic = np.clip(idx, 0, [nx - 1, ny - 1, nz - 1])
                hit |= use & (out | ((vox[ic[:, 0], ic[:, 1], ic[:, 2]] & 6) != 0))
    return hit


def plan_batch(vox, origin, res, paths, modes, cfg, diff=4, cont=4):
    L = C.CDLL(LIB)
    L.vigo_host_poly_plan_batch_ex.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _ip, _dp, _dp,
                                               _ip, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]
    P = len(paths)
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
    wp = np.ascontiguousarray(np.concatenate(paths), dtype=np.float64)
    md = np.asarray(modes, dtype=np.int32)
    cf = np.asarray(cfg, dtype=np.float64)
    v = np.ascontiguousarray(vox)
    org = np.ascontiguousarray(origin, dtype=np.float64)
    tr, info = np.zeros((P, CAP, 3)), np.zeros((P, 4))
    str_, sinfo = np.zeros((P, CAP, 3)), np.zeros((P, 4))
    secs = np.zeros(2)
    rc = L.vigo_host_poly_plan_batch_ex(vox.shape[0], vox.shape[1], vox.shape[2], org.ctypes.data_as(_dp), res,
                                        v.ctypes.data_as(C.c_void_p), P, off.ctypes.data_as(_ip), wp.ctypes.data_as(_dp),
                                        cf.ctypes.data_as(_dp), md.ctypes.data_as(_ip), diff, cont, CAP, tr.ctypes.data_as(_dp),
                                        info.ctypes.data_as(_dp), str_.ctypes.data_as(_dp), sinfo.ctypes.data_as(_dp),
                                        secs.ctypes.data_as(_dp))
    assert rc == 0
    return tr, info, str_, sinfo, secs


def maze():
    f = np.load(os.path.join(ROOT, "tests", "golden", "maze_config1.npz"))
    nx, ny, nz = (int(v) for v in f["dims"])
    n = nx * ny * nz
    occ = np.unpackbits(f["occ_bits"])[:n].reshape(nx, ny, nz)
    unk = np.unpackbits(f["unk_bits"])[:n].reshape(nx, ny, nz)
    return (occ * 5 + unk * 2).astype(np.uint8), f["origin"].astype(np.float64), float(f["res"][0]), f["waypoints"].astype(np.float64)


def pillar_world(seed):
    rng = np.random.default_rng(seed)
    vox = np.zeros((128, 128, 40), dtype=np.uint8)
    for _ in range(25):
        c = rng.integers(10, 118, size=2)
        s = rng.integers(1, 4, size=2)
        vox[c[0] - s[0]:c[0] + s[0] + 1, c[1] - s[1]:c[1] + s[1] + 1, :] |= 5
    return vox, np.array([-6.4, -6.4, -0.5]), 0.1


def random_paths(rng, P, lo, hi, long_every=16):
    out = []
    for i in range(P):
        W = 13 if i % long_every == 5 else int(rng.integers(4, 9))
        a, b = rng.uniform(lo, hi, size=(2, 3))
        f = np.linspace(0, 1, W)[:, None]
        p = a + f * (b - a)
        p[1:-1] += rng.normal(0, 0.15, size=(W - 2, 3)) * [1, 1, 0.3]
        out.append(p)
    return out


# box, map_resolution, delT, vel, r0, fs, corridor_res, max iterations (5: adding-waypoint paths can double per round),
# timeout (large: the verdict must not depend on the wall clock), mode (replaced per planner)
CFG = [0.4, 0.4, 0.2, 0.2, 0.1, 1.0, 0.5, 0.8, 8.0, 5, 100.0, 0.0]


def check(vox, origin, res, paths, modes, cfg=CFG, diff=4, cont=4):
    tr, info, str_, sinfo, secs = plan_batch(vox, origin, res, paths, modes, cfg, diff, cont)
    assert np.array_equal(info[:, :3], sinfo[:, :3]), np.nonzero((info[:, :3] != sinfo[:, :3]).any(1))[0]
    assert np.array_equal(info[:, 3], sinfo[:, 3])
    for i in range(len(paths)):
        n = min(int(info[i, 3]), CAP)
        assert np.abs(tr[i, :n] - str_[i, :n]).max(initial=0.0) <= 1e-9, i
        if info[i, 0]:
            hits = numpy_box_sweep(vox, origin, res, tr[i, :n], cfg[:3], cfg[3])
            assert not hits.any(), (i, int(hits.sum()))
    return info, secs


def test_batch_equals_solo_on_the_maze():
    vox, origin, res, wp = maze()
    rng = np.random.default_rng(21)
    paths = [wp] + [wp + np.concatenate([np.zeros((1, 3)), rng.normal(0, 0.1, size=(len(wp) - 2, 3)) * [1, 1, 0.2],
                                         np.zeros((1, 3))]) for _ in range(30)]
    long_path = np.concatenate([wp[:1], np.linspace(wp[0], wp[-1], 12)[1:-1], wp[-1:]])   # 12 waypoints
    long_path = np.concatenate([long_path[:6], (long_path[5:6] + long_path[6:7]) / 2, long_path[6:]])   # 13: host QP
    paths.append(long_path)
    modes = [i % 2 for i in range(len(paths))]
    info, secs = check(vox, origin, res, paths, modes)
    assert info[:, 0].any()
    print(f"maze: {int(info[:, 0].sum())}/32 valid; batch {secs[0] * 1e3:.1f} ms, solo {secs[1] * 1e3:.1f} ms")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_batch_equals_solo_on_pillar_worlds(seed):
    vox, origin, res = pillar_world(seed)
    rng = np.random.default_rng(100 + seed)
    paths = random_paths(rng, 32, [-5, -5, 0.8], [5, 5, 1.6])
    modes = list(rng.integers(0, 2, size=32))
    info, secs = check(vox, origin, res, paths, modes)
    assert 0 < info[:, 0].sum() and (info[:, 1] > 1).any()     # some valid plans, some that took more than one round
    assert (info[:, 2] > 11).any()                              # a path of more than 11 waypoints (host QP) took part


def test_reference_degrees_on_the_maze():
    """cfg/planner.yaml ships continuity_degree 3; differential_degree 3 (jerk) is its other documented choice"""
    vox, origin, res, wp = maze()
    rng = np.random.default_rng(22)
    paths = [wp] + [wp + np.concatenate([np.zeros((1, 3)), rng.normal(0, 0.1, size=(len(wp) - 2, 3)) * [1, 1, 0.2],
                                         np.zeros((1, 3))]) for _ in range(15)]
    info, _ = check(vox, origin, res, paths, [i % 2 for i in range(16)], diff=3, cont=3)
    assert info[:, 0].any()


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_degrees_on_pillar_worlds(seed):
    vox, origin, res = pillar_world(seed)
    rng = np.random.default_rng(200 + seed)
    paths = random_paths(rng, 16, [-5, -5, 0.8], [5, 5, 1.6], long_every=8)
    modes = list(rng.integers(0, 2, size=16))
    info, _ = check(vox, origin, res, paths, modes, diff=3, cont=3)
    assert 0 < info[:, 0].sum() and (info[:, 1] > 1).any()


def test_shapes_the_device_qp_refuses_are_solved_on_the_host():
    """continuity 2 at 11 waypoints needs 179 KiB of LDS: vigo_minsnap refuses it (vigo_minsnap_supported), and the
    batch must solve such a group on the host instead of giving up on every planner"""
    from trajectory_planner_amd import _lib
    assert not _lib.load().vigo_minsnap_supported(11, 7, 4, 2) and _lib.load().vigo_minsnap_supported(10, 7, 4, 2)
    vox, origin, res = pillar_world(4)
    rng = np.random.default_rng(44)
    paths = []
    for i in range(12):
        W = 11 if i < 6 else int(rng.integers(4, 9))
        a, b = rng.uniform([-5, -5, 0.8], [5, 5, 1.6], size=(2, 3))
        p = a + np.linspace(0, 1, W)[:, None] * (b - a)
        p[1:-1] += rng.normal(0, 0.15, size=(W - 2, 3)) * [1, 1, 0.3]
        paths.append(p)
    modes = [i % 2 for i in range(12)]                        # 11-waypoint paths in both modes
    info, _ = check(vox, origin, res, paths, modes, cont=2)
    assert info[:, 0].any() and (info[:, 1] >= 1).all()


def spiral(W, r, step_deg, a0=0.0):
    a = np.deg2rad(a0 + np.arange(W) * step_deg)
    return np.stack([r * np.cos(a), r * np.sin(a), np.linspace(0.9, 1.5, W)], 1)


def test_more_than_1024_corridor_boxes_are_solved_on_the_host():
    """at desired_velocity 0.25 a 38 m path of 11 waypoints has ~1200 corridor boxes: the device QP reports -1 (kMaxBox,
    pinned in tests/test_gpu_minsnap_params.py), the host QP has no such limit, and the batch must solve that planner on
    the host in the same round, as its solo twin does.  A planner whose first corridor is infeasible (device status -2:
    a zig-zag of 10 m legs) keeps today's behaviour: no polynomial, the fallback -- as alone."""
    from minsnap_ref import corridor_rows, minsnap_matrices
    from test_minsnap_params import host_solve
    cfg = list(CFG)
    cfg[5] = 0.25                                             # desired_velocity
    vox, origin, res = pillar_world(5)
    big = [spiral(11, 5.5, 40), spiral(11, 5.0, 40, 15)]
    zigzag = np.array([[-5.0, -4.0, 1.2], [5.0, -2.0, 1.2], [-5.0, 0.0, 1.2]])
    rng = np.random.default_rng(55)
    paths = big + [zigzag] + random_paths(rng, 8, [-5, -5, 0.8], [5, 5, 1.6], long_every=100)
    modes = [0, 0, 0] + [i % 2 for i in range(8)]
    # the premises: the spirals have more boxes than the device QP takes and a feasible first corridor; the zig-zag's
    # first corridor is infeasible (with fewer than 1024 boxes)
    for p, feasible in ((big[0], True), (big[1], True), (zigzag, False)):
        cor = np.full(len(p) - 1, cfg[6])
        _, _, _, Tk = minsnap_matrices(p, 7, 4, 4, cfg[5])
        assert (len(corridor_rows(p, Tk, cor, cfg[8])[0]) > 1024) == feasible
        assert (host_solve(p, 4, 4, cfg[5], None, cor, cfg[8])[0] == 0) == feasible
    info, _ = check(vox, origin, res, paths, modes, cfg=cfg)
    assert (info[:2, 1] >= 1).all()                           # the spirals were planned, not dropped in round 1
    assert info[2, 0] == 0 and info[2, 1] == 0                # the infeasible zig-zag: no polynomial, like its solo twin
