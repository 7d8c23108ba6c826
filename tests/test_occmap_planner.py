"""CPU: trajPlanner::polyTrajOccMap's solo makePlan (host QP, host sampling, the map's own lookups) through
vigo_host_occ_plan, against a Python restatement of the reference loop (polyTrajOccMap.cpp:326-399, :524-552): the QP
of each round from vigo_host_minsnap_full, samples at t += delT in PS.cpp:1026-1056's expression order, the
inflated-occupied AND unknown rule as a numpy lookup.  Pins the reference's quirks: the AND rule, the soft radius
1.0 / 1.0 / 0, updateDesiredAcc without effect, maximum_iteration_num + 1 solves, the one-waypoint path, makePlan(false)
without any check, makePlan(trajectory) with corridors, the PWL duration; getTrajectory(dt) against the t <= duration
loop."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
_dp = C.POINTER(C.c_double)
CAP = 4096
NAN = float("nan")
KEYS = ["polynomial_degree", "differential_degree", "continuity_degree", "desired_velocity", "desired_acceleration",
        "initial_radius", "timeout", "corridor_res", "shrinking_factor", "soft_constraint", "constraint_radius",
        "sample_delta_time", "maximum_iteration_num", "use_pwl_failsafe", "update_vel", "update_acc"]
DEFAULTS = dict(polynomial_degree=7, differential_degree=4, continuity_degree=4, desired_velocity=1.0,
                desired_acceleration=1.0, initial_radius=0.5, timeout=0.1, corridor_res=5.0, shrinking_factor=0.8,
                soft_constraint=0, constraint_radius=0.5, sample_delta_time=0.1, maximum_iteration_num=20,
                use_pwl_failsafe=0)
ORIGIN = np.array([-3.0, -3.0, 0.0])
RES = 0.1


def lib():
    L = C.CDLL(LIB)
    L.vigo_host_occ_plan.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int,
                                     C.c_int, _dp, C.c_double, _dp, _dp]
    L.vigo_host_minsnap_full.argtypes = [C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_double, _dp, C.c_double, _dp, _dp, _dp, _dp]
    L.vigo_host_pwl.argtypes = [C.c_int, _dp, C.c_int, C.c_double, C.c_double, _dp, C.c_int, _dp, C.POINTER(C.c_int)]
    return L


def P(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(_dp)


def cfg_vec(**kw):
    """NaN = key not set; timeout 100 s unless given: the loop is bounded by the iteration limit, not the clock"""
    c = {"timeout": 100.0, **kw}
    return np.array([float(c.get(k, NAN)) for k in KEYS], dtype=np.float64)


def plan(vox, wp, mode=1, conds=None, gt_dt=0.0, **kw):
    L = lib()
    v = np.ascontiguousarray(vox, dtype=np.uint8)
    wp = np.ascontiguousarray(wp, dtype=np.float64)
    cf = cfg_vec(**kw)
    tr, gt, info = np.zeros((CAP, 3)), np.zeros((CAP, 3)), np.zeros(8)
    cd = None if conds is None else np.ascontiguousarray(conds, dtype=np.float64)
    rc = L.vigo_host_occ_plan(*v.shape, P(ORIGIN), RES, v.ctypes.data_as(C.c_void_p), len(wp), P(wp), P(cf), P(cd), mode, CAP,
                              tr.ctypes.data_as(_dp), gt_dt, gt.ctypes.data_as(_dp), info.ctypes.data_as(_dp))
    assert rc == 0
    n, ng = int(info[2]), int(info[5])
    return dict(valid=bool(info[0]), iters=int(info[1]), traj=tr[:n], duration=info[3], gt=gt[:ng], end=info[6:8])


# ---- the restatement ----
def lookup_collides(vox, p):
    """isInflatedOccupied(p) && isUnknown(p): bits 0 and 1 of voxel floor((p - origin) / res); outside: every bit set"""
    idx = [math.floor((p[a] - ORIGIN[a]) / RES) if math.isfinite(p[a]) else -1 for a in range(3)]
    if any(i < 0 or i >= n for i, n in zip(idx, vox.shape)):
        return True
    return (int(vox[idx[0], idx[1], idx[2]]) & 3) == 3


def qp(wp, deg, diff, cont, vel, corridor, cres, soft, conds):
    K = len(wp) - 1
    co, kn = np.zeros(3 * K * (deg + 1)), np.zeros(K + 1)
    rc = lib().vigo_host_minsnap_full(len(wp), P(wp), deg, diff, cont, vel, P(corridor), cres, P(soft), P(conds),
                                      co.ctypes.data_as(_dp), kn.ctypes.data_as(_dp))
    return co.reshape(3, K * (deg + 1)), rc, [float(x) for x in kn]


def pos(co, kn, deg, t):
    """PS.cpp:1026-1056: the first interval holding t, x += c[d] * pow(t - k[i], d) ascending; default pose elsewhere"""
    for i in range(len(kn) - 1):
        if kn[i] <= t <= kn[i + 1]:
            tt = t - kn[i]
            c0 = (deg + 1) * i
            x = y = z = 0.0
            for d in range(deg + 1):
                x += float(co[0][c0 + d]) * math.pow(tt, d)
                y += float(co[1][c0 + d]) * math.pow(tt, d)
                z += float(co[2][c0 + d]) * math.pow(tt, d)
            return (x, y, z)
    return (0.0, 0.0, 0.0)


def sample(co, kn, deg, delT, last):
    out, t = [], 0.0
    while t < kn[-1]:
        out.append(pos(co, kn, deg, t))
        t += delT
    out.append(tuple(last))
    return out


def restate(vox, wp, corridor=True, conds=None, **kw):
    c = {**DEFAULTS, **kw}
    deg, diff, cont = int(c["polynomial_degree"]), int(c["differential_degree"]), int(c["continuity_degree"])
    vel = float(c["desired_velocity"]) if "update_vel" not in kw else float(kw["update_vel"])
    K = len(wp) - 1
    corr = [float(c["initial_radius"])] * K
    soft = np.array([1.0, 1.0, 0.0]) if c["soft_constraint"] else None   # PM.cpp:357-358: the bool as the radius
    delT, fs, max_iter = float(c["sample_delta_time"]), float(c["shrinking_factor"]), int(c["maximum_iteration_num"])
    wp = np.asarray(wp, np.float64)
    prev, iters, valid, traj, kn, rounds = None, 0, False, [], None, []
    while True:
        rounds.append(list(corr))
        co, mask, kn = qp(wp, deg, diff, cont, vel, np.array(corr) if corridor else None, float(c["corridor_res"]),
                          soft if corridor else None, conds)
        if prev is not None:                                 # an axis whose QP fails keeps its previous polynomial
            co = np.where(np.array([(mask >> a) & 1 for a in range(3)], bool)[:, None], co, prev)
        elif mask != 7:                                      # no polynomial to sample: not found
            break
        prev = co
        traj = sample(co, kn, deg, delT, wp[-1])
        iters += 1
        if not corridor:
            valid = True
            break
        t, hit, segs = 0.0, False, set()
        for p in traj:                                       # PM.cpp:524-546
            if lookup_collides(vox, p):
                hit = True
                s = next((i for i in range(K) if kn[i] <= t <= kn[i + 1]), -1)
                if s >= 0:
                    segs.add(s)
            t += delT
        if not hit:
            valid = True
            break
        for s in segs:
            corr[s] = corr[s] * fs
        if iters > max_iter:
            break
    return dict(valid=valid, iters=iters, traj=np.array(traj), co=prev, kn=kn, deg=deg, rounds=rounds[:iters])


def restated_get_trajectory(r, dt):
    """PM.cpp:434-446 over getPos's clamp to the duration"""
    dur = r["kn"][-1]
    out, t = [], 0.0
    while t <= dur:
        out.append(pos(r["co"], r["kn"], r["deg"], min(t, dur)))
        t += dt
    return np.array(out)


def assert_same(got, ref):
    assert got["valid"] == ref["valid"] and got["iters"] == ref["iters"], (got["valid"], got["iters"], ref["valid"], ref["iters"])
    assert got["traj"].shape == ref["traj"].shape
    np.testing.assert_allclose(got["traj"], ref["traj"], rtol=0, atol=1e-9)


def world(fill=None):
    """60 x 60 x 20 voxels of 0.1 m from (-3, -3, 0); fill: [(slices, bits)]"""
    vox = np.zeros((60, 60, 20), np.uint8)
    for sl, bits in fill or []:
        vox[sl] |= bits
    return vox


WP = np.array([[-2.0, -1.0, 1.0], [0.5, 0.9, 1.0], [2.0, -0.6, 1.0]])
BLOCK = (slice(21, 25), slice(29, 33), slice(0, 20))   # x in [-0.9, -0.5), y in [-0.1, 0.3): on the first leg


@pytest.mark.parametrize("bits", [1, 2, 3])
def test_and_rule(bits):
    vox = world([(BLOCK, bits)])
    got = plan(vox, WP)
    assert_same(got, restate(vox, WP))
    if bits == 3:
        assert got["iters"] > 1                      # both bits: samples collide
    else:
        assert got["valid"] and got["iters"] == 1    # one bit alone: no collision


def test_leaving_the_grid_collides_and_exhausts_the_iterations():
    wp = np.array([[-2.0, 0.0, 1.0], [3.5, 0.0, 1.0]])         # the goal lies beyond the grid: every round collides
    for max_iter in (0, 3):
        got = plan(world(), wp, maximum_iteration_num=max_iter)
        assert_same(got, restate(world(), wp, maximum_iteration_num=max_iter))
        assert not got["valid"] and got["iters"] == max_iter + 1


def test_random_worlds_and_conditions():
    rng = np.random.default_rng(5)
    seen = set()
    for trial in range(10):
        vox = world()
        for _ in range(12):
            c = rng.integers(5, 55, size=2)
            vox[c[0] - 2:c[0] + 2, c[1] - 2:c[1] + 2, :] |= int(rng.integers(1, 4))
        W = int(rng.integers(2, 6))
        wp = np.column_stack([np.linspace(-2.5, 2.5, W), rng.uniform(-2, 2, W), rng.uniform(0.5, 1.5, W)])
        conds = rng.uniform(-0.3, 0.3, size=(4, 3)) if trial % 2 else None
        kw = dict(maximum_iteration_num=int(rng.integers(1, 8)), shrinking_factor=0.7)
        got = plan(vox, wp, conds=conds, **kw)
        assert_same(got, restate(vox, wp, conds=conds, **kw))
        seen.add((got["valid"], got["iters"] > 1))
    assert len(seen) >= 2


def test_soft_constraint_radius_is_the_bool():
    vox = world([(BLOCK, 3)])
    wp = np.array([[-2.0, -1.0, 1.0], [-0.5, 0.5, 1.2], [0.5, -0.9, 0.8], [2.0, -0.6, 1.0]])
    got = plan(vox, wp, soft_constraint=1, constraint_radius=0.25)
    ref = restate(vox, wp, soft_constraint=1)
    assert_same(got, ref)
    hard = restate(vox, wp)
    assert hard["traj"].shape != ref["traj"].shape or np.abs(hard["traj"] - ref["traj"]).max() > 1e-6


def test_update_desired_acc_has_no_effect_vel_has():
    base = plan(world(), WP)
    acc = plan(world(), WP, update_acc=5.0)
    assert_same(acc, base)
    assert acc["duration"] == base["duration"]
    vel = plan(world(), WP, update_vel=2.0)
    assert vel["duration"] < base["duration"]
    assert_same(vel, restate(world(), WP, update_vel=2.0))


def test_one_waypoint_path():
    wp = np.array([[0.5, 0.5, 1.0]])
    got = plan(world(), wp, gt_dt=0.1)
    assert got["valid"] and got["iters"] == 0 and got["duration"] == 0.0
    np.testing.assert_array_equal(got["traj"], wp)
    assert len(got["gt"]) == 1                                 # t = 0 <= 0: one pose (no solver: zero, no crash)


def test_make_plan_false_does_no_check():
    vox = world([((slice(None), slice(None), slice(None)), 3)])   # every voxel inflated-occupied and unknown
    got = plan(vox, WP, mode=0)
    ref = restate(vox, WP, corridor=False)
    assert_same(got, ref)
    assert got["valid"] and got["iters"] == 1
    assert any(lookup_collides(vox, p) for p in got["traj"])  # it collides, and nobody looked


def test_make_plan_without_bool_uses_corridors():
    vox = world([(BLOCK, 3)])
    a, b = plan(vox, WP, mode=2), plan(vox, WP, mode=1)
    assert_same(a, b)
    assert a["iters"] > 1


@pytest.mark.parametrize("dt", [0.1, 0.07, 0.25])
def test_get_trajectory_is_the_t_le_duration_loop(dt):
    vox = world([(BLOCK, 3)])
    got = plan(vox, WP, gt_dt=dt)
    ref = restate(vox, WP)
    exp = restated_get_trajectory(ref, dt)
    assert got["gt"].shape == exp.shape
    np.testing.assert_allclose(got["gt"], exp, rtol=0, atol=1e-9)
    assert got["duration"] == ref["kn"][-1]


def test_pwl_failsafe_duration():
    wp = np.array([[-2.0, 0.0, 1.0], [3.5, 0.0, 1.0]])         # never valid
    got = plan(world(), wp, use_pwl_failsafe=1, maximum_iteration_num=1, gt_dt=0.1)
    assert not got["valid"]
    w4 = np.ascontiguousarray(np.column_stack([wp, np.zeros(2)]))
    tr, kn, nk = np.zeros((CAP, 4)), np.zeros(8), C.c_int()
    n = lib().vigo_host_pwl(2, P(w4), 0, 0.0, 0.1, tr.ctypes.data_as(_dp), CAP, kn.ctypes.data_as(_dp), C.byref(nk))
    assert n > 0
    assert got["duration"] == kn[nk.value - 1]                 # the PWL's last knot ...
    np.testing.assert_allclose(got["traj"], tr[:n, :3], rtol=0, atol=1e-12)   # ... and its trajectory
    ref = restate(world(), wp, maximum_iteration_num=1)
    # ... while getTrajectory(dt) still samples the polynomial (default pose past its own knots) up to that duration
    dur, out, t = got["duration"], [], 0.0
    while t <= dur:
        out.append(pos(ref["co"], ref["kn"], ref["deg"], min(t, dur)))
        t += 0.1
    np.testing.assert_allclose(got["gt"], np.array(out), rtol=0, atol=1e-9)
