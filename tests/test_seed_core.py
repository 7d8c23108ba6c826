"""-m "not gpu": the seed-path stage on the CPU — the host twin of vigo_seed_paths (vigo_seed_paths_host,
csrc/vigo_seed_core.hpp) against the facade's own per-planner steps (getTrajectory, inputPathCheck,
prepareFitPointsWith through vigo_host_seed_steps) bit for bit with libm's power, against itself with the kernels' exact
power, and against the Python restatement of tests/seed_cases.py on the crafted cases."""
import ctypes as C
import math

import numpy as np
import pytest

import seed_cases as sc
from trajectory_planner_amd import _lib

EXACT = lambda t, d: _lib.load().vigo_exact_pow(float(t), int(d))


@pytest.fixture(scope="module")
def workloads():
    """per workload: the world, the polynomials the facade's planners made, the facade's results"""
    out = {}
    for which in ("open", "pillar"):
        world = sc.workload_world(which)
        trajs, steps = sc.facade_steps(world, list(sc.workload_pairs(which)))
        out[which] = (world, trajs, steps)
    return out


def assert_twin_equals_facade(tw, steps, T):
    """the twin's outputs against the facade steps': counts, tries, dt, final_time, prev and the points as uint64"""
    for t in range(T):
        st = tw["status"][t]
        assert st in (sc.OK, sc.NO_SPACING, sc.GOAL_OCCUPIED, sc.TOO_SHORT), (t, st)
        assert bool(steps["found"][t]) == (st != sc.NO_SPACING), t
        assert bool(steps["fit_ok"][t]) == (st == sc.OK), t
        assert bool(steps["fit_wrote"][t]) == (st == sc.OK), t
        for k in ("tries", "seed_n"):
            assert tw[k][t] == steps[k][t], (t, k, tw[k][t], steps[k][t])
        for k in ("dt", "prev_seed", "prev_fit") + (("final_time",) if st != sc.NO_SPACING else ()):
            assert np.float64(tw[k][t]).view(np.uint64) == np.float64(steps[k][t]).view(np.uint64), (t, k, tw[k][t], steps[k][t])
        n = tw["seed_n"][t]
        assert np.array_equal(tw["seed"][t, :n].view(np.uint64), steps["seed"][t, :n].view(np.uint64)), t
        if st == sc.OK:
            m = tw["fit_n"][t]
            assert m == steps["fit_n"][t], t
            assert np.array_equal(tw["fit"][t, :m].view(np.uint64), steps["fit"][t, :m].view(np.uint64)), t


@pytest.mark.parametrize("which", ["open", "pillar"])
def test_twin_with_libm_equals_the_facade_steps_on_the_workloads(workloads, which):
    world, trajs, steps = workloads[which]
    rc, tw = sc.twin(world, sc.pack(trajs), 1, max_tries=16)
    assert rc == 0
    assert_twin_equals_facade(tw, steps, len(trajs))
    assert (tw["status"] != sc.DEFERRED).all()                  # the shipped capacity holds the workloads (a condition)
    assert (tw["status"] == sc.OK).sum() >= 48 and (tw["seed_n"][tw["status"] == sc.OK] >= 4).all()
    if which == "open":
        assert (tw["status"] == sc.OK).all()


def test_twin_with_libm_equals_the_facade_steps_on_the_waypoint_cases():
    world = sc.craft_world()
    seen = set()
    for name, wps, max_len, prev_seed, prev_fit in sc.waypoint_cases():
        trajs, steps = sc.facade_steps(world, [wps], max_len=max_len, prev_seed=[prev_seed], prev_fit=[prev_fit])
        rc, tw = sc.twin(world, sc.pack(trajs), 1, max_tries=16)
        assert rc == 0, name
        assert_twin_equals_facade(tw, steps, 1)
        seen.add((int(tw["status"][0]), min(int(tw["seed_n"][0]), 4)))
    assert {(sc.OK, 2), (sc.OK, 3), (sc.OK, 4), (sc.GOAL_OCCUPIED, 4)} <= seen, seen


@pytest.mark.parametrize("which", ["open", "pillar"])
def test_exact_power_changes_no_integer_and_points_within_the_bound(workloads, which):
    world, trajs, _ = workloads[which]
    a = sc.pack(trajs)
    (rc1, m1), (rc0, m0) = sc.twin(world, a, 1, max_tries=16), sc.twin(world, a, 0, max_tries=16)
    assert rc0 == 0 and rc1 == 0
    for k in ("status", "tries", "seed_n", "fit_n"):
        assert np.array_equal(m0[k], m1[k]), k
    assert np.array_equal(m0["dt"], m1["dt"])
    checked = 0
    for t, c in enumerate(trajs):
        # every seed pose is the sample at one t_j of the last try's clock: its bound is that sample's own
        n, m = m1["seed_n"][t], m1["fit_n"][t]
        seed_b = sc.point_bounds(c, float(m1["dt"][t]), m1["seed"][t, :n])
        assert (np.abs(m0["seed"][t, :n] - m1["seed"][t, :n]) <= seed_b).all(), t
        assert (np.abs(m0["fit"][t, :m] - m1["fit"][t, :m]) <= sc.fit_bounds(seed_b, m)).all(), t
        checked += n + m
    assert checked > 1000


def test_exact_power_within_the_bound_on_the_filled_waypoint_cases():
    """the fillPath branches (seeds of 2 and 3 poses): the filled points against their parents' bounds"""
    world = sc.craft_world()
    filled = 0
    for name, wps, max_len, prev_seed, prev_fit in sc.waypoint_cases():
        trajs, _ = sc.facade_steps(world, [wps], max_len=max_len, prev_seed=[prev_seed], prev_fit=[prev_fit])
        a = sc.pack(trajs)
        (_, m1), (_, m0) = sc.twin(world, a, 1, max_tries=16), sc.twin(world, a, 0, max_tries=16)
        for k in ("status", "tries", "seed_n", "fit_n"):
            assert np.array_equal(m0[k], m1[k]), (name, k)
        n, m = m1["seed_n"][0], m1["fit_n"][0]
        seed_b = sc.point_bounds(trajs[0], float(m1["dt"][0]), m1["seed"][0, :n])
        assert (np.abs(m0["seed"][0, :n] - m1["seed"][0, :n]) <= seed_b).all(), name
        assert (np.abs(m0["fit"][0, :m] - m1["fit"][0, :m]) <= sc.fit_bounds(seed_b, m)).all(), name
        filled += int(m > n)
    assert filled >= 2


def test_margins_hold_on_the_workloads(workloads):
    for which, (world, trajs, _) in workloads.items():
        log = []
        for c in trajs:
            sc.restate(world, c, max_tries=16, log=log)
        assert len(log) > 1000
        sc.check_margins(log)


@pytest.fixture(scope="module")
def crafted():
    return sc.crafted()


def test_margins_hold_on_the_crafted_cases(crafted):
    world = sc.craft_world()
    for name, c in crafted.items():
        log = []
        sc.restate(world, c, log=log)
        sc.check_margins(log)


@pytest.mark.parametrize("pow_mode", [0, 1])
def test_twin_equals_the_python_restatement_on_the_crafted_cases(crafted, pow_mode):
    world = sc.craft_world()
    power = EXACT if pow_mode == 0 else math.pow
    for name, c in crafted.items():
        want = sc.restate(world, c, power=power)
        for k, v in c.expect.items():                       # the case does what it was crafted for
            assert want[k] == v, (name, k, want[k], v)
        rc, tw = sc.twin(world, sc.pack([c]), pow_mode)
        assert rc == 0, name
        sc.assert_row(tw, 0, want, name)


def test_capacity_and_mixed_launch(crafted):
    world = sc.craft_world()
    cap = sc.capacity()
    assert cap >= 1024
    for pow_mode in (0, 1):
        rc, tw = sc.twin(world, sc.pack([crafted[f"samples_{cap}"], crafted["capacity_plus_1"]]), pow_mode)
        assert rc == 0 and list(tw["status"]) == [sc.OK, sc.DEFERRED]
    # a smaller capacity defers what a larger one runs
    rc, tw = sc.twin(world, sc.pack([crafted["samples_64"], crafted["samples_65"]]), 0, cap=64)
    assert rc == 0 and list(tw["status"]) == [sc.OK, sc.DEFERRED]
    # T = 65, every case in one call: each row is what the case gives alone
    names = list(crafted)
    trajs = [crafted[names[i % len(names)]] for i in range(65)]
    rc, tw = sc.twin(world, sc.pack(trajs), 0)
    assert rc == 0
    for t, c in enumerate(trajs):
        sc.assert_row(tw, t, sc.restate(world, c, power=EXACT), c.name)
    # point_cap below a list's length defers it
    rc, tw = sc.twin(world, sc.pack([crafted["past_max_length"]]), 0, point_cap=10)
    assert rc == 0 and tw["status"][0] == sc.DEFERRED
    # T = 0 and the hostile arguments: nothing is written
    rc, tw = sc.twin(world, sc.pack([]), 0)
    assert rc == 0
    a = sc.pack([crafted["one_try"]])
    for bad in (dict(max_tries=0), dict(point_cap=-1), dict(cap=0, pow_mode=2)):
        rc, tw = sc.twin(world, a, bad.pop("pow_mode", 0), **bad)
        assert rc == -1
        assert tw["status"][0] == sc.SENTINEL_I and np.all(tw["seed"] == sc.SENTINEL_D)
    bad_off = dict(a, seg_off=np.array([0, 5], np.int32))        # offsets outside [0, S]: that trajectory's status
    rc, tw = sc.twin(world, bad_off, 0)
    assert rc == 0 and tw["status"][0] == sc.BAD_INPUT and tw["seed_n"][0] == 0
