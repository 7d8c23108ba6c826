"""-m gpu: bsplineTraj::makePlanBatch(planners, trajectories, yaw) under setDeviceEpilogue through
vigo_host_plan_batch, on the 48-planner, ten-count workload of tests/test_gpu_mixed_facade.py.  With the switch on,
steps 5-6 and the sampled paths of every planner that planned come from ONE vigo_traj_finish call for all ten counts;
each planner must end with what the host epilogue and evalTrajToMsg give it — ok flag, linearFactor_, pose count,
positions and quaternions bit for bit.  One planner has no device, one has a sample step so small that its path
exceeds the capacity the facade sizes: both take the host route, with the same result."""
import numpy as np
import pytest

import finish_cases as fc
import mixed_cases as mc
from test_gpu_mixed_facade import POSES

pytestmark = pytest.mark.gpu
NO_DEVICE, SMALL_STEP, STEP = 5, 0, 4e-4      # planner 0's path is the shortest: at 4e-4 it still has more samples than the 2048 the facade sizes


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(r, label):
    for k in ("ok", "n_poses"):
        assert np.array_equal(r[k][0], r[k][1]), f"{label}: {k} differs: {r[k][0].tolist()} / {r[k][1].tolist()}"
    planned = r["ok"][0] != 0
    for k in ("factor", "pos", "quat"):
        same = bits(r[k][0][planned]) == bits(r[k][1][planned])
        assert same.all(), f"{label}: {k} differs at {np.argwhere(~same)[:4].tolist()}"


@pytest.fixture(scope="module")
def workload(small_world):
    poses = [POSES[t % len(POSES)] for t in range(48)]
    return mc.pose_lists(small_world, poses)


def test_device_epilogue_gives_every_planner_the_same_factor_and_path(small_world, workload):
    off, xyz = workload
    r = fc.plan_batch_finish(small_world, off, xyz, no_device=NO_DEVICE, small_step=SMALL_STEP, step=STEP, pose_cap=2600)
    ok = r["ok"][0]
    print(f"\n48 planners: {int(ok.sum())} planned; totals (device-decided, host route, device groups) off {r['totals'][0].tolist()}, "
          f"on {r['totals'][1].tolist()}; {r['total_ms'][0, 0]:.1f} ms off, {r['total_ms'][1, 0]:.1f} ms on; "
          f"the small-step planner has {int(r['n_poses'][0][SMALL_STEP])} poses")
    _same(r, "setDeviceEpilogue(true) against (false)")
    assert ok[NO_DEVICE] == 0 and r["n_poses"][0][NO_DEVICE] == 0            # no device: no plan, an empty path
    assert (r["n_poses"][0][ok == 0] == 0).all()
    others = np.array([t for t in range(48) if t not in (NO_DEVICE, SMALL_STEP)])
    assert ok[others].sum() >= 24
    assert len(set(r["n_poses"][0][others][ok[others] != 0].tolist())) >= 6   # the counts differ inside the one group
    assert ok[SMALL_STEP] == 1 and r["n_poses"][0][SMALL_STEP] > 2048
    assert r["totals"][0].tolist() == [0, 0, 0]
    # one device group for all the counts, one for the planner of the other step, whose row is over capacity
    assert r["totals"][1].tolist() == [int(ok[others].sum()), 1, 2]
    assert r["switches"] == 0


def test_factor_alone_and_without_yaw(small_world, workload):
    off, xyz = workload
    r = fc.plan_batch_finish(small_world, off, xyz, with_paths=False)
    _same(r, "makePlanBatch(planners)")
    assert (r["n_poses"] == 0).all() and r["totals"][1].tolist() == [int(r["ok"][0].sum()), 0, 1]
    r = fc.plan_batch_finish(small_world, off, xyz, yaw=False)
    _same(r, "yaw = false")
    planned = r["ok"][0] != 0
    assert (r["n_poses"][0][planned] > 0).all() and r["switches"] == 0
