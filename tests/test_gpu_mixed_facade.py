"""-m gpu: bsplineTraj::makePlanBatch under setMixedBatches through vigo_host_plan_batch: 48 planners of the small
world whose paths give many different control-point counts.  With the switch on, the solves and the device-resident rebound
rounds take planners of different counts in one device batch (vigo_optimize_mixed / vigo_rebound_rounds_mixed); every
planner must end with the plan it gets with the switch off — ok flag, solver status, control points bit for bit,
collisionSeg_, guides — in strictly fewer device batches."""
import numpy as np
import pytest

import mixed_cases as mc

pytestmark = pytest.mark.gpu
# poses per planner (the fit makes poses + 2 control points): seven counts in 8 .. 30, three in 34 .. 50
POSES = [6, 8, 10, 14, 18, 22, 28, 32, 38, 44]


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(r, label):
    for k in ("ok", "solver", "ncp", "n_guides", "n_seg"):
        assert np.array_equal(r[k][0], r[k][1]), f"{label}: {k} differs"
    for k in ("ctrl", "guides"):
        assert np.array_equal(bits(r[k][0]), bits(r[k][1])), f"{label}: {k} differs"
    assert np.array_equal(r["segs"][0], r["segs"][1]), f"{label}: collision segments differ"


def test_mixed_batches_give_every_planner_the_same_plan_in_fewer_device_batches(small_world):
    poses = [POSES[t % len(POSES)] for t in range(48)]
    off, xyz = mc.pose_lists(small_world, poses)
    r = mc.plan_batch_mixed(small_world, off, xyz)
    counts = sorted(set(int(x) for x in r["ncp"][0]))
    print(f"\n48 planners, control-point counts {counts}: {int(r['ok'][0].sum())} planned; device batches (planners in them) "
          f"off {r['counts'][0].tolist()}, on {r['counts'][1].tolist()}; {r['total_ms'][0, 0]:.1f} ms off, {r['total_ms'][1, 0]:.1f} ms on")
    assert len([c for c in counts if 8 <= c <= 30]) >= 6 and len([c for c in counts if 34 <= c <= 50]) >= 2
    _same(r, "setMixedBatches(true) against (false)")
    assert r["ok"][0].sum() >= 1
    assert 0 < r["counts"][1][0] < r["counts"][0][0]
    assert r["switches"] == 0


def test_a_workload_of_one_count_opens_the_same_batches(small_world):
    off, xyz = mc.pose_lists(small_world, [18], seed=5)
    off = (np.arange(49) * 18).astype(np.int32)
    r = mc.plan_batch_mixed(small_world, off, np.ascontiguousarray(np.tile(xyz, (48, 1))))
    assert len(set(int(x) for x in r["ncp"][0])) == 1
    _same(r, "one count")
    assert r["counts"][0].tolist() == r["counts"][1].tolist() and r["counts"][0][0] > 0
