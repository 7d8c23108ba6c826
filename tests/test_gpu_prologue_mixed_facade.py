"""-m gpu: bsplineTraj::makePlanBatch under BatchOptions::mixedPrologue through vigo_host_plan_batch: the 48
planners and ten control-point counts of tests/test_gpu_mixed_facade.py.  With the option on, the devicePrologue chain,
the deviceGuides = 1 and deviceAstar launches and the deviceReguide = 1 call group their planners as the mixed solves do and
call the _mixed entries; every planner must end with the plan it gets with the option off — ok flag, solver status,
control points and guides bit for bit, collisionSeg_, A* paths, sampled poses — in strictly fewer prologue groups."""
import numpy as np
import pytest

import mixed_cases as mc
import prologue_mixed_cases as pm
from test_gpu_mixed_facade import POSES

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(r, label):
    for k in ("ok", "solver", "ncp", "n_guides", "n_seg", "n_path_pts", "n_poses"):
        assert np.array_equal(r[k][0], r[k][1]), f"{label}: {k} differs"
    for k in ("ctrl", "guides", "paths", "pos", "quat"):
        assert np.array_equal(bits(r[k][0]), bits(r[k][1])), f"{label}: {k} differs"
    assert np.array_equal(r["segs"][0], r["segs"][1]), f"{label}: collision segments differ"
    assert r["switches"] == 0 and r["mixed_prologue_default"] == 0                # the process defaults read 0 afterwards


@pytest.fixture(scope="module")
def workload(small_world):
    return mc.pose_lists(small_world, [POSES[t % len(POSES)] for t in range(48)])


@pytest.mark.parametrize("stages", ["chain", "guides and astar"])
def test_mixed_prologue_gives_every_planner_the_same_plan_in_fewer_groups(small_world, workload, stages):
    off, xyz = workload
    mask = (pm.M_PROLOGUE if stages == "chain" else pm.M_GUIDES1 | pm.M_ASTAR) | pm.M_REGUIDE1 | pm.M_MIXED_BATCHES
    r = pm.plan_batch_mixed_prologue(small_world, off, xyz, mask)
    c = r["counts"]
    counts = sorted(set(int(x) for x in r["ncp"][0]))
    print(f"\n48 planners, control-point counts {counts}, {stages}: {int(r['ok'][0].sum())} planned; off / on: prologue groups "
          f"{c['prologueGroups'].tolist()}, re-guide groups {c['reguideGroups'].tolist()} (re-guide steps on the device {c['reguideDecided'].tolist()}: "
          f"{'re-guides happened' if c['reguideDecided'][0] + c['reguideHost'][0] > 0 else 'NO re-guide happened'}), prologue planners on the device "
          f"{c['prologueDecided'].tolist()}, guides + searches on the device {c['guidesAstarDecided'].tolist()}, solve batches {c['solveBatches'].tolist()}")
    assert len(counts) >= 8
    _same(r, f"mixedPrologue on against off, {stages}")
    assert r["ok"][0].sum() >= 1 and (r["n_guides"][0] > 0).any()
    assert 0 < c["prologueGroups"][1] < c["prologueGroups"][0]
    assert c["reguideGroups"][1] <= c["reguideGroups"][0]
    assert c["solveBatches"][0] == c["solveBatches"][1]
    # the device decides what it decided before
    for k in ("prologueDecided", "prologueHost", "reguideDecided", "reguideHost", "guidesAstarDecided"):
        assert c[k][0] == c[k][1], k


def test_a_workload_of_one_count_opens_the_same_groups(small_world):
    off, xyz = mc.pose_lists(small_world, [18], seed=5)
    off = (np.arange(49) * 18).astype(np.int32)
    r = pm.plan_batch_mixed_prologue(small_world, off, np.ascontiguousarray(np.tile(xyz, (48, 1))), pm.M_PROLOGUE | pm.M_REGUIDE1 | pm.M_MIXED_BATCHES)
    assert len(set(int(x) for x in r["ncp"][0])) == 1
    _same(r, "one count")
    c = r["counts"]
    assert c["prologueGroups"][0] == c["prologueGroups"][1] > 0 and c["reguideGroups"][0] == c["reguideGroups"][1]
