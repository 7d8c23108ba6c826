"""-m gpu: bsplineTraj's per-call BatchOptions / BatchStats through vigo_host_plan_batch: ONE
makePlanBatch(planners, trajectories, yaw) per run, under the options a switch mask names (vigo_host_switches' bits).

Every mask runs by two routes — the options passed to the call, and the same options set as the process default through
the setters with the overload without options — and both must give every planner the same plan: ok flag, solver status,
control points, collisionSeg_, guides, positions and quaternions bit for bit; the same counts in the call's BatchStats; and
those counts must be what the process totals moved by (the test is single-threaded).  After the options route the process
default reads 0 although nothing was restored: it was never written.

Two calls at the same time, on two threads with a map object, planners and handles each, under DIFFERENT options: each
must give the plans and the counts of its solo run — what a process-wide switch or a totals difference cannot promise.

Workload: mixed_cases.pose_lists on the small world, 12 planners, poses cycling through [6, 10, 18, 28, 38, 44]: two shape
classes, six counts, two planners per count.  Every mask must give the stage it selects work (its decided + host-run
count > 0, asserted), and mixed batches must open fewer solve batches than default options.  12 planners were enough for
every stage: measured on an MI355X, 9 of them plan, the prologue makes 15 A* searches (14 decided by the device, one by
the host), the straight paths reach 8 re-guide steps, and the solves and rounds open 34 device batches, 20 when mixed."""
import numpy as np
import pytest

import mixed_cases as mc
import plan_batch as pb
from plan_batch import STAT_NAMES as FIELDS

pytestmark = pytest.mark.gpu
POSES = [6, 10, 18, 28, 38, 44]
ASTAR, GUIDES1, GUIDES2, PROLOGUE, REGUIDE1, REGUIDE2, MIXED, EPILOGUE = 1, 2, 4, 8, 16, 32, 64, 128
ALL = ASTAR | GUIDES1 | REGUIDE1 | MIXED | EPILOGUE
MASKS = [ASTAR, GUIDES1, GUIDES2, PROLOGUE, REGUIDE1, REGUIDE2, MIXED, EPILOGUE, ALL]
# the stage a mask bit selects -> its (decided, host-run) counts
STAGE = {ASTAR: ("astarDecided", "astarHost"), GUIDES1: ("guidesDecided", "guidesHost"), GUIDES2: ("guidesDecided", "guidesHost"),
         PROLOGUE: ("prologueDecided", "prologueHost"), REGUIDE1: ("reguideDecided", "reguideHost"), REGUIDE2: ("reguideDecided", "reguideHost"),
         EPILOGUE: ("epilogueDecided", "epilogueHost")}
PLAN_KEYS = ("ok", "solver", "ncp", "n_seg", "n_guides", "n_poses")
BIT_KEYS = ("ctrl", "guides", "pos", "quat")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def plan(world, off, xyz, mask, via_setters=0, second_mask=-1, budget=16384):
    """one makePlanBatch(planners, trajectories, yaw = true) under `mask` by the route via_setters (plan_batch's routes), or,
    second_mask >= 0, two at the same time -> dict of arrays [2, ...] (slot 1: the second thread's call), stats / totals as dicts"""
    both = second_mask >= 0
    r = pb.plan_batch(world, off, xyz, [(mask, budget, via_setters), (max(second_mask, 0), budget, pb.BY_CALL)], [0, 1] if both else [0], concurrent=both,
                      outputs=("ok", "solver", "ncp", "ctrl", "segs", "guides", "poses"), with_paths=True, pose_cap=256)
    return dict(stats=[dict(zip(FIELDS, (int(x) for x in s))) for s in r["stats"]], totals=dict(zip(FIELDS, (int(x) for x in r["totals"]))),
                seconds=r["slot_seconds"][:, 0, :2], total_ms=r["slot_seconds"][:, 0, 2] * 1e3, switches=r["switches"],
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_seg", "segs", "n_guides", "guides", "n_poses", "pos", "quat")})


def same_plans(a, sa, b, sb, label):
    """slot sa of run a against slot sb of run b"""
    for k in PLAN_KEYS:
        assert np.array_equal(a[k][sa], b[k][sb]), f"{label}: {k} differs: {a[k][sa].tolist()} / {b[k][sb].tolist()}"
    assert np.array_equal(a["segs"][sa], b["segs"][sb]), f"{label}: collision segments differ"
    for k in BIT_KEYS:
        same = bits(a[k][sa]) == bits(b[k][sb])
        assert same.all(), f"{label}: {k} differs at {np.argwhere(~same)[:4].tolist()}"


@pytest.fixture(scope="module")
def straight(small_world):
    """the 12 planners of the module's docstring"""
    off, xyz = mc.pose_lists(small_world, [POSES[t % len(POSES)] for t in range(12)])
    return small_world, off, xyz


_solo = {}


def solo(straight, mask):
    """the run of `mask` by the options route, made once and shared (never written to)"""
    if mask not in _solo:
        _solo[mask] = plan(*straight, mask)
    return _solo[mask]


@pytest.mark.parametrize("mask", MASKS)
def test_options_passed_to_the_call_equal_the_setters_and_count_for_the_call_alone(straight, mask):
    by_call = solo(straight, mask)
    by_setters = plan(*straight, mask, via_setters=1)
    st = by_call["stats"][0]
    print(f"\nmask {mask}: {int(by_call['ok'][0].sum())} of {by_call['ok'].shape[1]} planned; stats {st}; "
          f"{by_call['total_ms'][0]:.1f} ms by options, {by_setters['total_ms'][0]:.1f} ms by setters")
    same_plans(by_call, 0, by_setters, 0, f"mask {mask}: options passed to the call against the setters")
    assert st == by_setters["stats"][0], f"mask {mask}: the call's counts differ between the routes"
    assert st == by_call["totals"] and st == by_setters["totals"], f"mask {mask}: the counts are not what the process totals moved by"
    # the options route never wrote the default; the setters route put it back
    assert by_call["switches"] == 0 and by_setters["switches"] == 0
    # every stage the mask selects had work, and no other opt-in stage counted any
    selected = {STAGE[bit] for bit in STAGE if mask & bit}
    for decided, host in set(STAGE.values()):
        assert (st[decided] + st[host] > 0) == ((decided, host) in selected), f"mask {mask}: {decided} {st[decided]}, {host} {st[host]}"
    assert (st["epilogueGroups"] > 0) == bool(mask & EPILOGUE) and st["solveBatches"] > 0 and st["seedDecided"] + st["seedHost"] == 0
    if mask & MIXED:
        plain = solo(straight, 0)
        assert st["solveBatches"] < plain["stats"][0]["solveBatches"], "mixed batches opened no fewer device batches"
    if mask in (MIXED, EPILOGUE, ASTAR):       # (the other stages differ from the host steps by the last places of atan2)
        same_plans(by_call, 0, solo(straight, 0), 0, f"mask {mask} against default options")


def test_default_options_equal_the_untouched_default(straight):
    by_call = solo(straight, 0)
    untouched = plan(*straight, 0, via_setters=2)          # the overload without options, no setter called
    same_plans(by_call, 0, untouched, 0, "default-constructed options against the overload without options")
    assert by_call["stats"][0] == untouched["stats"][0] and by_call["ok"][0].sum() >= 1 and untouched["switches"] == 0
    assert len(set(int(x) for x in by_call["ncp"][0])) == len(POSES)


@pytest.mark.parametrize("mask, second", [(MIXED, 0), (EPILOGUE, GUIDES2)])
def test_two_calls_at_once_each_plan_and_count_as_alone(straight, mask, second):
    both = plan(*straight, mask, second_mask=second)
    for slot, m in enumerate((mask, second)):
        alone = solo(straight, m)
        same_plans(both, slot, alone, 0, f"thread {slot} under mask {m}, the other under {(second, mask)[slot]}")
        assert both["stats"][slot] == alone["stats"][0], f"thread {slot} under mask {m}: counts {both['stats'][slot]} / alone {alone['stats'][0]}"
    assert both["totals"] == {k: both["stats"][0][k] + both["stats"][1][k] for k in FIELDS}
    assert both["switches"] == 0
