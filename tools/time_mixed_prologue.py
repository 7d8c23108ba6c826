#!/usr/bin/env python3
"""makePlanBatch with BatchOptions::mixedPrologue off against on: P planners over the ten control-point counts of
tests/test_gpu_mixed_facade.py under devicePrologue + deviceReguide = 1 + mixedBatches, both settings in ONE process,
interleaved run by run on fresh planners (vigo_host_plan_batch), the first `--warmup` rounds discarded.
"off" is the behaviour before the option existed: the baseline.  Prints the median and the spread (min .. max) of
prologueSeconds, chainSeconds and the call's wall time per setting, the group counts, and one JSON line.

    python tools/time_mixed_prologue.py --planners 1024 --reps 7 --warmup 2
"""
import argparse
import json
import os
import sys

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "tests"))
sys.path.insert(0, R)
import mixed_cases as mc  # noqa: E402
import prologue_mixed_cases as pm  # noqa: E402
from test_gpu_mixed_facade import POSES  # noqa: E402
from trajectory_planner_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planners", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    world = synth.make_box_world(synth.SEED_BASE + 2, n=128, n_boxes=60, centre_range=5.5, z_range=2.0)      # the suite's small world
    off, xyz = mc.pose_lists(world, [POSES[t % len(POSES)] for t in range(a.planners)])
    mask = pm.M_PROLOGUE | pm.M_REGUIDE1 | pm.M_MIXED_BATCHES
    r = pm.plan_batch_mixed_prologue(world, off, xyz, mask, reps=a.warmup + a.reps)
    same = all(np.array_equal(np.ascontiguousarray(r[k][0]).view(np.int64), np.ascontiguousarray(r[k][1]).view(np.int64)) for k in ("ctrl", "guides")) and \
        np.array_equal(r["ok"][0], r["ok"][1])
    sec = r["seconds"][:, a.warmup:, :] * 1e3
    out = dict(planners=a.planners, counts=sorted(set(int(x) for x in r["ncp"][0])), reps=a.reps, warmup=a.warmup, same_plans=bool(same),
               planned=int(r["ok"][0].sum()))
    for s, name in enumerate(("off", "on")):
        out[name] = {k: int(v[s]) for k, v in r["counts"].items()}
        for j, what in enumerate(("prologue_ms", "chain_ms", "total_ms")):
            v = sec[s, :, j]
            out[name][what] = dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3))
    print(f"{a.planners} planners, counts {out['counts']}, {out['planned']} planned, same plans: {same}; {a.reps} interleaved repeats after {a.warmup} warm-up rounds")
    print(f"{'':>10} {'prologue groups':>16} {'re-guide groups':>16} {'prologue ms':>24} {'chain ms':>24} {'total ms':>24}")
    for name in ("off", "on"):
        o = out[name]
        f = lambda d: f"{d['median']:8.2f} ({d['min']:.2f} .. {d['max']:.2f})"
        print(f"{name:>10} {o['prologueGroups']:>16} {o['reguideGroups']:>16} {f(o['prologue_ms']):>24} {f(o['chain_ms']):>24} {f(o['total_ms']):>24}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
