"""Times the mixed-count entries on an MI355X (profiles/README.md, "Mixed batches"):
  solve_*   vigo_optimize_mixed with EVERY count equal to 32 against vigo_optimize on the same B x 32 batch (config 2's
            world and trajectories), B = 1024 and 16 384: the price of the general-only plan — one launch of the general
            kernel where the uniform entry picks the level / no-obstacle kernels.  Host clock around call + synchronise,
            the two entries alternating in one process, medians of --reps after --warmup.
  plan_*    bsplineTraj::makePlanBatch through vigo_host_plan_batch on --planners planners whose control-point
            counts are spread over 8 .. 40 (most of them short, as the seed stage leaves them), setMixedBatches off
            against on, alternating, fresh planners every run; device batches opened per run under either setting.
Prints one JSON line; --out appends it to a file.  Run on the GPU box."""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trajectory_planner_amd import synth  # noqa: E402
from trajectory_planner_amd._lib import load  # noqa: E402
from trajectory_planner_amd.vigo import PREC_F64, PREC_F64_FAST, Vigo, default_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--planners", type=int, default=1024)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("time_mixed_batch: no GPU (a CPU run measures nothing about the device)")
med = lambda x: float(np.median(x))
out = {"build": load().vigo_build_id().decode(), "reps": args.reps, "warmup": args.warmup}

# ---- (i) the general-only plan on a uniform batch ----------------------------------------------------------------------
world = synth.make_box_world(synth.SEED_BASE + 2)
T = lambda a, dev: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
for mode, prec in (("f64", PREC_F64), ("f64_fast", PREC_F64_FAST)):
    P = default_params()
    P.max_iterations = 50
    v = Vigo(0, P, prec)
    v.set_grid(T(world.voxels, v.device), world.origin, world.res)
    for B in (1024, 16384):
        b = synth.make_bspline_batch(world, B, 32, 7)
        ctrl0, goff, gpv = T(b.ctrl, v.device), T(b.guide_off, v.device), T(b.guide_pv, v.device)
        gunk = v.guides_unknown(gpv)
        n_pts = torch.full((B,), 32, dtype=torch.int32, device=v.device)
        runs = {"uniform": lambda c: v.optimize(c, goff, gpv, gunk, inplace=True),
                "mixed": lambda c: v.optimize_mixed(n_pts, c, goff, gpv, gunk, inplace=True)}
        ms = {k: [] for k in runs}
        results = {}
        for rep in range(args.warmup + args.reps):
            for k, run in runs.items():              # alternating
                c = ctrl0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = run(c)
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3)
                results[k] = (r.ctrl, r.status)
        same = bool(torch.equal(results["uniform"][0], results["mixed"][0]) and torch.equal(results["uniform"][1], results["mixed"][1]))
        for k in runs:
            out[f"solve_{mode}_{B}x32_{k}_ms"] = round(med(ms[k][args.warmup:]), 4)
        out[f"solve_{mode}_{B}x32_same_bits"] = same
    v.close()

# ---- (ii) makePlanBatch, switch off against on ---------------------------------------------------------------------------
import mixed_cases as mc  # noqa: E402

pworld = synth.make_pipeline_world()
rng = np.random.default_rng(17)
ncp = np.clip(np.round(8 + rng.gamma(2.0, 5.0, size=args.planners)), 8, 40).astype(int)
off, xyz = mc.pose_lists(pworld, [int(n) - 2 for n in ncp], seed=29)
r = mc.plan_batch_mixed(pworld, off, xyz, reps=args.warmup + args.reps)
got = sorted(set(int(x) for x in r["ncp"][0]))
out.update(plan_planners=args.planners, plan_distinct_counts=len(got), plan_count_range=[got[0], got[-1]], plan_mean_count=round(float(r["ncp"][0].mean()), 2),
           plan_planned=int(r["ok"][0].sum()), plan_same_plans=bool(all(np.array_equal(r[k][0], r[k][1]) for k in ("ok", "solver", "ncp", "ctrl", "segs", "guides"))),
           plan_off_ms=round(med(r["total_ms"][0, args.warmup:]), 3), plan_on_ms=round(med(r["total_ms"][1, args.warmup:]), 3),
           plan_off_device_batches=int(r["counts"][0, 0]), plan_on_device_batches=int(r["counts"][1, 0]))
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
