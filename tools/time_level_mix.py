"""Times vigo_optimize on batches that mix level trajectories with trajectories that have vertical structure, on an MI355X
(profiles/README.md, "One launch for a small batch"): 1024 x 32 on the configs[1] world and trajectories (bench.py), fp64
reference order, 50 iterations, no obstacle list.  A share of 0, 1/64, 1/2 and 1 of the trajectories — evenly spread
over the batch — gets vertical jitter far beyond the level band (sigma 0.03 on every control point; the class counts are
checked with the level rule of tests/gpu_util.py).  Time per call: the host clock around call + synchronise on a fresh
copy of the control points, median of --reps (>= 50) after --warmup.  Prints one JSON line per process; --out appends it
to a file.  Run on the GPU box, one process per library to compare."""
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

from gpu_util import is_level  # noqa: E402
from trajectory_planner_amd import synth  # noqa: E402
from trajectory_planner_amd._lib import load  # noqa: E402
from trajectory_planner_amd.vigo import Vigo, default_params  # noqa: E402

SHARES = (("0", 0), ("1/64", 16), ("1/2", 512), ("1", 1024))   # (name, trajectories of 1024 that are not level)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.reps < 50:
    sys.exit("time_level_mix: at least 50 timed calls per share")
if not torch.cuda.is_available():
    sys.exit("time_level_mix: no GPU (a CPU run measures nothing about the device)")

B, N = 1024, 32
world = synth.make_box_world(synth.SEED_BASE + 2, n=256, n_boxes=200)
base = synth.make_bspline_batch(world, B, N, synth.SEED_BASE + 2 + 1000)
assert is_level(base.ctrl).all()
T = lambda a, dev: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
P = default_params()
P.max_iterations = 50
v = Vigo(0, P)
v.set_grid(T(world.voxels, v.device), world.origin, world.res)
goff, gpv = T(base.guide_off, v.device), T(base.guide_pv, v.device)
gunk = v.guides_unknown(gpv)

out = {"build": load().vigo_build_id().decode(), "B": B, "N": N, "reps": args.reps, "warmup": args.warmup,
       "fuse_switch": os.environ.get("VIGO_EXP_FUSE", "")}
for name, n_out in SHARES:
    ctrl = base.ctrl.copy()
    which = (np.arange(n_out) * (B // n_out)) if n_out else np.zeros(0, dtype=np.int64)
    ctrl[which, :, 2] += np.random.default_rng(41).normal(0.0, 0.03, size=(n_out, N))
    level = is_level(ctrl)
    assert int((~level).sum()) == n_out and not level[which].any()
    ctrl0 = T(ctrl, v.device)
    ms = []
    for rep in range(args.warmup + args.reps):
        c = ctrl0.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = v.optimize(c, goff, gpv, gunk, inplace=True)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms[args.warmup:])
    out[f"share_{name}"] = {"not_level": n_out, "level": int(level.sum()), "median_ms": round(float(np.median(ms)), 4),
                            "min_ms": round(float(ms.min()), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4),
                            "iters_sum": int(r.iters.sum().item())}
v.close()
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
