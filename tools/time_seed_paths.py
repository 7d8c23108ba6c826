"""Times the seed-path stage (getTrajectory(dt), the inputPathCheck search, updatePath's head) for 1024 start/goal pairs on
a pillar world, 60 x 60 x 20 voxels of 0.1 m:
  stage_*   up to installed control points, through vigo_host_seed_timing (wall clock around calls that end in a stream
            synchronise; the three variants alternate): the serial host loop followed by updatePathBatch (what existed
            before seedPathBatch), seedPathBatch on the host workers, seedPathBatch with the vigo_seed_paths launch
  entry_*   the device entry alone on vigo_minsnap's polynomials for the same pairs, into output arrays allocated before
            the clock: the call to its synchronise (host clock), and the download of every output array
Medians of --reps repetitions after --warmup.  Prints one JSON line; --out appends it to a file.  Run on the GPU box."""
import argparse
import ctypes as C
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trajectory_planner_amd._lib import load  # noqa: E402
from trajectory_planner_amd.vigo import Vigo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("time_seed_paths: no GPU (a CPU run measures nothing about the device)")

rng = np.random.default_rng(5)
vox = np.zeros((60, 60, 20), np.uint8)
for _ in range(25):
    c = rng.integers(3, 57, size=2)
    s = rng.integers(1, 4, size=2)
    vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], :] |= int(rng.choice([1, 3, 3]))
origin, res, P = np.array([-3.0, -3.0, 0.0]), 0.1, args.pairs
se = np.ascontiguousarray(np.concatenate([rng.uniform([-2.5, -2.5, 0.8], [-1.0, 2.5, 1.4], size=(P, 1, 3)),
                                          rng.uniform([1.0, -2.5, 0.8], [2.5, 2.5, 1.4], size=(P, 1, 3))], 1))
_dp = C.POINTER(C.c_double)
D = lambda a: a.ctypes.data_as(_dp)
med = lambda x: float(np.median(x))

# ---- the stage through the facade ------------------------------------------------------------------------------------
H = C.CDLL(os.path.join(R, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so"))
H.vigo_host_seed_timing.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, _dp,
                                    C.POINTER(C.c_longlong)]
poly_cfg = np.full(16, np.nan)
poly_cfg[3] = poly_cfg[4] = 1.0                                 # desired_velocity, desired_acceleration
bsp_cfg = np.array([0.5, 0.0, 2.0, 0.5, 0.5, 0.5])              # a small A* pool: 1024 planners each own one
n = args.warmup + args.reps
ms, totals = np.zeros((n, 3)), np.zeros(2, np.int64)
rc = H.vigo_host_seed_timing(*vox.shape, D(origin), res, vox.ctypes.data_as(C.c_void_p), P, D(se), D(poly_cfg), D(bsp_cfg), 16, n, D(ms),
                             totals.ctypes.data_as(C.POINTER(C.c_longlong)))
assert rc == 0, rc
ms = ms[args.warmup:]

# ---- the device entry alone --------------------------------------------------------------------------------------------
lib = load()
v = Vigo(0)
dev = v.device
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
v.set_grid(T(vox), origin, res)
coeffs, knots, status = v.minsnap(T(se), conds=T(np.zeros((P, 4, 3))), vel=1.0)
assert (status == 0).all()
seg_off = T(np.arange(P + 1, dtype=np.int32))
a = [seg_off, coeffs.reshape(P, 3, 8).contiguous(), knots.reshape(-1).contiguous(), knots[:, 1].contiguous(), T(np.full(P, 0.25)),
     T(np.full(P, 0.25)), T(np.full(P, 1000.0))]
# the output arrays are allocated once, outside the clock: the timed call is the entry alone
OUT = ("status", "tries", "dt", "final_time", "seed_n", "seed", "fit_n", "fit", "prev_seed", "prev_fit")
CAP = 128
r = {k: torch.zeros(P, dtype=torch.int32, device=dev) for k in ("status", "tries", "seed_n", "fit_n")}
r.update({k: torch.zeros(P, dtype=torch.float64, device=dev) for k in ("dt", "final_time", "prev_seed", "prev_fit")})
r.update({k: torch.zeros(P, CAP, 3, dtype=torch.float64, device=dev) for k in ("seed", "fit")})
a += [torch.zeros(P, dtype=torch.float64, device=dev), torch.zeros(P, dtype=torch.float64, device=dev)]   # prev_in_seed, prev_in_fit
ptr = lambda x: C.c_void_p(x.data_ptr())
launch, download = [], []
for _ in range(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.vigo_seed_paths(v._h, P, P, 7, *[ptr(x) for x in a], 16, CAP, *[ptr(r[k]) for k in OUT])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    host = {k: x.cpu() for k, x in r.items()}
    t2 = time.perf_counter()
    assert rc == 0, rc
    launch.append(1e3 * (t1 - t0))
    download.append(1e3 * (t2 - t1))
st = host["status"].numpy()
line = {"tool": "time_seed_paths", "pairs": P, "reps": args.reps, "warmup": args.warmup, "build": lib.vigo_build_id().decode(),
        "stage_serial_then_updatePathBatch_ms": med(ms[:, 0]), "stage_seedPathBatch_host_ms": med(ms[:, 1]),
        "stage_seedPathBatch_device_ms": med(ms[:, 2]), "stage_ms_min": ms.min(0).tolist(), "stage_ms_max": ms.max(0).tolist(),
        "stage_device_decided": int(totals[0]), "stage_host_run": int(totals[1]),
        "entry_launch_ms": med(launch[args.warmup:]), "entry_download_ms": med(download[args.warmup:]),
        "entry_status_counts": np.bincount(st, minlength=6).tolist(), "entry_mean_tries": float(host["tries"].float().mean()),
        "entry_mean_seed_poses": float(host["seed_n"].float().mean())}
text = json.dumps(line)
print(text)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
