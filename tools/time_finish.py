"""Times the plan's last stage (steps 5-6 of makePlan() and the samples of evalTrajToMsg) for --planners planners, on two
workloads: every planner with 32 control points, and the ten control-point counts of tests/test_gpu_mixed_facade.py in
turn.  The control points are random walks with the spacing of a planned path; the stage reads nothing else.
  host_*    bsplineTraj's host epilogue — the spline object, linearFeasibilityReparam() and evalTrajToMsg per planner on the
            facade's workers — with setDeviceEpilogue(false): the code path of the parent commit
  launch_*  the vigo_traj_finish launch alone, between two events on the handle's stream, tables cached
  stage_*   the facade stage with setDeviceEpilogue(true): pack, upload, launch, download, install (paths and yaw included)
host and stage alternate inside vigo_host_finish_timing, which also counts the planners whose factor or path differs between
the two (must be 0).  Medians of --reps after --warmup.  Prints one JSON line; --out appends it to a file.  Run on the GPU box."""
import argparse
import ctypes as C
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trajectory_planner_amd import synth  # noqa: E402
from trajectory_planner_amd._lib import load  # noqa: E402
from trajectory_planner_amd.vigo import Vigo  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--planners", type=int, default=1024)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("time_finish: no GPU (a CPU run measures nothing about the device)")

POSES = [6, 8, 10, 14, 18, 22, 28, 32, 38, 44]      # + 2 control points each
P = args.planners
n_all = args.warmup + args.reps
med = lambda x: float(np.median(np.asarray(x)[args.warmup:]))
rng = np.random.default_rng(11)
lib = load()
H = C.CDLL(os.path.join(R, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so"))
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
H.vigo_host_finish_timing.restype = C.c_int
H.vigo_host_finish_timing.argtypes = [C.c_void_p, ip, dp, C.c_double, dp, C.c_int, C.c_int, ip, dp, C.c_int, dp, C.POINTER(C.c_longlong)]
vox = np.zeros((8, 8, 8), np.uint8)
origin = np.zeros(3)
cfg = np.ascontiguousarray(synth.PIPELINE_CFG, dtype=np.float64)


def rows(counts, Ns):
    ctrl = np.zeros((len(counts), Ns, 3))
    for b, n in enumerate(counts):
        h = rng.uniform(0.0, 2 * np.pi)
        step = 0.25 * np.array([np.cos(h), np.sin(h), 0.0]) + rng.normal(0.0, 0.03, (n, 3))
        ctrl[b, :n] = rng.uniform(-3.0, 3.0, 3) + np.cumsum(step, axis=0)
    return ctrl


def measure(counts):
    Ns = max(counts)
    ctrl, npts = rows(counts, Ns), np.ascontiguousarray(counts, dtype=np.int32)
    ms, bad = np.zeros((n_all, 2)), C.c_longlong(-1)
    rc = H.vigo_host_finish_timing(vox.ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), origin.ctypes.data_as(dp), 0.1, cfg.ctypes.data_as(dp), P, Ns,
                                   npts.ctypes.data_as(ip), ctrl.ctypes.data_as(dp), n_all, ms.ctypes.data_as(dp), C.byref(bad))
    assert rc == 0, rc
    # the launch alone: the planners' limits (the harness's 2.0 / 3.0), the facade's sample step (ts) and capacity
    v = Vigo(0)
    d = v.device
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    dt = v.params.ts
    S_cap = int((Ns - 3) * v.params.ts_ctrl / dt) + 2
    dc, dl, dn = T(ctrl), T(np.tile([2.0, 3.0], (P, 1))), (None if len(set(counts)) == 1 else T(npts))
    out = (torch.zeros(P, S_cap, 3, dtype=torch.float64, device=d), torch.zeros(P, S_cap, 3, dtype=torch.float64, device=d))
    v.use_current_stream()
    launch = []
    for _ in range(n_all):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = v.traj_finish(dc, dl, dt, S_cap, n_pts=dn, out=out, want_max=False)
        e1.record()
        torch.cuda.synchronize()
        launch.append(e0.elapsed_time(e1))
    assert (r["status"] == 0).all()
    v.close()
    return {"counts": sorted(set(counts)), "Ns": Ns, "samples_mean": float(r["n"].double().mean()), "host_ms": med(ms[:, 0]), "stage_ms": med(ms[:, 1]),
            "launch_ms": med(launch), "host_ms_min_max": [float(ms[args.warmup:, 0].min()), float(ms[args.warmup:, 0].max())],
            "stage_ms_min_max": [float(ms[args.warmup:, 1].min()), float(ms[args.warmup:, 1].max())],
            "launch_ms_min_max": [float(np.min(launch[args.warmup:])), float(np.max(launch[args.warmup:]))], "mismatch": int(bad.value)}


line = {"tool": "time_finish", "planners": P, "reps": args.reps, "warmup": args.warmup, "build": lib.vigo_build_id().decode(),
        "uniform32": measure([32] * P), "ten_counts": measure([POSES[t % len(POSES)] + 2 for t in range(P)])}
text = json.dumps(line)
print(text)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
