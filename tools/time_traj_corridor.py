"""Times vigo_traj_corridor_check on config 3's 4096 segments regrouped into 512 trajectories of 8 (synth.
make_corridor_trajectories, ~10 000 samples per segment) against vigo_corridor_check on the same 4096 segments with the
same sample counts and step, on the 256 x 256 x 64 world of tools/time_corridor.py (HIP events, a warm-up, 20
alternating repetitions), and polyTrajOctomap::makePlanBatch of 32 and 1024 planners through vigo_host_poly_plan_batch
(wall clock, one run after a warm-up); prints one JSON line (medians in ms).  Run on the GPU box."""
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

dev = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
rng = np.random.default_rng(3)
vox = np.zeros((256, 256, 64), dtype=np.uint8)
for _ in range(300):
    c = rng.integers(8, 248, size=2); s = rng.integers(1, 6, size=2)
    vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], 0:rng.integers(10, 64)] |= 4
unk = rng.random((32, 32, 8)) < 0.05
vox[np.repeat(np.repeat(np.repeat(unk, 8, 0), 8, 1), 8, 2)] |= 2
v = Vigo(0)
v.set_grid(T(vox), np.array([-12.8, -12.8, -1.0]), 0.1)
box, res = [0.4, 0.4, 0.2], 0.2
seg_off, coeffs, knots, delT, endpoint = synth.make_corridor_trajectories(33, 512, 8, extent_lo=(-10, -10, 0.5),
                                                                          extent_hi=(10, 10, 2.5), n_samples=10000)
# the same samples per segment for the per-segment entry: each run's length, the trajectory's step
K = 8
run_len = np.zeros(512 * K, np.int32)
lib = load()
import ctypes as C  # noqa: E402
for t in range(512):
    k = np.ascontiguousarray(knots[t * (K + 1):(t + 1) * (K + 1)])
    first, length, n = np.zeros(K, np.int32), np.zeros(K, np.int32), C.c_int32()
    assert lib.vigo_traj_sample_runs(K, k.ctypes.data_as(C.c_void_p), float(delT[t]), first.ctypes.data_as(C.c_void_p),
                                     length.ctypes.data_as(C.c_void_p), C.byref(n)) == 0
    run_len[t * K:(t + 1) * K] = length
seg_delT = np.repeat(delT, K)
d_args = [T(a) for a in (seg_off, coeffs, knots, delT, endpoint)]
d_c, d_n, d_d = T(coeffs), T(run_len), T(seg_delT)


def traj():
    return v.traj_corridor_check(*d_args, box, res, nonfinite_collides=True)


def segs():
    return v.corridor_check(d_c, d_n, d_d, box, res)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def facade_times(reps=1):
    """median milliseconds of polyTrajOctomap::makePlanBatch for 32 and 1024 planners (vigo_host_poly_plan_batch, no solo
    twins) on a seeded pillar world, paths of 4-8 waypoints (every 16th of 13), modes mixed"""
    HL = C.CDLL(os.path.join(R, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so"))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    HL.vigo_host_poly_plan_batch.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_double, C.c_void_p, C.c_int, ip, dp, dp, ip,
                                             C.c_int, dp, dp, dp, dp, dp]
    r = np.random.default_rng(5)
    wv = np.zeros((128, 128, 40), dtype=np.uint8)
    for _ in range(25):
        c = r.integers(10, 118, size=2); s = r.integers(1, 4, size=2)
        wv[c[0] - s[0]:c[0] + s[0] + 1, c[1] - s[1]:c[1] + s[1] + 1, :] |= 5
    org = np.array([-6.4, -6.4, -0.5])
    cfg = np.array([0.4, 0.4, 0.2, 0.2, 0.1, 1.0, 0.5, 0.8, 8.0, 20, 0.1, 0.0])
    out = {}
    for P in (32, 1024):
        paths = []
        for i in range(P):
            W = 13 if i % 16 == 5 else int(r.integers(4, 9))
            a, b = r.uniform([-5, -5, 0.8], [5, 5, 1.6], size=(2, 3))
            paths.append(a + np.linspace(0, 1, W)[:, None] * (b - a))
        off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
        wp = np.ascontiguousarray(np.concatenate(paths))
        md = (np.arange(P) % 2).astype(np.int32)
        tr, info, secs = np.zeros((P, 1, 3)), np.zeros((P, 4)), np.zeros(2)
        t = []
        for _ in range(reps + 1):
            assert HL.vigo_host_poly_plan_batch(128, 128, 40, org.ctypes.data_as(dp), 0.1, wv.ctypes.data_as(C.c_void_p), P,
                                                off.ctypes.data_as(ip), wp.ctypes.data_as(dp), cfg.ctypes.data_as(dp),
                                                md.ctypes.data_as(ip), 1, tr.ctypes.data_as(dp), info.ctypes.data_as(dp), None,
                                                None, secs.ctypes.data_as(dp)) == 0
            t.append(secs[0] * 1e3)
        out["makePlanBatch_%d_ms" % P] = float(np.median(t[1:]))
        out["makePlanBatch_%d_valid" % P] = int(info[:, 0].sum())
    return out


for _ in range(3):
    traj(); segs()
torch.cuda.synchronize()
tt, ts = [], []
for _ in range(20):
    tt.append(timed(traj))
    ts.append(timed(segs))
st, n, flag, first, count, seg = traj()
fl2, _, _ = segs()
print(json.dumps({
    "workload": "512 trajectories x 8 segments (4096 segments, %d samples), box 0.4/0.4/0.2, map_resolution 0.2" % int(run_len.sum()),
    "traj_corridor_check_ms": float(np.median(tt)), "corridor_check_same_samples_ms": float(np.median(ts)),
    "ratio": float(np.median(tt) / np.median(ts)),
    "traj_ms_all": [round(x, 4) for x in tt], "seg_ms_all": [round(x, 4) for x in ts],
    "colliding_trajectories": int(flag.sum()), "colliding_segments_traj": int(seg.sum()),
    "colliding_segments_per_segment_entry": int(fl2.sum()),
    **facade_times()}))
