"""Times the map snapshot refresh on the config-2 world (256^3) and a config-4 world (512^3), or the sizes given: the whole
route (vigo_set_grid_host: the only one before vigo_update_grid_region) against the region route for boxes of 64x64x32 and
128x128x64 voxels in the middle of the map — vigo_update_grid_region_host raw and with r = (4,4,2), the device-pointer forms
between device events, and the facade's refresh (DeviceLink::sync after ++version / after markChanged, checked against
mapAdapter::snapshotTotals).  The routes alternate inside one process: 3 warm-ups, then 20 repeats of each in turn.  One
JSON line per (size, box) with mean / min / max / std in ms; `--out FILE` appends them there too.  Run on the GPU box."""
import ctypes as C, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
from trajectory_planner_amd import _lib, synth
from trajectory_planner_amd.vigo import Vigo
dev = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
WARM, REPS, RADIUS = 3, 20, (4, 4, 2)
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [256, 512]
host = C.CDLL(os.path.join(R, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so"))
host.vigo_host_snapshot_refresh.restype = C.c_int
host.vigo_host_snapshot_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return dict(mean=float(ms.mean()), min=float(ms.min()), max=float(ms.max()), std=float(ms.std()))


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for size in sizes:
    world = (synth.make_box_world(synth.SEED_BASE + 2, n=size, keep_ids=False) if size <= 256 else
             synth.make_box_world(synth.SEED_BASE + 4, n=size, n_boxes=800, centre_range=24.0, keep_ids=False))
    vox = np.ascontiguousarray(world.voxels)
    vox_d = T(vox)
    v = Vigo(0)
    v.set_grid(vox_d, world.origin, world.res)
    for box in ((64, 64, 32), (128, 128, 64)):
        lo = tuple((size - b) // 2 for b in box)
        sub = np.ascontiguousarray(vox[tuple(slice(l, l + b) for l, b in zip(lo, box))])
        sub_d = T(sub)
        routes = {
            "set_grid_host": lambda: wall(lambda: v.set_grid_host(vox, world.origin, world.res)),
            "update_region_host_raw": lambda: wall(lambda: v.update_grid_region_host(lo, sub)),
            "update_region_host_inflate": lambda: wall(lambda: v.update_grid_region_host(lo, sub, RADIUS)),
            "set_grid_dev": lambda: events(lambda: v.set_grid(vox_d, world.origin, world.res)),
            "update_region_dev_raw": lambda: events(lambda: v.update_grid_region(lo, sub_d)),
            "update_region_dev_inflate": lambda: events(lambda: v.update_grid_region(lo, sub_d, RADIUS)),
        }
        ms = {k: [] for k in routes}
        for rep in range(WARM + REPS):
            for k, fn in routes.items():
                t = fn()
                if rep >= WARM:
                    ms[k].append(t)
        row = {"config": f"map region update, {size}^3 box world, box {box[0]}x{box[1]}x{box[2]}, r {RADIUS}",
               "build_id": _lib.load().vigo_build_id().decode(), "grid_bytes": int(vox.size), "box_bytes": int(sub.size),
               "launches": {"raw": 1, "inflate": 6}, "ms": {k: stats(t) for k, t in ms.items()}}
        # the facade: the same box announced by the owner, one refresh per repeat by either route
        dims, org = np.array(vox.shape, dtype=np.int32), np.ascontiguousarray(world.origin, dtype=np.float64)
        lo_a, n_a = np.array(lo, dtype=np.int32), np.array(box, dtype=np.int32)
        for mode, key in ((0, "facade_refresh_whole"), (1, "facade_refresh_box")):
            t, totals = np.zeros(WARM + REPS), np.zeros(3, dtype=np.int64)
            rc = host.vigo_host_snapshot_refresh(vox.ctypes.data, dims.ctypes.data, org.ctypes.data, float(world.res), lo_a.ctypes.data,
                                                 n_a.ctypes.data, mode, WARM + REPS, t.ctypes.data, totals.ctypes.data)
            assert rc == 0, rc
            want = [WARM + REPS, 0, 0] if mode == 0 else [0, WARM + REPS, (WARM + REPS) * int(sub.size)]
            assert totals.tolist() == want, (totals.tolist(), want)
            row["ms"][key] = stats(t[WARM:])
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")
    del v, vox_d
    torch.cuda.empty_cache()
