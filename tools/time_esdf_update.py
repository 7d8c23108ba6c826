"""Times the ESDF region update — vigo_update_grid_region + vigo_update_esdf after vigo_build_esdf_tracked — against the
whole rebuild it replaces (vigo_build_esdf), on the config-2 world (256^3) and a config-4 world (512^3), or the sizes
given.  Run on the GPU box; one JSON line per measurement.  Device events on the handle's stream around each timed
call, warm repeats, one process.

Boxes of 16^3, 32^3 and 64^3 voxels at three kinds of place — "obstacle": the box whose occupied share is nearest one half, "open": empty
with the emptiest neighbourhood, "corner": at (0,0,0) — each FILLED (every voxel occupied) and CLEARED, from the unchanged world: a
repeat writes the box and refreshes (timed), then writes the world's own bytes back and refreshes (not timed).  Per
measurement: update_ms (both calls), region_ms and refresh_ms (each alone, from events between them), y_lines and x_lines
of the refresh, and the whole build of the same library beside it.

  --build-only        only vigo_build_esdf (what a library without the update can do); with --lib PATH: of that library,
                      e.g. a build of the parent commit
  --profile N S KIND  one case (world N, box S, kind) in a loop, nothing else: the run to put under
                      `rocprofv3 --kernel-trace --stats` for the time of each pass (k_esdf_region_z / _y / _x / _brick)"""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
from trajectory_planner_amd import _lib, synth
if "--lib" in sys.argv:                                   # another build, which may lack the newest entry points
    import ctypes
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    _other = ctypes.CDLL(_lib.LIB_PATH)
    _lib.PROTOTYPES = {k: p for k, p in _lib.PROTOTYPES.items() if hasattr(_other, k)}
from trajectory_planner_amd.vigo import Vigo
dev = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
COARSE = 8


def make_world(n):
    return (synth.make_box_world(synth.SEED_BASE + 2, n=n, keep_ids=False) if n <= 256 else
            synth.make_box_world(synth.SEED_BASE + 4, n=n, n_boxes=800, centre_range=24.0, keep_ids=False))


def places(occ, s):
    """{kind: lo} for boxes of s^3 on multiples of COARSE voxels, from counts of COARSE^3 cells: the box whose occupied
    share is nearest one half, the empty box with the fewest occupied voxels in its neighbourhood of one box width (of
    those the one nearest the grid's centre), and the corner"""
    N, m = occ.shape[0] // COARSE, s // COARSE
    c = occ.reshape(N, COARSE, N, COARSE, N, COARSE).sum(axis=(1, 3, 5)).astype(np.int64)

    def window_sums(g):
        """the count of [p - g, p + m + g) clipped, for every box position p"""
        I = np.zeros((N + 2 * g + 1,) * 3, dtype=np.int64)
        I[1 + g:1 + g + N, 1 + g:1 + g + N, 1 + g:1 + g + N] = c
        I = I.cumsum(0).cumsum(1).cumsum(2)
        w, k = m + 2 * g, N - m + 1
        a, b = slice(0, k), slice(w, w + k)
        return (I[b, b, b] - I[a, b, b] - I[b, a, b] - I[b, b, a] + I[a, a, b] + I[a, b, a] + I[b, a, a] - I[a, a, a])

    own, near = window_sums(0), window_sums(m)
    far = sum((np.arange(N - m + 1) - (N - m) / 2.0).reshape([-1 if a == k else 1 for a in range(3)]) ** 2 for k in range(3))
    at = lambda score: tuple(int(v) * COARSE for v in np.unravel_index(np.argmin(score), score.shape))
    return {"obstacle": at(np.abs(own / float(s ** 3) - 0.5) * 1e6 + far * 1e-3),
            "open": at(np.where(own == 0, near * 1e6 + far, np.inf)), "corner": (0, 0, 0)}


def timed(fn, reps):
    """mean ms of fn() by device events, after fn's own warm-up by the caller"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def build_rows(v, n, reps):
    for _ in range(2): v.build_esdf(plane=2)
    return {"build_ms": timed(lambda: v.build_esdf(plane=2), reps)}


args = [a for a in sys.argv[1:]]
sizes = [int(a) for a in args if a.isdigit()] or [256, 512]
build_id = _lib.load().vigo_build_id().decode()
if "--profile" in args:
    i = args.index("--profile")
    n, s, kind = int(args[i + 1]), int(args[i + 2]), args[i + 3]
    world = make_world(n)
    lo = places((world.voxels & 4) != 0, s)[kind]
    own = T(world.voxels[tuple(slice(l, l + s) for l in lo)])
    full = torch.full((s, s, s), 4, dtype=torch.uint8, device=dev)
    v = Vigo(0)
    v.set_grid(T(world.voxels), world.origin, world.res)
    v.build_esdf(plane=2, tracked=True)
    for _ in range(20):
        v.update_grid_region(lo, full); v.update_esdf()
        v.update_grid_region(lo, own); v.update_esdf()
    torch.cuda.synchronize()
    print(json.dumps({"profile": f"{n}^3, box {s}^3 {kind} at {lo}: 20 x (fill + refresh, restore + refresh)", "build_id": build_id}))
    sys.exit(0)
for n in sizes:
    world = make_world(n)
    occ = (world.voxels & 4) != 0
    v = Vigo(0)
    v.set_grid(T(world.voxels), world.origin, world.res)
    reps = 20 if n <= 256 else 5
    row = {"config": f"5d: vigo_build_esdf, {n}^3 box world, plane 2", "build_id": build_id, "lib": os.path.relpath(_lib.LIB_PATH, R)}
    row.update(build_rows(v, n, reps))
    print(json.dumps(row), flush=True)
    if "--build-only" in args:
        del v; torch.cuda.empty_cache()
        continue
    free0 = torch.cuda.mem_get_info(dev)[0]
    v.build_esdf(plane=2, tracked=True)
    torch.cuda.synchronize(); free1 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(2): v.build_esdf(plane=2, tracked=True)
    tracked_ms = timed(lambda: v.build_esdf(plane=2, tracked=True), reps)
    print(json.dumps({"config": f"5d: vigo_build_esdf_tracked, {n}^3", "build_id": build_id, "build_tracked_ms": tracked_ms,
                      "tracking_bytes_measured": free0 - free1, "tracking_bytes_stated": 12 * n ** 3 + 2 * n * n + 16}), flush=True)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for s in (16, 32, 64):
        for kind, lo in places(occ, s).items():
            own = T(world.voxels[tuple(slice(l, l + s) for l in lo)])
            for op, box in (("fill", torch.full((s, s, s), 4, dtype=torch.uint8, device=dev)), ("clear", torch.zeros(s, s, s, dtype=torch.uint8, device=dev))):
                v.update_grid_region(lo, box)
                stats = v.update_esdf(stats=True)
                v.update_grid_region(lo, own)
                back = v.update_esdf(stats=True)
                marks = []
                for _ in range(reps):
                    e = [ev(), ev(), ev()]
                    e[0].record(); v.update_grid_region(lo, box); e[1].record(); v.update_esdf(); e[2].record()
                    v.update_grid_region(lo, own); v.update_esdf()
                    marks.append(e)
                torch.cuda.synchronize()
                region = sum(e[0].elapsed_time(e[1]) for e in marks) / reps
                refresh = sum(e[1].elapsed_time(e[2]) for e in marks) / reps
                print(json.dumps({"config": f"5d: region update, {n}^3, box {s}^3 {kind} {op}", "lo": lo, "build_id": build_id,
                                  "changed_bytes": int((own.cpu().numpy() != box.cpu().numpy()).sum()),
                                  "region_ms": region, "refresh_ms": refresh, "update_ms": region + refresh,
                                  "y_lines": stats["y_lines"], "x_lines": stats["x_lines"], "x_lines_total": n * n,
                                  "restore_x_lines": back["x_lines"], "build_ms": row["build_ms"],
                                  "update_over_build": (region + refresh) / row["build_ms"]}), flush=True)
    # the lattice after all that equals a fresh build's
    a = v.update_esdf(return_lattice=True)
    b = v.build_esdf(plane=2, return_lattice=True)
    print(json.dumps({"config": f"5d: {n}^3 after every update", "bit_identical_to_a_rebuild": bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))}), flush=True)
    del a, b, v
    torch.cuda.empty_cache()
