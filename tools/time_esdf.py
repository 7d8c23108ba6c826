"""Times vigo_esdf_query at the BASELINE configs[4] size (1 048 576 queries, 256^3 lattice): uniform random and
brick-sorted query order; prints one JSON line per case.  Run on the GPU box.  `--f32`: vigo_esdf_query_f32 (float3 in,
float4 out — the I/O width SURVEY.md §8(d) config 5 states) instead of the fp64 entry; `--both`: one after the other.
`--build [N ...]`: times vigo_build_esdf instead (device events around warm repeats on the handle's stream) on the
config-2 world (256^3) and a config-4 world (512^3), or the sizes given, against the host route — synth.edt_esdf, the
upload and vigo_set_esdf — and compares the two lattices bit for bit; `--no-host` leaves the host route out.  Also per
size: the workspace as the device's free memory shows it (the drop across the first build, the bricked field allocated
beforehand) beside the 8 bytes per voxel the source states, and the build of an EMPTY map of the same size — the longest
scans there are."""
import json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
from trajectory_planner_amd import synth
from trajectory_planner_amd.vigo import Vigo
dev = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
if "--build" in sys.argv:
    from trajectory_planner_amd import _lib
    sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [256, 512]
    for n in sizes:
        world = (synth.make_box_world(synth.SEED_BASE + 2, n=n, keep_ids=False) if n <= 256 else
                 synth.make_box_world(synth.SEED_BASE + 4, n=n, n_boxes=800, centre_range=24.0, keep_ids=False))
        v = Vigo(0)
        v.set_grid(T(world.voxels), world.origin, world.res)
        # the handle's allocations are the library's own (not torch's): a field of these dims first, so that the first
        # build allocates the workspace and nothing else, and the device's free memory before and after it
        v.set_esdf(torch.zeros(n, n, n, dtype=torch.float32, device=dev), world.origin, world.res)
        torch.cuda.synchronize(); free0 = torch.cuda.mem_get_info(dev)[0]
        v.build_esdf(plane=2)
        torch.cuda.synchronize(); free1 = torch.cuda.mem_get_info(dev)[0]
        row = {"config": f"5c: vigo_build_esdf, {n}^3 box world, plane 2", "build_id": _lib.load().vigo_build_id().decode(),
               "workspace_bytes_measured": free0 - free1, "workspace_bytes_stated": 8 * n ** 3,
               "site_fraction": float(((world.voxels & 4) != 0).mean())}
        for key, kw in (("build_ms", dict(plane=2)), ("build_plane0_unknown_ms", dict(plane=0, unknown_is_site=True))):
            for _ in range(3): v.build_esdf(**kw)
            reps = 20 if n <= 256 else 5
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): v.build_esdf(**kw)
            e1.record(); torch.cuda.synchronize()
            row[key] = e0.elapsed_time(e1) / reps
        lat = v.build_esdf(plane=2, return_lattice=True)
        if "--no-host" not in sys.argv:
            t0 = time.perf_counter()
            dist, origin = synth.edt_esdf(world)
            t1 = time.perf_counter()
            dist_d = T(dist); v.set_esdf(dist_d, origin, world.res); torch.cuda.synchronize()
            t2 = time.perf_counter()
            row.update(host_edt_s=t1 - t0, upload_and_set_esdf_ms=(t2 - t1) * 1e3, host_route_s=t2 - t0,
                       bit_identical_to_edt_esdf=bool(torch.equal(lat.view(torch.int32), dist_d.view(torch.int32))))
            del dist_d
        v.set_grid(torch.zeros(n, n, n, dtype=torch.uint8, device=dev), world.origin, world.res)
        v.build_esdf(plane=2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3): v.build_esdf(plane=2)
        e1.record(); torch.cuda.synchronize()
        row["build_empty_map_ms"] = e0.elapsed_time(e1) / 3
        print(json.dumps(row), flush=True)
        del lat, v
        torch.cuda.empty_cache()
    sys.exit(0)
n = 256
dist, origin = synth.sphere_esdf(n, 0.1, (0.0, 0.0, 0.0), 5.0)
v = Vigo(0)
dist_d = T(dist)
v.set_esdf(dist_d, origin, 0.1)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20): v.set_esdf(dist_d, origin, 0.1)
torch.cuda.synchronize()
print(json.dumps({"config": "5b: vigo_set_esdf, 256^3 (row-major lattice -> one 128-B line per 1x3x3 cells, 3.56x the bytes)", "ms": (time.perf_counter() - t0) / 20 * 1e3}))
rng = np.random.default_rng(5)
pts_h = rng.uniform(-12.7, 12.7, size=(1 << 20, 3))
idx = np.lexsort(tuple(np.floor((pts_h[:, a] + 12.8) / 0.4).astype(int) for a in (2, 1, 0)))
modes = ["f32"] if "--f32" in sys.argv else (["f64", "f32"] if "--both" in sys.argv else ["f64"])
for mode in modes:
    for name, p in (("uniform random", pts_h), ("brick-sorted", pts_h[idx])):
        if mode == "f32":
            pts = T(p.astype(np.float32))
            out = torch.empty(pts.shape[0], 4, dtype=torch.float32, device=dev)
            run = lambda: v.esdf_query_f32(pts, out)
        else:
            pts = T(p)
            run = lambda: v.esdf_query(pts)
        for _ in range(5): run()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(50): r = run()
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 50
        chk = float(r[:, 0].double().sum().item()) if mode == "f32" else float(r[0].sum().item())
        print(json.dumps({"config": f"5b: 1M trilinear ESDF queries, {name}, {mode} I/O", "ms": dt * 1e3, "queries_per_s": (1 << 20) / dt,
                          "algorithmic_GBps": (1 << 20) * 60 / dt / 1e9, "frac_of_hbm_peak": (1 << 20) * 60 / dt / 8e12, "checksum": chk}))
