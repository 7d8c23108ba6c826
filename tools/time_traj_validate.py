"""Times plan validation on the config-2 world (256^3): 1024 and 16 384 held plans over ten control-point counts (8 .. 46, the
counts of tests/test_gpu_mixed_facade.py), half of them with two dynamic obstacles, gate step 0.025 s, ratio 0.
  (a) one vigo_traj_validate on the rows padded to the largest count, list included
  (b) the route to the same flags before it: per distinct count, vigo_traj_collision + vigo_traj_dynamic_collision on that
      count's rows, kept contiguous per count in advance (20 launches for ten counts; no position, no list)
  (c) 1024 planners through the facade: isCurrTrajValidBatch against the per-planner loop (isCurrTrajValid(pos) +
      hasDynamicCollisionTrajectory), wall clock, by vigo_host_validate_batch
(a) and (b) alternate inside one process: 3 warm-ups, then 20 repeats of each in turn, each repeat a device-event window
around 10 calls (the figure is per call).  Before timing, (a)'s flags are held against (b)'s.  One JSON line per size with
median / min / max / std in ms; `--out FILE` appends them there too.  Run on the GPU box."""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np, torch
from trajectory_planner_amd import _lib, synth
from trajectory_planner_amd.vigo import Vigo
dev = torch.device("cuda", 0)
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
WARM, REPS, CALLS, DT = 3, 20, 10, 0.025
COUNTS = (8, 10, 12, 16, 20, 24, 30, 34, 40, 46)
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [1024, 16384]


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return dict(median=float(np.median(ms)), min=float(ms.min()), max=float(ms.max()), std=float(ms.std()))


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS


def held_plans(world, B, seed):
    """straight jittered rows, control points 0.25 m apart at z = 1 inside the map -> ctrl [B, 46, 3] (zero padded), n_pts,
    and per row two obstacles (one on the row's middle, one far away) for every second row"""
    rng = np.random.default_rng(seed)
    n_pts = np.array([COUNTS[b % len(COUNTS)] for b in range(B)], dtype=np.int32)
    half = -float(world.origin[0]) - 0.3
    heading = rng.uniform(0.0, 2 * np.pi, size=B)
    length = (n_pts - 1) * synth.CTRL_SPACING
    dirv = np.stack([np.cos(heading), np.sin(heading), np.zeros(B)], axis=1)
    centre = np.concatenate([rng.uniform(-1.0, 1.0, size=(B, 2)) * (half - length[:, None] / 2), np.full((B, 1), 1.0)], axis=1)
    s = (np.arange(max(COUNTS))[None, :] - (n_pts[:, None] - 1) / 2) * synth.CTRL_SPACING
    ctrl = centre[:, None, :] + s[:, :, None] * dirv[:, None, :] + rng.normal(0.0, 0.02, size=(B, max(COUNTS), 3)) * [1, 1, 0]
    ctrl[np.arange(max(COUNTS))[None, :] >= n_pts[:, None]] = 0.0
    lists = [[[*centre[b], 0, 0, 0, 0.6, 0.6, 1.0], [90.0, 90.0, 1.0, 0, 0, 0, 0.6, 0.6, 1.0]] if b % 2 == 0 else [] for b in range(B)]
    return ctrl, n_pts, lists


def csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    return off, np.array([o for l in lists for o in l], dtype=np.float64).reshape(-1, 9)


world = synth.make_box_world(synth.SEED_BASE + 2, n=256, keep_ids=False)
v = Vigo(0)
v.set_grid(T(world.voxels), world.origin, world.res)
for B in sizes:
    ctrl, n_pts, lists = held_plans(world, B, 4100 + B)
    off, obs = csr(lists)
    d_ctrl, d_n, d_off, d_obs = T(ctrl), T(n_pts), T(off), T(obs)
    groups = []
    for n in COUNTS:
        rows = np.flatnonzero(n_pts == n)
        goff, gobs = csr([lists[b] for b in rows])
        groups.append((rows, T(ctrl[rows, :n]), T(goff), T(gobs)))
    one = lambda: v.traj_validate(d_ctrl, DT, n_pts=d_n, obs_off=d_off, obs=d_obs)

    def per_count():
        return [(v.traj_collision(c, DT), v.traj_dynamic_collision(c, DT, obs_off=o, obs=ob)) for _, c, o, ob in groups]
    r = one()
    status = r["status"].cpu().numpy()
    for (rows, *_), ((flag, first), dyn) in zip(groups, per_count()):
        assert np.array_equal(flag.cpu().numpy(), status[rows] & 1) and np.array_equal(first.cpu().numpy(), r["first"].cpu().numpy()[rows])
        assert np.array_equal(dyn.cpu().numpy(), (status[rows] >> 1) & 1)
    assert np.array_equal(np.flatnonzero(status), r["invalid"].cpu().numpy()[:int(r["n_invalid"][0])])
    ms = {"validate_one_call": [], "gates_per_count": []}
    for rep in range(WARM + REPS):
        for k, fn in (("validate_one_call", one), ("gates_per_count", per_count)):
            t = events(fn)
            if rep >= WARM:
                ms[k].append(t)
    row = {"config": f"plan validation, 256^3 box world, {B} held plans over counts {list(COUNTS)}, dt {DT}, ratio 0, every second plan with 2 obstacles",
           "build_id": _lib.load().vigo_build_id().decode(), "plans": B, "invalid": int((status != 0).sum()), "static": int((status & 1).sum()),
           "dynamic": int(((status >> 1) & 1).sum()), "launches": {"validate_one_call": 2, "gates_per_count": 2 * len(COUNTS)},
           "ms": {k: stats(t) for k, t in ms.items()}}
    if B == 1024:
        # (c) the facade on as many planners: pose lists of count - 2 poses each (the fit adds two control points)
        from test_gpu_validate_facade import validate_batch
        import mixed_cases as mc
        poff, pxyz = mc.pose_lists(world, [COUNTS[t % len(COUNTS)] - 2 for t in range(B)])
        f = validate_batch(world, poff, pxyz, reps=WARM + 7)
        assert np.array_equal(f["valid"][0], f["valid"][1]) and f["stats"].tolist() == [B, 0, 1]
        row["facade"] = {"planners": B, "valid": int(f["valid"][0].sum()), "device_groups": int(f["stats"][2]),
                         "ms": {"isCurrTrajValidBatch": stats(f["ms"][WARM:, 0]), "per_planner_loop": stats(f["ms"][WARM:, 1])}}
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")
