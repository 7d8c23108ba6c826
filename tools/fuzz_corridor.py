"""Randomised parity sweep of vigo_corridor_check and vigo_box_collision_points against the oracle (bit for bit), drawn
from the families of tests/corridor_cases.py: its worlds (resolution 0.1 / 0.05, with and without interior metric
bounds), its box / map_resolution list plus random boxes from 0.1 to 1.3 m, degrees 3-9, ragged sample counts, boundary
huggers, fast and degenerate segments, non-finite coefficients and cancelling polynomials.

In the suite (tests/test_gpu_corridor_cases.py, with the routing census of tests/test_corridor_cases.py): the named,
seeded cases of those families, every route of k_corridor with a stated minimum, trajectory mode included.  What this
tool still adds: volume and fresh seeds — worlds, boxes and segments the suite has never seen, as many as asked for.
Not part of the test suite; run on the GPU box:  python tools/fuzz_corridor.py [cases] [seed]"""
import ctypes as C, json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import trajectory_planner_amd._lib as L
if os.environ.get("VIGO_EXP_LIB"):                      # dev: an alternative build of the library
    L.LIB_PATH = os.path.join(R, os.environ["VIGO_EXP_LIB"])
import numpy as np, torch
import corridor_cases as cc
import oracle_lib as ol
from gpu_util import to_dev
from corridor_restatement import segment_route
from trajectory_planner_amd.vigo import Vigo

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
rng = np.random.default_rng(seed)
O = ol.oracle()
bad = 0
t0 = time.time()
for case in range(cases):
    res = float(rng.choice([0.1, 0.05]))
    n = int(rng.choice([48, 96]))
    world = cc.make_world(f"fuzz {seed}/{case}", int(rng.integers(1 << 30)), n, int(rng.choice([24, 32, 40, 64])), res, bool(rng.random() < 0.3))
    v = Vigo(0)
    v.set_grid(to_dev(world.voxels, v.device), world.origin, world.res)
    g, keep = ol.make_grid(world)
    if world.bounds is not None:
        v.set_metric_bounds(*world.bounds); g.bmin[:] = list(world.bounds[0]); g.bmax[:] = list(world.bounds[1])
    if rng.random() < 0.5:
        _, box, map_res = cc.BOXES[int(rng.integers(len(cc.BOXES)))]
    else:
        box = tuple(rng.uniform(0.1, 1.3, size=3) * [1, 1, 0.5]); map_res = float(rng.choice([0.05, 0.1, 0.2, 0.25, 0.45]))
    lo, hi = cc._extent(world, box)
    if not (hi - lo > 0.2).all():                         # the box leaves no room for poses inside this world's bounds
        box, map_res = cc.CFG_BOX, cc.CFG_RES
    deg = int(rng.integers(3, 10)) if rng.random() < 0.6 else 7
    count = lambda: int(rng.choice([int(rng.integers(50, 1500)), int(rng.integers(1500, 6000)), int(rng.integers(6000, 20000))]))
    segs = [cc.smooth(rng, world, box, deg, k) for k in (0, 1, 17, 33, 511, 512, 513, 1025)]
    segs += [cc.smooth(rng, world, box, deg, count(), speed=float(rng.choice([0.1, 1.0, 40.0]))) for _ in range(6)]
    for a in range(3):
        for against in ("face", "bound", "rim"):
            segs.append(cc.hugger(rng, world, box, map_res, deg, count(), a, against, float(rng.choice([0.0, 1e-7, 1e-6, 2e-5, 1e-3])), bool(rng.random() < 0.5)))
    c, k, d = cc.smooth(rng, world, box, deg, 1500)
    c[int(rng.integers(0, 3)), int(rng.integers(0, deg + 1))] = float(rng.choice([np.nan, np.inf, -np.inf, 1e300, 1e39, -4e38, 1e20, 3.4028234e38]))
    segs.append((c, k, d))
    for f in (0.0, -1.0, 1e-9):                            # (the oracle and the device walk these clocks step by step)
        c, k, d = cc.smooth(rng, world, box, deg, int(rng.integers(100, 3000)))
        segs.append((c, k, d * f))
    segs.append(cc.cancelling(world, box, map_res, deg, count() + 2, float(rng.choice([1e-6, 1e-5, 1e-4])), 3.0, axis=int(rng.integers(0, 3)),
                              cell=int(rng.integers(4, world.voxels.shape[2] - 4))))
    coeffs = np.ascontiguousarray(np.stack([s[0] for s in segs])); n_samp = np.array([s[1] for s in segs], np.int32); delT = np.array([s[2] for s in segs])
    flag, first, count_ = (x.cpu().numpy() for x in v.corridor_check(to_dev(coeffs, v.device), to_dev(n_samp, v.device), to_dev(delT, v.device), box, map_res))
    with ol.pow_mode(True):
        rf, ri, rc = ol.corridor_check_batch(g, coeffs, n_samp, delT, np.array(box), map_res)
    ok = True
    for s in np.nonzero((flag != rf) | (first != ri) | (count_ != rc))[0]:
        ok = False
        route = segment_route(coeffs[s], int(n_samp[s]), float(delT[s]), box, map_res, world.grid)["route"]
        print(json.dumps({"segment": int(s), "n": int(n_samp[s]), "route": route, "oracle": [int(rf[s]), int(ri[s]), int(rc[s])],
                          "device": [int(flag[s]), int(first[s]), int(count_[s])]}), flush=True)
    # the per-pose sweep on random poses and on poses on faces, bounds and the rim
    half = n * res / 2
    pts = np.concatenate([rng.uniform(-half * 1.1, half * 1.1, size=(400, 3)) * [1, 1, 0.2] + [0, 0, 0.8], cc.face_poses(world, box, map_res, rng)])
    got = v.box_collision_points(to_dev(pts, v.device), box, map_res).cpu().numpy()
    bx = np.ascontiguousarray(box, dtype=np.float64)
    for i in range(len(pts)):
        ok = ok and got[i] == O.vgo_box_collision(C.byref(g), C.c_float(pts[i, 0]), C.c_float(pts[i, 1]), C.c_float(pts[i, 2]), ol._d(bx), C.c_double(map_res))
    if not ok:
        bad += 1
        print(json.dumps({"MISMATCH": case, "res": res, "box": list(box), "map_res": map_res, "deg": deg}), flush=True)
    v.close()
print(json.dumps({"cases": cases, "mismatches": bad, "seconds": time.time() - t0}))
sys.exit(1 if bad else 0)
