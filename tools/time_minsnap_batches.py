#!/usr/bin/env python3
"""Wall time of the two min-snap makePlanBatch calls: secs_out[0] of vigo_host_poly_plan_batch_ex (32 polyTrajOctomap
planners) and vigo_host_occ_plan_batch (24 polyTrajOccMap planners, corridors) on the first pillar-world workloads of
tests/test_gpu_poly_batch.py / tests/test_gpu_occmap_batch.py, with the host library given by --lib (A/B of two builds:
one process per run, alternating).  Each entry is called once untimed first (HIP start-up, code-object load), then once
for the figure; batch and solo twins must agree.  Prints one JSON line.  Needs a GPU.
(profiles/README.md, "Host facades", holds a run of this.)"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(R, "tests")); sys.path.insert(0, R)
ap = argparse.ArgumentParser(); ap.add_argument("--lib", required=True); ap.add_argument("--tag", required=True)
a = ap.parse_args()
import test_gpu_poly_batch as pb
import test_gpu_occmap_batch as ob
from test_occmap_planner import cfg_vec
pb.LIB = ob.LIB = os.path.abspath(a.lib)
import ctypes as C
_dp = C.POINTER(C.c_double)

def poly():
    vox, origin, res = pb.pillar_world(1)
    rng = np.random.default_rng(101)
    paths = pb.random_paths(rng, 32, [-5, -5, 0.8], [5, 5, 1.6])
    modes = list(rng.integers(0, 2, size=32))
    tr, info, str_, sinfo, secs = pb.plan_batch(vox, origin, res, paths, modes, pb.CFG)
    assert np.array_equal(info[:, :3], sinfo[:, :3])
    return secs[0], int(info[:, 0].sum())

def occ():
    # ob.plan_batch does not return secs: the same call with the secs array kept
    rng = np.random.default_rng(41)
    vox = ob.pillar_world(1)
    paths = ob.random_paths(rng, 24)
    cfgs = [cfg_vec(maximum_iteration_num=int(rng.integers(2, 10)), shrinking_factor=0.75) for _ in paths]
    conds = rng.uniform(-0.4, 0.4, size=(len(paths), 4, 3)); conds[::3] = 0.0
    L = C.CDLL(ob.LIB)
    L.vigo_host_occ_plan_batch.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, ob._ip, _dp, _dp, _dp,
                                           C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]
    Pn = len(paths)
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
    wp = np.ascontiguousarray(np.concatenate(paths), dtype=np.float64)
    cf = np.ascontiguousarray(cfgs, dtype=np.float64); cd = np.ascontiguousarray(conds, dtype=np.float64)
    v = np.ascontiguousarray(vox)
    tr, info, str_, sinfo, secs = np.zeros((Pn, ob.CAP, 3)), np.zeros((Pn, 5)), np.zeros((Pn, ob.CAP, 3)), np.zeros((Pn, 5)), np.zeros(2)
    D = lambda x: x.ctypes.data_as(_dp)
    rc = L.vigo_host_occ_plan_batch(*v.shape, D(ob.ORIGIN), ob.RES, v.ctypes.data_as(C.c_void_p), Pn, off.ctypes.data_as(ob._ip), D(wp),
                                    D(cf), D(cd), 1, ob.CAP, D(tr), D(info), D(str_), D(sinfo), D(secs))
    assert rc == 0 and np.array_equal(info[:, :3], sinfo[:, :3])
    return secs[0], int(info[:, 0].sum())

poly(); occ()
p, pv = poly(); o, ov = occ()
print(json.dumps({"lib": a.tag, "poly_batch_ms": round(p * 1e3, 3), "poly_valid": pv, "occ_batch_ms": round(o * 1e3, 3), "occ_valid": ov}), flush=True)
