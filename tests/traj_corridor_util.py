"""Shared by tests/test_gpu_traj_corridor.py and tests/test_gpu_corridor_cases.py: the five rules of
vigo_traj_corridor_check (include/vigo.h) restated in Python over the oracle's own sampler (vgo_poly_pos) and box sweep
(vgo_box_collision), and the CSR packing of trajectories for the entry."""
import ctypes as C
import math

import numpy as np

import oracle_lib as ol
from gpu_util import to_dev
from trajectory_planner_amd._lib import load

BOX = np.array([0.4, 0.4, 0.2])
RES = 0.2


def restate(g, seg_off, coeffs, knots, delT, endpoint, nonfinite, exact=True, device_sweep=None, box=BOX, map_res=RES):
    """The five rules in Python: (status, n, flag, first, count, seg mask).  Statuses other than 0 come from
    vigo_traj_sample_runs (pinned against the literal loop by tests/test_traj_runs.py): the loop cannot run there.
    exact=False, device_sweep=Vigo: the facade's present route instead (libm pow, vigo_box_collision_points).
    box, map_res: the collision box and map_resolution of the sweep (default: the cfg values)."""
    O = ol.oracle()
    T = len(seg_off) - 1
    S, _, d1 = coeffs.shape
    deg = d1 - 1
    out = dict(status=np.zeros(T, np.int32), n=np.zeros(T, np.int32), flag=np.zeros(T, np.uint8),
               first=np.full(T, -1, np.int32), count=np.zeros(T, np.int32), seg=np.zeros(S, np.uint8))
    box = np.ascontiguousarray(box, dtype=np.float64)
    map_res = float(map_res)
    default_hit = None                                         # the sweep at the default pose, once per call
    p = np.zeros(3)
    with ol.pow_mode(exact):
        for t in range(T):
            a, b = int(seg_off[t]), int(seg_off[t + 1])
            K = b - a
            k = [float(x) for x in knots[a + t:a + t + K + 1]]
            d = float(delT[t])
            st = runs_status(k, d)
            out["status"][t] = st
            if st:
                continue
            poses, segs = [], []
            tt = 0.0
            while tt < k[-1]:                                  # rule 1
                if tt < k[0]:                                  # (before the first knot: no segment, the default pose)
                    poses.append((0.0, 0.0, 0.0))
                    segs.append(-1)
                    tt += d
                    continue
                s = next((i for i in range(K) if k[i] <= tt <= k[i + 1]), -1)   # rule 2
                if s < 0:
                    poses.append((0.0, 0.0, 0.0))
                else:
                    c = np.ascontiguousarray(coeffs[a + s])
                    O.vgo_poly_pos(deg, ol._d(c[0]), ol._d(c[1]), ol._d(c[2]), tt - k[s], ol._d(p))
                    poses.append(tuple(p))
                segs.append(s)
                tt += d
            poses.append(tuple(float(x) for x in endpoint[t]))   # rule 3
            segs.append(next((i for i in range(K) if k[i] <= tt <= k[i + 1]), -1))
            if device_sweep is not None:
                hit = device_sweep.box_collision_points(to_dev(np.array(poses), device_sweep.device), box, map_res).cpu().numpy()
            else:
                if default_hit is None:
                    default_hit = O.vgo_box_collision(C.byref(g), 0.0, 0.0, 0.0, ol._d(box), map_res)
                hit = [default_hit if s < 0 else O.vgo_box_collision(C.byref(g), q[0], q[1], q[2], ol._d(box), map_res)
                       for q, s in zip(poses[:-1], segs[:-1])]   # rule 4 (a sample outside every segment is the default pose)
                q = poses[-1]
                hit.append(O.vgo_box_collision(C.byref(g), q[0], q[1], q[2], ol._d(box), map_res))
            first, count = -1, 0
            for j, (q, s) in enumerate(zip(poses, segs)):
                h = bool(hit[j]) or (nonfinite and not all(math.isfinite(x) for x in q))
                if h:
                    count += 1
                    first = j if first < 0 else first
                    if s >= 0:
                        out["seg"][a + s] = 1                  # rule 5
            out["n"][t] = len(poses)
            out["flag"][t] = count > 0
            out["first"][t] = first
            out["count"][t] = count
    return out


def runs_status(k, d):
    kk = np.ascontiguousarray(k, dtype=np.float64)
    K = len(kk) - 1
    buf = np.zeros(max(K, 1), np.int32)
    n = C.c_int32()
    return load().vigo_traj_sample_runs(K, kk.ctypes.data_as(C.c_void_p), float(d), buf.ctypes.data_as(C.c_void_p),
                                        buf.ctypes.data_as(C.c_void_p), C.byref(n))


def pack(trajs):
    """[(knots, coeffs [K,3,d+1], delT, endpoint)] -> the entry's CSR layout"""
    seg_off = np.cumsum([0] + [len(c) for _, c, _, _ in trajs]).astype(np.int32)
    coeffs = np.concatenate([c for _, c, _, _ in trajs]) if seg_off[-1] else np.zeros((0, 3, 8))
    knots = np.concatenate([np.asarray(k, np.float64) for k, _, _, _ in trajs])
    delT = np.array([d for _, _, d, _ in trajs], np.float64)
    endpoint = np.array([e for _, _, _, e in trajs], np.float64)
    return seg_off, np.ascontiguousarray(coeffs, dtype=np.float64), knots, delT, endpoint
