"""Shared by tests/test_pathsearch_core.py (CPU) and tests/test_gpu_pathsearch.py: the workloads findCollisionSeg and
pathSearch are run on — the two pipeline batches of tests/guide_cases.py and crafted trajectories on a small world with
a 16 x 16 x 8 node pool (an exhausted search stays inside the kernels' first table, so "not found" is decided) — and
ctypes wrappers of the host entries (host/src/cabi_host.cpp: vigo_host_path_search_core / vigo_host_collision_segs_core =
csrc/vigo_pathsearch_core.hpp compiled for the host around the device's search core; vigo_host_prologue_paths = the
facade's own findCollisionSeg -> pathSearch)."""
import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
OK, FAILED, DEFERRED = 0, 1, 2
MAX_SEGS = 48                                                     # VIGO_MAX_COLLISION_SEGS
UNBOUNDED = dict(cap_log2=20, max_nodes=(1 << 20) - 1, heap_cap=1 << 20, max_expansions=1 << 30)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def shipped():
    """the kernels' capacities (vigo_astar_capacity: the 8192-slot table of the second pass)"""
    from trajectory_planner_amd import _lib
    n, h = C.c_int32(0), C.c_int32(0)
    assert _lib.load().vigo_astar_capacity(C.byref(n), C.byref(h)) == 0
    return dict(cap_log2=13, max_nodes=n.value, heap_cap=h.value, max_expansions=1 << 30)


def host_lib():
    lib = C.CDLL(LIB)
    head = [C.c_void_p, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp]
    lib.vigo_host_path_search_core.argtypes = head + [_ip, _ip, C.c_double, C.c_double, _ip, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_longlong, C.c_longlong, _ip, _ip, _ip, _ip, _dp, _ip]
    lib.vigo_host_path_search_core.restype = C.c_int
    lib.vigo_host_collision_segs_core.argtypes = head + [C.c_double, C.c_longlong, _ip, _ip, _ip]
    lib.vigo_host_collision_segs_core.restype = C.c_int
    lib.vigo_host_prologue_paths.argtypes = head + [_dp, C.c_int, C.c_longlong, _ip, _ip, _ip, _ip, _dp]
    lib.vigo_host_prologue_paths.restype = C.c_int
    return lib


@dataclass
class Workload:
    name: str
    vox: np.ndarray          # uint8 [nx, ny, nz], bit 0 = inflated-occupied
    origin: np.ndarray
    res: float
    ctrl: np.ndarray         # [B, N, 3]
    cfg: np.ndarray          # distance_threshold, min_height, max_height, max_obstacle_size[3] (the facade's parameters)
    seg_off: Optional[np.ndarray] = None     # a supplied segment list, or None: the scanned segments
    seg: Optional[np.ndarray] = None
    ncr: float = 0.0

    @property
    def B(self):
        return self.ctrl.shape[0]

    @property
    def N(self):
        return self.ctrl.shape[1]

    @property
    def pool(self):
        return tuple(2 * int(self.cfg[3 + a] / self.res) for a in range(3))           # setMap, BT.cpp:187-195

    def subset(self, idx):
        seg_off = seg = None
        if self.seg_off is not None:
            seg_off, rows = [0], []
            for b in idx:
                rows.append(self.seg[self.seg_off[b]:self.seg_off[b + 1]])
                seg_off.append(seg_off[-1] + len(rows[-1]))
            seg_off, seg = np.array(seg_off, dtype=np.int32), np.concatenate(rows).reshape(-1, 2).astype(np.int32)
        return Workload(self.name, self.vox, self.origin, self.res, np.ascontiguousarray(self.ctrl[list(idx)]), self.cfg, seg_off, seg, self.ncr)


@dataclass
class Result:
    rc: int
    status: np.ndarray
    seg_off: np.ndarray
    seg: np.ndarray          # [S, 2]
    path_off: np.ndarray     # [S + 1]
    path: np.ndarray         # [P, 3]
    counts: np.ndarray       # [B, 2]

    def of(self, b):
        """trajectory b: (status, segments, [paths])"""
        k0, k1 = int(self.seg_off[b]), int(self.seg_off[b + 1])
        return int(self.status[b]), self.seg[k0:k1], [self.path[self.path_off[k]:self.path_off[k + 1]] for k in range(k0, k1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a: Result, b: Result):
    return (np.array_equal(a.status, b.status) and np.array_equal(a.seg_off, b.seg_off) and np.array_equal(a.seg, b.seg) and
            np.array_equal(a.path_off, b.path_off) and a.path.shape == b.path.shape and np.array_equal(bits(a.path), bits(b.path)))


def _head(w: Workload):
    keep = [np.ascontiguousarray(w.vox), np.ascontiguousarray(w.origin, dtype=np.float64), np.ascontiguousarray(w.ctrl, dtype=np.float64)]
    return keep, [keep[0].ctypes.data_as(C.c_void_p), (C.c_int * 3)(*w.vox.shape), keep[1].ctypes.data_as(_dp), float(w.res), w.B, w.N,
                  keep[2].ctypes.data_as(_dp)]


def caps(w: Workload, search_path_cap):
    seg_cap = max(w.B * MAX_SEGS, 1)
    return seg_cap, min(seg_cap * (search_path_cap + 1), 1 << 22)


def twin(lib, w: Workload, cap=None, search_path_cap=512, seg_cap=None, point_cap=None, fill=-7):
    """vigo_host_path_search_core under the capacities `cap` (default UNBOUNDED) -> Result; buffers pre-filled"""
    cap = dict(UNBOUNDED) if cap is None else cap
    keep, head = _head(w)
    sc, pc = caps(w, search_path_cap)
    sc, pc = (sc if seg_cap is None else seg_cap), (pc if point_cap is None else point_cap)
    status, seg_off = np.full(max(w.B, 1), fill, dtype=np.int32), np.full(w.B + 1, fill, dtype=np.int32)
    seg, path_off = np.full((max(sc, 1), 2), fill, dtype=np.int32), np.full(max(sc, 0) + 1, fill, dtype=np.int32)
    path, counts = np.full((max(pc, 1), 3), float(fill)), np.full((max(w.B, 1), 2), fill, dtype=np.int32)
    so = None if w.seg_off is None else np.ascontiguousarray(w.seg_off, dtype=np.int32)
    sg = None if w.seg is None else np.ascontiguousarray(np.concatenate([w.seg.reshape(-1), np.zeros(2, dtype=np.int32)]), dtype=np.int32)
    rc = lib.vigo_host_path_search_core(*head, None if so is None else so.ctypes.data_as(_ip), None if sg is None else sg.ctypes.data_as(_ip), float(w.ncr),
                                        float(w.res), (C.c_int * 3)(*w.pool), float(w.cfg[1]), float(w.cfg[2]), cap["cap_log2"], cap["max_nodes"],
                                        cap["heap_cap"], cap["max_expansions"], search_path_cap, sc, pc, status.ctypes.data_as(_ip),
                                        seg_off.ctypes.data_as(_ip), seg.ctypes.data_as(_ip), path_off.ctypes.data_as(_ip), path.ctypes.data_as(_dp),
                                        counts.ctypes.data_as(_ip))
    if rc != 0:
        return Result(rc, status, seg_off, seg, path_off, path, counts)
    S = int(seg_off[w.B])
    return Result(rc, status[:w.B], seg_off, seg[:S].copy(), path_off[:S + 1].copy(), path[:path_off[S]].copy(), counts[:w.B])


def twin_segments(lib, w: Workload, seg_cap=None):
    """vigo_host_collision_segs_core -> (rc, seg_off, seg [S, 2], status)"""
    keep, head = _head(w)
    sc = w.B * MAX_SEGS if seg_cap is None else seg_cap
    seg_off, seg, status = np.full(w.B + 1, -7, dtype=np.int32), np.full((max(sc, 1), 2), -7, dtype=np.int32), np.full(max(w.B, 1), -7, dtype=np.int32)
    rc = lib.vigo_host_collision_segs_core(*head, float(w.ncr), sc, seg_off.ctypes.data_as(_ip), seg.ctypes.data_as(_ip), status.ctypes.data_as(_ip))
    if rc != 0:
        return rc, seg_off, seg, status
    return rc, seg_off, seg[:seg_off[w.B]].copy(), status[:w.B]


def facade(lib, w: Workload):
    """the facade's own findCollisionSeg -> pathSearch (vigo_host_prologue_paths) as a Result: a failed trajectory is
    FAILED and owns nothing"""
    assert w.seg_off is None and w.ncr == 0.0
    keep, head = _head(w)
    cfg = np.ascontiguousarray(w.cfg, dtype=np.float64)
    seg_cap, pt_cap = 64 * w.B, 2048 * w.B
    status, seg_off = np.zeros(w.B, dtype=np.int32), np.zeros(w.B + 1, dtype=np.int32)
    seg, path_off, path = np.zeros((seg_cap, 2), dtype=np.int32), np.zeros(seg_cap + 1, dtype=np.int32), np.zeros((pt_cap, 3))
    rc = lib.vigo_host_prologue_paths(*head, cfg.ctypes.data_as(_dp), seg_cap, pt_cap, status.ctypes.data_as(_ip), seg_off.ctypes.data_as(_ip),
                                      seg.ctypes.data_as(_ip), path_off.ctypes.data_as(_ip), path.ctypes.data_as(_dp))
    assert rc == 0, rc
    S = int(seg_off[-1])
    return Result(0, np.where(status == -2, FAILED, OK).astype(np.int32), seg_off, seg[:S].copy(), path_off[:S + 1].copy(), path[:path_off[S]].copy(),
                  np.zeros((w.B, 2), dtype=np.int32))


def pipeline_workload(seed=None, n=1024, N=32):
    """the control points of guide_cases.pipeline_workload's batch on the pipeline world"""
    from trajectory_planner_amd import synth
    world = synth.make_pipeline_world()
    seed = synth.SEED_BASE + 2 + 2000 if seed is None else seed
    b = synth.make_pipeline_batch(world, n, N, seed)
    return Workload(f"pipeline batch, seed {seed:#x}", np.ascontiguousarray(world.voxels), np.ascontiguousarray(world.origin, dtype=np.float64),
                    float(world.res), np.ascontiguousarray(b.ctrl, dtype=np.float64), np.array(synth.PIPELINE_CFG, dtype=np.float64))


# ---- crafted trajectories ---------------------------------------------------------------------------------------------
CRAFTED_N = 32
CRAFTED_CFG = np.array([0.5, 0.7, 1.3, 0.8, 0.8, 0.4])            # a 16 x 16 x 8 node pool at 0.1 m


def _line(gaps=None, x0=-2.17, N=CRAFTED_N):
    """control points along y = 0, z = 1, 0.14 m apart (`gaps`: index -> the spacing before that point)"""
    d = np.full(N, 0.14)
    d[0] = 0.0
    for i, g in (gaps or {}).items():
        d[i] = g
    c = np.zeros((N, 3))
    c[:, 0] = x0 + np.cumsum(d)
    c[:, 2] = 1.0
    return c


def _vi(x):
    return int(np.floor((x + 2.4) / 0.1 + 1e-9))


def _block(vox, x0, x1, y0=-0.3, y1=0.3):
    vox[_vi(x0):_vi(x1), _vi(y0):_vi(y1), :] |= 1


def _wall(vox, x0, x1):
    vox[_vi(x0):_vi(x1), :, :] |= 1


def _cage(vox, cx):
    """a closed box of two-voxel walls around the 0.2 m x 0.2 m free cell at (cx, 0)"""
    _block(vox, cx - 0.3, cx + 0.3)
    vox[_vi(cx - 0.1):_vi(cx + 0.1), _vi(-0.1):_vi(0.1), :] &= 0xFE


def crafted_workloads():
    """-> [(name, Workload of ONE trajectory)]: each case has its own world"""
    origin, res = np.array([-2.4, -2.4, 0.0]), 0.1
    empty = lambda: np.zeros((48, 48, 24), dtype=np.uint8)
    out = []

    def add(name, vox, ctrl, **kw):
        out.append((name, Workload(name, vox, origin, res, np.ascontiguousarray(ctrl[None]), CRAFTED_CFG, **kw)))

    c = _line()
    add("no segments", empty(), c)
    v = empty(); _block(v, -0.2, 0.2)
    add("one block, one search", v, c)
    v = empty(); _wall(v, -0.2, 0.0)
    add("a failed last segment", v, c)
    v = empty(); _cage(v, 0.0)
    add("a merge taken", v, c)
    v = empty(); _block(v, -1.4, -1.1); _cage(v, 0.5)
    add("a merge taken while another segment stays unmerged", v, c)
    v = empty(); _wall(v, -1.0, -0.8); _block(v, 0.4, 0.7)
    add("a failed first choice with gap > 2", v, c)
    v = empty(); _cage(v, 0.0); _wall(v, 0.1, 0.3)
    add("a second choice that fails too", v, c)
    v = empty(); _block(v, c[27, 0] - 0.1, c[27, 0] + 0.1, -0.2, 0.2)
    add("the endIdx - 1 duplicate segment", v, c)
    c2 = _line(gaps={12: 0.28}, x0=-2.3)
    v = empty(); v[_vi(c2[11, 0] + 0.1), _vi(-0.1):_vi(0.1), :] |= 1
    add("a line-only segment", v, c2)
    v = empty(); _block(v, -0.2, 0.2)
    add("a supplied list that differs from the scanned one", v, c, seg_off=np.array([0, 2], dtype=np.int32),
        seg=np.array([[13, 19], [20, 22]], dtype=np.int32))
    add("a supplied list of more than VIGO_MAX_COLLISION_SEGS segments", empty(), c, seg_off=np.array([0, MAX_SEGS + 1], dtype=np.int32),
        seg=np.tile(np.array([[5, 7]], dtype=np.int32), (MAX_SEGS + 1, 1)))
    return out


def zigzag_workload(N=120):
    """one trajectory that alternates between an occupied and a free spot: more than VIGO_MAX_COLLISION_SEGS scanned segments"""
    v = np.zeros((48, 48, 24), dtype=np.uint8)
    _block(v, -0.2, 0.2)
    c = np.zeros((N, 3))
    c[:, 2] = 1.0
    c[0::2, 0] = -0.6
    return Workload("zigzag", v, np.array([-2.4, -2.4, 0.0]), 0.1, np.ascontiguousarray(c[None]), CRAFTED_CFG)
