"""Shared by tests/test_guide_core.py (CPU) and tests/test_gpu_guides.py: the workloads the guide assignment is run on —
the prologue of the pipeline batch (segments and paths by the host pipeline: vigo_host_prologue_paths), a second seed,
and crafted trajectories (a two-point path, line-collision segments at the clip bounds 3 and N - 4, a segment ending at
N - 1, a path shortcutPath cannot shorten, one it shortens to its ends, failed searches including the very first, a zero
diff, a path longer than the device buffer) — and ctypes wrappers of the host entries (host/src/cabi_host.cpp:
vigo_host_guide_core = csrc/vigo_guide_core.hpp compiled for the host, vigo_host_guide_facade = the facade's own
assignGuidePointsSemiCircle, vigo_host_atan2)."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
OK, DEFERRED = 0, 1
_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)


def host_lib():
    lib = C.CDLL(LIB)
    head = [C.c_void_p, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp]
    lib.vigo_host_guide_core.argtypes = head + [_ip, _ip, _ip, _dp, C.c_int, C.c_int, C.c_longlong, _ip, _dp, _bp, _ip, _ip]
    lib.vigo_host_guide_core.restype = C.c_int
    lib.vigo_host_guide_facade.argtypes = head + [_ip, _ip, _ip, _dp, C.c_longlong, _ip, _dp]
    lib.vigo_host_guide_facade.restype = C.c_int
    lib.vigo_host_prologue_paths.argtypes = head + [_dp, C.c_int, C.c_longlong, _ip, _ip, _ip, _ip, _dp]
    lib.vigo_host_prologue_paths.restype = C.c_int
    lib.vigo_host_atan2.argtypes = [C.c_longlong, _dp, _dp, _dp]
    lib.vigo_host_atan2.restype = C.c_int
    return lib


def capacity():
    """the longest path vigo_guide_assign holds (vigo_guide_capacity)"""
    from trajectory_planner_amd import _lib
    n = C.c_int32(0)
    assert _lib.load().vigo_guide_capacity(C.byref(n)) == 0
    return n.value


@dataclass
class Workload:
    name: str
    vox: np.ndarray          # uint8 [nx, ny, nz]: bit 0 inflated-occupied, bit 1 unknown
    origin: np.ndarray
    res: float
    ctrl: np.ndarray         # [B, N, 3]
    seg_off: np.ndarray      # int32 [B + 1]
    seg: np.ndarray          # int32 [S, 2]
    path_off: np.ndarray     # int32 [S + 1]
    path: np.ndarray         # [P, 3]

    @property
    def B(self):
        return self.ctrl.shape[0]

    @property
    def N(self):
        return self.ctrl.shape[1]

    def subset(self, idx, name=None):
        """the trajectories idx, in that order"""
        seg_off, seg, path_off, path = [0], [], [0], []
        for b in idx:
            for k in range(self.seg_off[b], self.seg_off[b + 1]):
                seg.append(self.seg[k])
                path.append(self.path[self.path_off[k]:self.path_off[k + 1]])
                path_off.append(path_off[-1] + len(path[-1]))
            seg_off.append(len(seg))
        return Workload(name or self.name, self.vox, self.origin, self.res, np.ascontiguousarray(self.ctrl[list(idx)]),
                        np.array(seg_off, dtype=np.int32), np.array(seg, dtype=np.int32).reshape(-1, 2),
                        np.array(path_off, dtype=np.int32), np.concatenate(path).reshape(-1, 3) if path else np.zeros((0, 3)))

    def pairs_of(self, off, b):
        return slice(int(off[b * self.N]), int(off[(b + 1) * self.N]))


def _head(w: Workload):
    vox = np.ascontiguousarray(w.vox)
    keep = [vox, np.ascontiguousarray(w.origin, dtype=np.float64), np.ascontiguousarray(w.ctrl, dtype=np.float64),
            np.ascontiguousarray(w.seg_off, dtype=np.int32), np.ascontiguousarray(w.seg, dtype=np.int32).reshape(-1),
            np.ascontiguousarray(w.path_off, dtype=np.int32), np.ascontiguousarray(w.path, dtype=np.float64).reshape(-1)]
    # (empty arrays still need a valid pointer)
    keep = [k if k.size else np.zeros(4, dtype=k.dtype) for k in keep]
    args = [keep[0].ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), keep[1].ctypes.data_as(_dp), float(w.res), w.B, w.N,
            keep[2].ctypes.data_as(_dp), keep[3].ctypes.data_as(_ip), keep[4].ctypes.data_as(_ip), keep[5].ctypes.data_as(_ip),
            keep[6].ctypes.data_as(_dp)]
    return keep, args


def pair_count(w: Workload):
    """the pairs of the workload when nothing is deferred: interior points one each, a segment without one up to four"""
    n = 0
    for f, s in w.seg:
        n += max(0, min(s, w.N) - max(f + 1, 0))
        if s - f == 1:
            n += max(0, min(s + 1, w.N - 4) - max(f - 1, 3) + 1)
    return n


def core(lib, w: Workload, mode, path_cap=1 << 30, pair_cap=None, fill=-7.0):
    """vigo_host_guide_core -> (rc, off [B*N+1], pv [G,6], unk [G], status [B], decision [G,3]); buffers pre-filled with `fill`"""
    cap = pair_count(w) + 8 if pair_cap is None else pair_cap
    keep, args = _head(w)
    off = np.full(w.B * w.N + 1, -7, dtype=np.int32)
    pv = np.full((max(cap, 1), 6), fill)
    unk = np.full(max(cap, 1), 7, dtype=np.uint8)
    status = np.full(max(w.B, 1), -7, dtype=np.int32)
    dec = np.full((max(cap, 1), 3), -7, dtype=np.int32)
    rc = lib.vigo_host_guide_core(*args, mode, path_cap, cap, off.ctypes.data_as(_ip), pv.ctypes.data_as(_dp), unk.ctypes.data_as(_bp),
                                  status.ctypes.data_as(_ip), dec.ctypes.data_as(_ip))
    if rc != 0:
        return rc, off, pv, unk, status, dec
    g = int(off[-1]) if w.B else 0
    return rc, off, pv[:g], unk[:g], status[:w.B], dec[:g]


def facade(lib, w: Workload):
    """the facade's assignGuidePointsSemiCircle on the same inputs -> (off [B*N+1], pv [G,6])"""
    cap = pair_count(w) + 8
    keep, args = _head(w)
    off, pv = np.zeros(w.B * w.N + 1, dtype=np.int32), np.zeros((cap, 6))
    rc = lib.vigo_host_guide_facade(*args, cap, off.ctypes.data_as(_ip), pv.ctypes.data_as(_dp))
    assert rc == 0, rc
    return off, pv[:off[-1]]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def pipeline_workload(lib, seed=None, n=1024, N=32):
    """the prologue of synth.make_pipeline_batch(make_pipeline_world(), n, N, seed): segments and paths by the host pipeline"""
    from trajectory_planner_amd import synth
    world = synth.make_pipeline_world()
    seed = synth.SEED_BASE + 2 + 2000 if seed is None else seed
    b = synth.make_pipeline_batch(world, n, N, seed)
    vox = np.ascontiguousarray(world.voxels)
    origin = np.ascontiguousarray(world.origin, dtype=np.float64)
    cfg = np.ascontiguousarray(synth.PIPELINE_CFG, dtype=np.float64)
    ctrl = np.ascontiguousarray(b.ctrl, dtype=np.float64)
    seg_cap, pt_cap = 8 * n, 1024 * n
    status, seg_off = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int32)
    seg, path_off, path = np.zeros((seg_cap, 2), dtype=np.int32), np.zeros(seg_cap + 1, dtype=np.int32), np.zeros((pt_cap, 3))
    rc = lib.vigo_host_prologue_paths(vox.ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), origin.ctypes.data_as(_dp), float(world.res), n, N,
                                      ctrl.ctypes.data_as(_dp), cfg.ctypes.data_as(_dp), seg_cap, pt_cap, status.ctypes.data_as(_ip),
                                      seg_off.ctypes.data_as(_ip), seg.ctypes.data_as(_ip), path_off.ctypes.data_as(_ip), path.ctypes.data_as(_dp))
    assert rc == 0, rc
    S = int(seg_off[-1])
    w = Workload(f"pipeline batch, seed {seed:#x}", vox, origin, float(world.res), ctrl, seg_off, seg[:S].copy(), path_off[:S + 1].copy(),
                 path[:path_off[S]].copy())
    return w, world, status


# ---- crafted trajectories ---------------------------------------------------------------------------------------------
CRAFTED_N = 32


def crafted_world():
    """a 4.8 m x 4.8 m x 2.4 m grid at 0.1 m with a wall x in [-0.2, 0.2], y in [-1.6, 1.6]; the voxels at x > 1.6 unknown"""
    vox = np.zeros((48, 48, 24), dtype=np.uint8)
    vox[22:26, 8:40, :] |= 1
    vox[40:, :, :] |= 2
    return vox, np.array([-2.4, -2.4, 0.0]), 0.1


def _line_ctrl(y=0.0, x0=-2.17, dx=0.14, N=CRAFTED_N):
    c = np.zeros((N, 3))
    c[:, 0] = x0 + dx * np.arange(N)
    c[:, 1] = y
    c[:, 2] = 1.0
    return c


def crafted_workload(long_path=300):
    """one trajectory per case; names[b] says which"""
    vox, origin, res = crafted_world()
    N = CRAFTED_N
    names, ctrls, segs, paths = [], [], [], []

    def add(name, ctrl, seg_list, path_list):
        names.append(name)
        ctrls.append(ctrl)
        segs.append(seg_list)
        paths.append([np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in path_list])

    def detour(c, f, s, side=1.0, n=9):
        """ctrl[f] -> an arc over the wall's end on the given side -> ctrl[s], ctrl[s] appended (as pathSearch leaves it)"""
        a, b = c[f], c[s]
        t = np.linspace(0.0, 1.0, n)[:, None]
        p = a + t * (b - a)
        p[:, 1] += side * 1.9 * np.sin(np.pi * t[:, 0])
        return np.concatenate([p, b[None, :]])

    c = _line_ctrl()
    add("straight two-point path", c, [(10, 14)], [[c[10], c[14]]])
    mid = lambda f, s, dy: (c[f] + c[s]) / 2 + np.array([0.0, dy, 0.0])
    add("line collisions at the clip bounds", c, [(3, 4), (N - 5, N - 4), (2, 3), (N - 4, N - 3)],
        [[c[3], mid(3, 4, 0.3), c[4]], [c[N - 5], mid(N - 5, N - 4, -0.3), c[N - 4]], [c[2], mid(2, 3, 0.2), c[3]],
         [c[N - 4], mid(N - 4, N - 3, 0.2), c[N - 3]]])
    add("segment ending at N - 1", c, [(N - 7, N - 1)], [detour(c, N - 7, N - 1, n=7)])
    hug = [(-0.4, 0.0, 1.0), (-0.4, 1.8, 1.0), (0.4, 1.8, 1.0), (0.4, 0.0, 1.0)]
    c2 = _line_ctrl()
    c2[13], c2[19] = hug[0], hug[-1]
    add("a path shortcutPath cannot shorten", c2, [(13, 19)], [hug])
    zig = np.stack([np.linspace(-2.0, -0.6, 20), -2.0 + 0.15 * (np.arange(20) % 2), np.ones(20)], axis=1)
    c3 = _line_ctrl(y=-2.0)
    c3[2], c3[12] = zig[0], zig[-1]
    add("a path shortened to its ends", c3, [(2, 12)], [zig])
    add("detours on both sides, several segments", c, [(8, 13), (14, 20), (21, 22)],
        [detour(c, 8, 13), detour(c, 14, 20, side=-1.0, n=17), [c[21], mid(21, 22, 0.25), c[22]]])
    c4 = _line_ctrl()
    c4[5] = 0.0                                                  # guidePoint (still zero) - controlPoint = 0: a NaN direction
    add("failed searches: the very first, a zero diff, a stale guide point", c4, [(4, 7), (9, 13), (14, 17), (20, 21)],
        [[c4[4]], detour(c4, 9, 13), [c4[14]], [c4[20]]])
    lp = np.stack([np.linspace(-2.2, 2.2, long_path), np.full(long_path, -2.1), np.ones(long_path)], axis=1)
    c5 = _line_ctrl(y=-2.1)
    add("a path longer than the device buffer", c5, [(6, 10), (12, 18)], [detour(c5, 6, 10), lp])
    add("no segments", c, [], [])
    add("detour after the long one", c, [(8, 13)], [detour(c, 8, 13, side=-1.0)])
    seg_off, seg, path_off, path = [0], [], [0], []
    for sl, pl in zip(segs, paths):
        for s, p in zip(sl, pl):
            seg.append(s)
            path.append(p)
            path_off.append(path_off[-1] + len(p))
        seg_off.append(len(seg))
    w = Workload("crafted", vox, origin, res, np.ascontiguousarray(np.stack(ctrls)), np.array(seg_off, dtype=np.int32),
                 np.array(seg, dtype=np.int32).reshape(-1, 2), np.array(path_off, dtype=np.int32), np.concatenate(path))
    return w, names
