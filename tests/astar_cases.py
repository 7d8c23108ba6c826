"""Shared by tests/test_astar_core.py (CPU) and tests/test_gpu_astar.py: the A* searches both are run on — the random
worlds of tests/test_astar_restatement.py, crafted cases (equal-f ties, the ends' push-out, ends outside the pool, an
enclosed goal) and every prologue search of the pipeline batch — and ctypes wrappers of the host entries
(host/src/cabi_host.cpp: vigo_host_astar_stats = the facade's host A*, vigo_host_astar_core = the device's search core
compiled for the host, vigo_host_prologue_searches)."""
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from test_astar_restatement import _random_case

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
FOUND, NOT_FOUND, DEFERRED, PATH_TOO_LONG = 0, 1, 2, 3
UNBOUNDED = dict(cap_log2=20, max_nodes=(1 << 20) - 1, heap_cap=1 << 20, max_expansions=1 << 30)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def host_lib():
    lib = C.CDLL(LIB)
    head = [C.c_void_p, _ip, _dp, C.c_double, _ip, C.c_double, C.c_double, C.c_double, _dp, _dp]
    lib.vigo_host_astar_stats.argtypes = head + [_dp, C.c_int, _ip]
    lib.vigo_host_astar_stats.restype = C.c_int
    lib.vigo_host_astar_core.argtypes = head + [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _ip, _ip]
    lib.vigo_host_astar_core.restype = C.c_int
    lib.vigo_host_prologue_searches.argtypes = [C.c_void_p, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_int, _dp, _ip, _ip,
                                                _dp, _ip, _ip]
    lib.vigo_host_prologue_searches.restype = C.c_int
    return lib


@dataclass
class Case:
    name: str
    vox: np.ndarray          # uint8 [nx, ny, nz], bit 0 = inflated-occupied
    origin: np.ndarray
    res: float
    pool: tuple
    min_h: float
    max_h: float
    step: float
    start: np.ndarray
    end: np.ndarray


def _head(c: Case):
    vox = np.ascontiguousarray(c.vox)
    return vox, [vox.ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), (C.c_double * 3)(*c.origin), c.res, (C.c_int * 3)(*c.pool), c.min_h,
                 c.max_h, c.step, (C.c_double * 3)(*c.start), (C.c_double * 3)(*c.end)]


def host_astar(lib, c: Case, cap=4096):
    """the facade's host A* -> (path [n, 3] or None, stats: pops, reached, heap peak, rewrites, pushed)"""
    vox, head = _head(c)
    out, stats = np.zeros((cap, 3)), np.zeros(5, dtype=np.int32)
    n = lib.vigo_host_astar_stats(*head, out.ctypes.data_as(_dp), cap, stats.ctypes.data_as(_ip))
    assert n != -2
    return (out[:n].copy() if n >= 0 else None), stats


def core_astar(lib, c: Case, cap_log2, max_nodes, heap_cap, max_expansions, path_cap=4096):
    """the device's search core on the host -> (status, path or None, stats: pops, pushed, heap peak, rewrites, path buffer)"""
    vox, head = _head(c)
    out, stats, n = np.full((path_cap, 3), -7.0), np.zeros(4, dtype=np.int32), C.c_int(0)
    st = lib.vigo_host_astar_core(*head, cap_log2, max_nodes, heap_cap, max_expansions, path_cap, out.ctypes.data_as(_dp), C.byref(n),
                                  stats.ctypes.data_as(_ip))
    return st, (out[:n.value].copy() if st == FOUND else None), stats, out


def restatement_cases(seeds=range(3), per_seed=8):
    out = []
    for seed in seeds:
        rng = np.random.default_rng(100 + seed)
        for k in range(per_seed):
            vox, origin, s, e = _random_case(rng)
            out.append(Case(f"random {seed}/{k}", vox, origin, 0.1, (40, 40, 40), 0.7, 1.3, 0.1, s, e))
    return out


def crafted_cases():
    origin = np.array([-2.4, -2.4, 0.0])
    empty = np.zeros((48, 48, 24), dtype=np.uint8)
    mk = lambda name, vox, s, e, pool=(40, 40, 40), band=(0.7, 1.3): Case(name, vox, origin, 0.1, pool, band[0], band[1], 0.1, np.array(s, float),
                                                                          np.array(e, float))
    out = [mk("ties: axis-aligned, empty world", empty, (-1.0, 0.0, 1.0), (1.0, 0.0, 1.0)),
           mk("ties: diagonal, empty world", empty, (-0.8, -0.8, 1.0), (0.8, 0.8, 1.0)),
           mk("ties: start == end", empty, (0.3, 0.3, 1.0), (0.3, 0.3, 1.0))]
    wall = empty.copy()
    wall[22:26, 8:40, :] |= 1                                   # a wall across the straight line: a detour with rewrites
    out.append(mk("wall: detour", wall, (-1.2, 0.05, 1.0), (1.2, -0.05, 1.0)))
    out.append(mk("start inside the wall (pushed out)", wall, (0.0, 0.0, 1.0), (1.5, 0.3, 1.0)))
    out.append(mk("end inside the wall (pushed out)", wall, (-1.5, 0.3, 1.0), (0.0, 0.1, 1.0)))
    out.append(mk("both ends inside obstacles", wall, (-0.1, -0.5, 1.0), (0.12, 0.6, 1.0)))
    out.append(mk("ends outside the pool", empty, (-2.2, 0.0, 1.0), (2.2, 0.0, 1.0), pool=(20, 20, 20)))
    out.append(mk("start pushed out of the pool", wall, (0.0, 0.0, 1.0), (0.3, 0.0, 1.0), pool=(6, 6, 6)))
    cage = empty.copy()
    cage[30:37, 20:27, :] |= 1
    cage[31:36, 21:26, :] &= 0xFE                                # a free room whose walls are closed: the goal is unreachable
    # (a 30 x 30 x 20 pool: the exhausted search pushes fewer nodes than the device table holds; in the 40^3 pool it pushes more)
    out.append(mk("enclosed goal (open set exhausted)", cage, (-1.0, 0.0, 1.0), (0.95, -0.05, 1.0), pool=(30, 30, 20)))
    out.append(mk("enclosed goal, larger pool", cage, (-1.0, 0.0, 1.0), (0.95, -0.05, 1.0)))
    out.append(mk("narrow height band", wall, (-1.2, 0.0, 1.0), (1.2, 0.0, 1.0), band=(0.95, 1.05)))
    out.append(mk("tall band, near the map's edge", wall, (-2.3, -2.3, 0.5), (-1.0, -2.0, 1.5), band=(0.0, 3.0)))
    return out


def pipeline_searches(lib, n=1024, N=32, seed=None, path_cap=512):
    """every first-choice prologue search of synth.make_pipeline_batch(make_pipeline_world(), n, N, seed), by the host A*:
    (world, pool, ends [Q, 6], len [Q] (-1 = not found), path [Q, path_cap, 3], stats [Q, 5])"""
    from trajectory_planner_amd import synth
    world = synth.make_pipeline_world()
    b = synth.make_pipeline_batch(world, n, N, synth.SEED_BASE + 2 + 2000 if seed is None else seed)
    vox = np.ascontiguousarray(world.voxels)
    origin = np.ascontiguousarray(world.origin, dtype=np.float64)
    cfg = np.ascontiguousarray(synth.PIPELINE_CFG, dtype=np.float64)
    ctrl = np.ascontiguousarray(b.ctrl)
    cap = 8 * n
    ends, owner, ln = np.zeros((cap, 6)), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    path, stats, pool = np.zeros((cap, path_cap, 3)), np.zeros((cap, 5), dtype=np.int32), np.zeros(3, dtype=np.int32)
    q = lib.vigo_host_prologue_searches(vox.ctypes.data_as(C.c_void_p), (C.c_int * 3)(*vox.shape), origin.ctypes.data_as(_dp), float(world.res), n, N,
                                        ctrl.ctypes.data_as(_dp), cfg.ctypes.data_as(_dp), cap, path_cap, ends.ctypes.data_as(_dp),
                                        owner.ctypes.data_as(_ip), ln.ctypes.data_as(_ip), path.ctypes.data_as(_dp), stats.ctypes.data_as(_ip),
                                        pool.ctypes.data_as(_ip))
    assert 0 < q <= cap
    return world, tuple(int(v) for v in pool), ends[:q].copy(), ln[:q].copy(), path[:q].copy(), stats[:q].copy()
