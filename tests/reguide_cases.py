"""Shared by tests/test_reguide_core.py (CPU) and tests/test_gpu_reguide.py: the workloads the re-guide step of the rebound
loop is run on — crafted trajectories on the small world of tests/pathsearch_cases.py with states made by hand, and a
batch derived from the pipeline workload's prologue by a seeded perturbation that imitates a solve — and ctypes wrappers
of the host entries (host/src/cabi_host.cpp: vigo_host_rebound_reguide_core = csrc/vigo_reguide_core.hpp around the
path-search and guide twins; vigo_host_reguide_facade = bsplineTraj::reboundStep itself; vigo_host_reguide_rules = the
header's rules on flags)."""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import guide_cases as gc
import pathsearch_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
DONE, SEARCH_FAILED, NOT_REQUIRED, DEFERRED, SKIPPED = 0, 1, 2, 3, 4          # VIGO_REGUIDE_*
RB_ACTIVE, RB_DONE, RB_NEEDS_HOST = 0, 1, 2
MAX_SEGS = 48
STATE_INTS = 8 + 2 * MAX_SEGS                                     # vigo_rebound_state_t as int32 columns
S_STATUS, S_SOLVE_FIRST, S_FAIL, S_GATE_STATIC, S_GATE_DYNAMIC, S_ROUNDS, S_LBFGS, S_NSEG, S_SEG = 0, 1, 2, 3, 4, 5, 6, 7, 8
CAP = 512                                                         # search_path_cap of these tests
_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)


def host_lib():
    lib = C.CDLL(LIB)
    head = [C.c_void_p, _ip, _dp, C.c_double, C.c_int, C.c_int, _dp]
    lib.vigo_host_rebound_reguide_core.argtypes = head + [_ip, _dp, _bp, _dp, C.c_double, C.c_double, C.c_double, _ip, C.c_double, C.c_double, C.c_int,
                                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_longlong, _ip, _dp, _bp,
                                                          C.c_longlong, C.c_longlong, _ip, _ip, _dp, _ip]
    lib.vigo_host_rebound_reguide_core.restype = C.c_int
    lib.vigo_host_reguide_facade.argtypes = head + [_ip, _dp, _dp, _dp, _ip, C.c_longlong, _ip, _dp, C.c_longlong, C.c_longlong, _ip, _ip, _dp, _ip]
    lib.vigo_host_reguide_facade.restype = C.c_int
    lib.vigo_host_reguide_rules.argtypes = [C.c_int, C.c_double, _bp, _bp, C.c_int, _ip, _bp, C.c_int, _ip, _bp, _ip]
    lib.vigo_host_reguide_rules.restype = C.c_int
    return lib


def make_state(B, segs=None, status=RB_NEEDS_HOST, gate_static=1, gate_dynamic=0, fail_count=0, fill=-3):
    """[B, STATE_INTS] int32; segs: per trajectory a list of (first, second).  The unused segment slots, rounds and
    lbfgs_status hold `fill`-like marks so that a write to them shows."""
    st = np.full((B, STATE_INTS), fill, dtype=np.int32)
    st[:, S_STATUS], st[:, S_SOLVE_FIRST], st[:, S_FAIL] = status, 0, fail_count
    st[:, S_GATE_STATIC], st[:, S_GATE_DYNAMIC], st[:, S_ROUNDS], st[:, S_LBFGS], st[:, S_NSEG] = gate_static, gate_dynamic, 2, -997, 0
    for b, sg in enumerate(segs or []):
        st[b, S_NSEG] = len(sg)
        for k, (f, s) in enumerate(sg[:MAX_SEGS]):
            st[b, S_SEG + 2 * k], st[b, S_SEG + 2 * k + 1] = f, s
    return st


@dataclass
class Case:
    name: str
    vox: np.ndarray
    origin: np.ndarray
    res: float
    cfg: np.ndarray          # distance_threshold, min_height, max_height, max_obstacle_size[3]
    ctrl: np.ndarray         # [B, N, 3]
    goff: np.ndarray         # int32 [B*N+1]
    gpv: np.ndarray          # [G, 6]
    weights: np.ndarray      # [B, 4]
    state: np.ndarray        # int32 [B, STATE_INTS]
    ncr: float = 0.0
    step: Optional[float] = None     # the searches' lattice step (default: the map's resolution)
    pool_: Optional[tuple] = None
    expect: Optional[int] = None     # crafted: the status under the shipped capacities

    @property
    def B(self):
        return self.ctrl.shape[0]

    @property
    def N(self):
        return self.ctrl.shape[1]

    @property
    def pool(self):
        return self.pool_ or tuple(2 * int(self.cfg[3 + a] / self.res) for a in range(3))

    def gunk(self):
        """isUnknown of the current guide points (bit 1 of the voxel byte; outside the grid unknown)"""
        p = self.gpv[:, :3]
        idx = np.floor((p - self.origin) / self.res)
        inside = ((idx >= 0) & (idx < np.array(self.vox.shape))).all(axis=1)
        i = np.clip(idx, 0, np.array(self.vox.shape) - 1).astype(int)
        return np.where(inside, (self.vox[i[:, 0], i[:, 1], i[:, 2]] >> 1) & 1, 1).astype(np.uint8)

    def subset(self, idx, name=None):
        idx = list(idx)
        N = self.N
        goff, rows = [0], []
        for b in idx:
            for i in range(N):
                rows.append(self.gpv[self.goff[b * N + i]:self.goff[b * N + i + 1]])
                goff.append(goff[-1] + len(rows[-1]))
        gpv = np.concatenate(rows).reshape(-1, 6) if rows else np.zeros((0, 6))
        return Case(name or self.name, self.vox, self.origin, self.res, self.cfg, np.ascontiguousarray(self.ctrl[idx]), np.array(goff, dtype=np.int32),
                    gpv, np.ascontiguousarray(self.weights[idx]), np.ascontiguousarray(self.state[idx]), self.ncr, self.step, self.pool_)


def concat(cases, name):
    """cases on ONE world as one batch"""
    c0 = cases[0]
    goff = [np.array([0], dtype=np.int64)]
    for c in cases:
        goff.append(c.goff[1:].astype(np.int64) + goff[-1][-1])
    return Case(name, c0.vox, c0.origin, c0.res, c0.cfg, np.concatenate([c.ctrl for c in cases]), np.concatenate(goff).astype(np.int32),
                np.concatenate([c.gpv.reshape(-1, 6) for c in cases]), np.concatenate([c.weights for c in cases]),
                np.concatenate([c.state for c in cases]), c0.ncr, c0.step, c0.pool_)


@dataclass
class Result:
    rc: int
    status: np.ndarray       # [B]  (the facade: need_optimize)
    state: np.ndarray
    weights: np.ndarray
    off: np.ndarray          # merged CSR
    pv: np.ndarray
    unk: Optional[np.ndarray]
    path_seg_off: np.ndarray
    path_off: np.ndarray
    path: np.ndarray
    raw: dict = field(default_factory=dict)      # the whole buffers (sentinel checks)

    def paths_of(self, b):
        k0, k1 = int(self.path_seg_off[b]), int(self.path_seg_off[b + 1])
        return [self.path[self.path_off[k]:self.path_off[k + 1]] for k in range(k0, k1)]

    def pairs_of(self, b, N):
        """per control point the (point, direction) rows"""
        return [self.pv[self.off[b * N + i]:self.off[b * N + i + 1]] for i in range(N)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def shipped():
    """the kernels' capacities: vigo_astar_capacity's table and heap, vigo_guide_capacity's path length"""
    d = pc.shipped()
    d["guide_path_cap"] = gc.capacity()
    return d


UNBOUNDED = dict(pc.UNBOUNDED, guide_path_cap=1 << 30)


def pair_room(c: Case):
    """the current pairs plus what a re-guide of every control point by every possible segment could append"""
    return len(c.gpv) + c.B * (c.N + 4 * MAX_SEGS) + 8


def _head(c: Case):
    keep = [np.ascontiguousarray(c.vox), np.ascontiguousarray(c.origin, dtype=np.float64), np.ascontiguousarray(c.ctrl, dtype=np.float64)]
    return keep, [keep[0].ctypes.data_as(C.c_void_p), (C.c_int * 3)(*c.vox.shape), keep[1].ctypes.data_as(_dp), float(c.res), c.B, c.N,
                  keep[2].ctypes.data_as(_dp)]


def _guides(c: Case, with_guides=True):
    if not with_guides:
        return [], None, None, None
    goff = np.ascontiguousarray(c.goff, dtype=np.int32)
    gpv = np.ascontiguousarray(np.concatenate([c.gpv.reshape(-1), np.zeros(6)]))
    gunk = np.ascontiguousarray(np.concatenate([c.gunk(), np.zeros(1, dtype=np.uint8)]))
    return [goff, gpv, gunk], goff.ctypes.data_as(_ip), gpv.ctypes.data_as(_dp), gunk.ctypes.data_as(_bp)


def twin(lib, c: Case, mode, cap, pair_cap=None, seg_cap=None, point_cap=None, fill=-7, with_guides=True, want_paths=True):
    """vigo_host_rebound_reguide_core -> Result; every output buffer pre-filled with `fill`"""
    keep, head = _head(c)
    keep2, p_goff, p_gpv, p_gunk = _guides(c, with_guides)
    pcap = pair_room(c) if pair_cap is None else pair_cap
    scap = c.B * MAX_SEGS if seg_cap is None else seg_cap
    ptcap = min(scap * (CAP + 1), 1 << 21) if point_cap is None else point_cap
    weights, state = np.ascontiguousarray(c.weights, dtype=np.float64).copy(), np.ascontiguousarray(c.state, dtype=np.int32).copy()
    off, pv = np.full(c.B * c.N + 1, fill, dtype=np.int32), np.full((max(pcap, 1), 6), float(fill))
    unk, status = np.full(max(pcap, 1), fill & 0xFF, dtype=np.uint8), np.full(max(c.B, 1), fill, dtype=np.int32)
    pso, po, pa = np.full(c.B + 1, fill, dtype=np.int32), np.full(max(scap, 0) + 1, fill, dtype=np.int32), np.full((max(ptcap, 1), 3), float(fill))
    step = c.res if c.step is None else c.step
    rc = lib.vigo_host_rebound_reguide_core(
        *head, p_goff, p_gpv, p_gunk, weights.ctypes.data_as(_dp), float(c.ncr), float(c.cfg[0]), float(step), (C.c_int * 3)(*c.pool), float(c.cfg[1]),
        float(c.cfg[2]), cap["cap_log2"], cap["max_nodes"], cap["heap_cap"], cap["max_expansions"], CAP, cap["guide_path_cap"], mode,
        state.ctypes.data_as(_ip), pcap, off.ctypes.data_as(_ip), pv.ctypes.data_as(_dp), unk.ctypes.data_as(_bp), scap, ptcap,
        pso.ctypes.data_as(_ip) if want_paths else None, po.ctypes.data_as(_ip) if want_paths else None, pa.ctypes.data_as(_dp) if want_paths else None,
        status.ctypes.data_as(_ip))
    raw = dict(off=off, pv=pv, unk=unk, status=status, path_seg_off=pso, path_off=po, path=pa, weights=weights, state=state)
    if rc != 0 or not c.B:
        return Result(rc, status[:c.B], state, weights, off, pv, unk, pso, po, pa, raw)
    G = int(off[-1])
    S = int(pso[c.B]) if want_paths else 0
    return Result(rc, status[:c.B], state, weights, off, pv[:G], unk[:G], pso, po[:S + 1], pa[:po[S]] if want_paths else pa[:0], raw)


def facade(lib, c: Case):
    """bsplineTraj::reboundStep(r, true, gate_dynamic, false) on the case's state -> Result (status: needOptimize)"""
    keep, head = _head(c)
    keep2, p_goff, p_gpv, _ = _guides(c)
    pcap, scap = pair_room(c), c.B * 64
    ptcap = scap * 2048
    weights, state = np.ascontiguousarray(c.weights, dtype=np.float64).copy(), np.ascontiguousarray(c.state, dtype=np.int32).copy()
    cfg = np.ascontiguousarray(c.cfg, dtype=np.float64)
    off, pv = np.zeros(c.B * c.N + 1, dtype=np.int32), np.zeros((pcap, 6))
    pso, po, pa, need = np.zeros(c.B + 1, dtype=np.int32), np.zeros(scap + 1, dtype=np.int32), np.zeros((ptcap, 3)), np.zeros(c.B, dtype=np.int32)
    rc = lib.vigo_host_reguide_facade(*head, p_goff, p_gpv, weights.ctypes.data_as(_dp), cfg.ctypes.data_as(_dp), state.ctypes.data_as(_ip), pcap,
                                      off.ctypes.data_as(_ip), pv.ctypes.data_as(_dp), scap, ptcap, pso.ctypes.data_as(_ip), po.ctypes.data_as(_ip),
                                      pa.ctypes.data_as(_dp), need.ctypes.data_as(_ip))
    assert rc == 0, rc
    S = int(pso[c.B])
    return Result(rc, need, state, weights, off, pv[:off[-1]], None, pso, po[:S + 1], pa[:po[S]])


def rules(lib, N, ncr, pt, ln, prev, need, cap=MAX_SEGS):
    """vigo_host_reguide_rules -> (n_new, seg [n, 2], listed [n])"""
    pt, ln, need = [np.ascontiguousarray(a, dtype=np.uint8) for a in (pt, ln, need)]
    prev = np.ascontiguousarray(np.array(prev, dtype=np.int32).reshape(-1))
    prev_p = np.concatenate([prev, np.zeros(2, dtype=np.int32)])
    seg, listed, n_list = np.zeros((cap, 2), dtype=np.int32), np.zeros(cap, dtype=np.uint8), C.c_int(0)
    n = lib.vigo_host_reguide_rules(N, float(ncr), pt.ctypes.data_as(_bp), ln.ctypes.data_as(_bp), len(prev) // 2, prev_p.ctypes.data_as(_ip),
                                    need.ctypes.data_as(_bp), cap, seg.ctypes.data_as(_ip), listed.ctypes.data_as(_bp), C.byref(n_list))
    if n > cap:
        return n, seg, None
    assert n_list.value == int(listed[:n].sum())
    return n, seg[:n], listed[:n]


# ---- crafted trajectories ---------------------------------------------------------------------------------------------
def _pairs(N, per_point):
    """per_point: {control point: [(point[3], direction[3]), ...]} -> (goff [N+1], gpv [G, 6])"""
    goff, rows = [0], []
    for i in range(N):
        for p, d in per_point.get(i, []):
            rows.append(np.concatenate([np.asarray(p, dtype=float), np.asarray(d, dtype=float)]))
        goff.append(len(rows))
    return np.array(goff, dtype=np.int32), (np.array(rows).reshape(-1, 6) if rows else np.zeros((0, 6)))


def _far(c, i):          # a guide 1 m to the side the control point is already past: dist = +1 >= dthresh
    return (c[i] - np.array([0.0, 1.0, 0.0]), np.array([0.0, 1.0, 0.0]))


def _near(c, i):         # a guide 0.6 m ahead: dist = -0.6, dthresh - dist > 0
    return (c[i] + np.array([0.0, 0.6, 0.0]), np.array([0.0, 1.0, 0.0]))


def crafted_cases():
    """-> [Case of ONE trajectory]: each has its own world (tests/pathsearch_cases.py) and a state made by hand; `expect` is
    the status under the shipped capacities"""
    worlds = dict(pc.crafted_workloads())
    out = []

    def add(name, world, expect, segs=(), pairs=None, weights=(1.0, 1.0, 1.0, 1.0), ncr=0.0, **st):
        w = worlds[world] if isinstance(world, str) else world
        c = w.ctrl[0]
        goff, gpv = _pairs(w.N, pairs(c) if pairs else {})
        out.append(Case(name, w.vox, w.origin, w.res, w.cfg, w.ctrl, goff, gpv, np.array([weights], dtype=np.float64),
                        make_state(1, [list(segs)], **st), ncr=ncr, expect=expect))

    block = "one block, one search"                       # control points 14 .. 17 inside: the scanned segment is (13, 18)
    add("a new segment no previous segment covers", block, DONE, segs=[(5, 8)])
    add("a covered segment whose guides are all beyond dthresh", block, DONE, segs=[(13, 18)],
        pairs=lambda c: {i: [_far(c, i)] for i in range(14, 18)})
    add("a covered segment with one guide inside dthresh", block, NOT_REQUIRED, segs=[(12, 19)],
        pairs=lambda c: {i: [_far(c, i), _near(c, i)] for i in range(13, 19)}, weights=(4.0, 1.0, 1.0, 1.0), fail_count=2)
    add("one covered control point without a near guide", block, DONE, segs=[(13, 18)],
        pairs=lambda c: {i: ([_near(c, i)] if i != 16 else [_far(c, i), _far(c, i)]) for i in range(14, 18)})
    add("previous segments empty", block, DONE)
    add("a line-only segment", "a line-only segment", DONE, segs=[(3, 5)])
    add("a line-only segment whose ends the previous segments hold, guides near", "a line-only segment", NOT_REQUIRED, segs=[(10, 13)],
        pairs=lambda c: {i: [_near(c, i)] for i in range(10, 14)})
    add("the endIdx - 1 duplicate", "the endIdx - 1 duplicate segment", None)
    add("a re-guide search that fails", "a failed last segment", SEARCH_FAILED, weights=(2.0, 1.0, 1.0, 1.0), fail_count=1)
    wall = "a failed last segment"                        # a wall across the world: control point 15 inside, segment (14, 16)
    add("a failed search of a covered segment whose guides are beyond dthresh", wall, SEARCH_FAILED, segs=[(14, 16)],
        pairs=lambda c: {15: [_far(c, 15)]})
    add("a failed search, the covered point far from both of its guides", wall, SEARCH_FAILED, segs=[(13, 18)],
        pairs=lambda c: {15: [_far(c, 15), _far(c, 15)], 16: [_near(c, 16)]}, fail_count=2, weights=(4.0, 2.0, 1.0, 1.0))
    add("a failed search with not_check_ratio 0.2", wall, SEARCH_FAILED, ncr=0.2)
    add("a failed first choice with gap > 2", "a failed first choice with gap > 2", SEARCH_FAILED, segs=[(20, 24)])
    add("a second choice that fails too", "a second choice that fails too", SEARCH_FAILED)
    add("a second choice that fails too, every point covered and near", "a second choice that fails too", NOT_REQUIRED, segs=[(3, 28)],
        pairs=lambda c: {i: [_near(c, i)] for i in range(3, 29)})
    add("a covered wall segment left out of the list, the block behind it re-guided", "a failed first choice with gap > 2", DONE, segs=[(8, 12)],
        pairs=lambda c: {i: [_near(c, i)] for i in range(8, 13)}, gate_dynamic=1)
    add("a covered block left out of the list, the wall before it fails", "a failed first choice with gap > 2", SEARCH_FAILED, segs=[(18, 21)],
        pairs=lambda c: {i: [_near(c, i)] for i in (19, 20)}, gate_dynamic=1)
    add("a merge taken inside the re-guide list", "a merge taken", DONE)
    add("a merge taken while another listed segment stays unmerged", "a merge taken while another segment stays unmerged", None)
    add("gate_dynamic set, re-guided", block, DONE, gate_dynamic=1, weights=(1.0, 1.0, 1.0, 8.0))
    add("gate_dynamic set, search failed", "a failed last segment", SEARCH_FAILED, gate_dynamic=1, fail_count=3)
    add("ineligible: fail_count == 4", block, SKIPPED, fail_count=4)
    add("ineligible: status ACTIVE", block, SKIPPED, status=RB_ACTIVE)
    add("ineligible: status DONE", block, SKIPPED, status=RB_DONE)
    add("ineligible: gate_static == 0", block, SKIPPED, gate_static=0, gate_dynamic=1)
    add("a control point that already carries 5 pairs", block, DONE, segs=[(13, 18)],
        pairs=lambda c: {15: [_far(c, 15)] * 5, 14: [_near(c, 14)], 16: [_near(c, 16)], 17: [_near(c, 17)]})
    add("no collision left: an empty list", "no segments", NOT_REQUIRED, segs=[(13, 18)])
    add("more than 48 new segments", pc.zigzag_workload(120), DEFERRED, segs=[(3, 9)])
    add("7 control points", _short_world(), NOT_REQUIRED)
    return out


def _short_world():
    """N = 7: endIdx = 3, the scan looks at control point 3 alone and can close no segment"""
    v = np.zeros((48, 48, 24), dtype=np.uint8)
    pc._block(v, -0.2, 0.2)
    c = np.zeros((7, 3))
    c[:, 0] = -0.42 + 0.14 * np.arange(7)
    c[:, 2] = 1.0
    return pc.Workload("7 control points", v, np.array([-2.4, -2.4, 0.0]), 0.1, np.ascontiguousarray(c[None]), pc.CRAFTED_CFG)


def long_path_case():
    """one segment whose path has more points than vigo_guide_capacity: a search on a lattice of a fifth of the map's
    resolution along a tunnel one voxel wide and high (the open set stays a few nodes wide, so the shipped table holds
    the search) — the path search succeeds, the guide step defers"""
    v = np.ones((48, 48, 24), dtype=np.uint8)
    v[2:46, 24, 10] = 0                                   # the tunnel: y in [0, 0.1), z in [1.0, 1.1), x from -2.2 to 2.2
    N = 32
    c = np.zeros((N, 3))
    c[:, 0] = -2.15 + 0.135 * np.arange(N)
    c[:, 1], c[:, 2] = 0.05, 1.05
    c[8:24, 1] = 0.25                                     # control points 8 .. 23 leave the tunnel sideways into the rock
    w = pc.Workload("long path", v, np.array([-2.4, -2.4, 0.0]), 0.1, np.ascontiguousarray(c[None]), np.array([0.5, 1.0, 1.1, 0.8, 0.8, 0.4]))
    goff, gpv = _pairs(N, {})
    return Case("a path longer than vigo_guide_capacity", w.vox, w.origin, w.res, w.cfg, w.ctrl, goff, gpv, np.ones((1, 4)),
                make_state(1, [[]]), step=0.005, pool_=(1000, 40, 40), expect=DEFERRED)


# ---- the derived batch ---------------------------------------------------------------------------------------------
DERIVED_SEED = 0x5EED0001


def derived_batch(n=128, N=32, seed=DERIVED_SEED):
    """n trajectories of guide_cases.pipeline_workload after the host prologue (segments by findCollisionSeg / pathSearch,
    guide pairs by the guide step with libm's atan2: what makePlanBatch holds when the loop starts), their control points
    moved by a seeded perturbation that imitates a solve: every guided point goes a fraction of the way to its first guide
    point; for a seeded subset a window of control points is shifted sideways, into the obstacles"""
    glib = gc.host_lib()
    w, world, status = gc.pipeline_workload(glib, n=n, N=N)
    rc, off, pv, unk, gst, _ = gc.core(glib, w, 0)
    assert rc == 0 and (gst == gc.OK).all()
    from trajectory_planner_amd import synth
    rng = np.random.default_rng(seed)
    ctrl = w.ctrl.copy()
    segs = []
    for b in range(n):
        segs.append([tuple(int(x) for x in s) for s in w.seg[w.seg_off[b]:w.seg_off[b + 1]]])
        frac = rng.uniform(0.3, 0.9)
        for i in range(N):
            if off[b * N + i + 1] > off[b * N + i]:
                ctrl[b, i] += frac * (pv[off[b * N + i], :3] - ctrl[b, i])
        if rng.random() < 0.55:
            i0 = int(rng.integers(4, N - 9))
            width = int(rng.integers(3, 7))
            t = ctrl[b, i0 + width] - ctrl[b, i0 - 1]
            side = np.array([-t[1], t[0], 0.0]) / max(np.hypot(t[0], t[1]), 1e-9)
            ctrl[b, i0:i0 + width] += side * rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 0.9)
    fail = (np.arange(n) % 4).astype(np.int32)
    st = make_state(n, segs, gate_dynamic=0)
    st[:, S_FAIL] = fail
    st[:, S_GATE_DYNAMIC] = (np.arange(n) % 5 == 0)
    weights = np.ones((n, 4))
    weights[:, 0] = 2.0 ** fail
    weights[:, 3] = 1.0 + (np.arange(n) % 3)
    return Case(f"derived batch, seed {seed:#x}", w.vox, w.origin, w.res, np.array(synth.PIPELINE_CFG, dtype=np.float64), np.ascontiguousarray(ctrl),
                off.astype(np.int32), pv.copy(), weights, st)


# ---- makePlanBatch under setDeviceReguide (needs a GPU) --------------------------------------------------------------
def pipeline_paths(P, N=32, seed=11):
    """P straight jittered paths of N - 2 poses with free ends on the pipeline world (synth.make_pipeline_batch's candidates,
    plannable or not)"""
    from trajectory_planner_amd import synth
    world = synth.make_pipeline_world()
    rng = np.random.default_rng(seed)
    K = N - 2
    s = np.arange(K) * synth.CTRL_SPACING
    out = []
    while sum(len(x) for x in out) < P:
        M = 2 * P
        start = np.concatenate([rng.uniform(-8.0, 8.0, size=(M, 2)), np.full((M, 1), 1.0)], axis=1)
        heading = rng.uniform(0.0, 2 * np.pi, size=M)
        dirv = np.stack([np.cos(heading), np.sin(heading), np.zeros(M)], axis=1)
        lat = np.stack([-np.sin(heading), np.cos(heading), np.zeros(M)], axis=1)
        pts = start[:, None, :] + s[None, :, None] * dirv[:, None, :] + rng.normal(0.0, 0.05, size=(M, K, 1)) * lat[:, None, :]
        out.append(pts[(synth.lookup(world, pts[:, 0], 0) == 0) & (synth.lookup(world, pts[:, -1], 0) == 0)])
    return world, np.ascontiguousarray(np.concatenate(out)[:P])


SLOT_TWIN, SLOT_DEVICE, SLOT_HOST, SLOT_UNTOUCHED = 0, 1, 2, 3    # setDeviceReguide(2), (1), (0), never called


def plan_batch_reguide(P, slots=0b111, budget=16384, reps=1):
    """P planners of the pipeline world: SLOT_UNTOUCHED once, first, then `reps` rounds over the slots of `slots` (bit k: slot
    k runs) among the first three; twin: the re-guide steps SLOT_TWIN's last run logged, and how many of them the kernels'
    host twin decides under the shipped capacities -> dict of per-slot arrays"""
    import plan_batch as pb
    world, pts = pipeline_paths(P)
    cap = shipped()
    r = pb.plan_batch(world, *pb.uniform_paths(pts), [(m, budget, pb.BY_CALL) for m in (pb.REGUIDE2, pb.REGUIDE1, 0)] + [(0, budget, pb.UNTOUCHED)],
                      [SLOT_UNTOUCHED] + [s for s in range(3) if (slots >> s) & 1] * reps, outputs=("ok", "solver", "ncp", "ctrl", "segs", "paths", "guides"),
                      replay_slot=SLOT_TWIN if slots & 1 else -1, caps=[cap[k] for k in ("cap_log2", "max_nodes", "heap_cap", "guide_path_cap")], ncp_cap=64, lib=LIB)
    return dict(total_ms=r["slot_seconds"][:, :, 2] * 1e3, counts=pb.stat(r, "reguideDecided", "reguideHost"), twin=r["twin"], switches=r["switches"],
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_seg", "segs", "n_path_pts", "paths", "n_guides", "guides")})
