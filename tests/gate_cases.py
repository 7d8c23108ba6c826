"""Shared by tests/test_gate_cases.py (CPU: every case is about what its name says), tests/test_gpu_gate_cases.py (device
against oracle, through the map entry points and through the rebound loop) and tools/fuzz_map_gates.py: the named,
seeded edge cases of the map kernels (csrc/vigo_map.hip) and the walks of csrc/vigo_grid.hpp and
csrc/vigo_pathsearch_core.hpp.  numpy and the CPU oracle only; no GPU, no torch.

  A  first_hit_cases    the static gate's first index: one marked voxel per trajectory at a sample known in advance,
                        samples either side of the 64-lane stride, pairs whose earlier sample sits on the higher lane
  B  clock_cases        the sample count: the only occupied voxel is the one of the last sample, on clocks that end on
                        tmax bit for bit or whose next step passes it by a few ulp
  C  eval_cases         vigo_bspline_eval over ts_ctrl and N at every knot, one ulp either side, and the clamps
  D  nonfinite_case     one NaN / inf / 1e300 coordinate per trajectory: outside the map is occupied, no dynamic hit
  E  dynamic_cases      obstacle lists (empty, shared, copies, none) and the edges of the hit test
  F  occupancy_cases    vigo_ctrl_occupancy: trajectories across block borders and walls, the line walk's step count
  G  lookup_cases       point lookups on parity worlds, points on voxel faces and one ulp either side
  H  inflate_cases      vigo_inflate_grid against dilate_reference
  R  ratio_case         not_check_ratio = 1/3 in the rebound loop: the last sample the static gate looks at

A gate case holds its world, ts_ctrl, N, dt, control points, obstacle lists and, where construction fixes it, the
expected result (exp_* fields; None: the oracle alone says)."""
import ctypes as C
from dataclasses import dataclass, field
from functools import lru_cache
from typing import Optional

import numpy as np

import oracle_lib as ol

RESOLUTIONS = (0.13, 0.1, 0.05, 0.2)                    # G's (res, origin) pairs: off, on, off, on the lattice
TS_CTRL = (0.05, 0.07, 0.1, 0.2, 0.25, 1.0 / 3.0, 1.0)  # C's knot spacings
EVAL_N = (4, 5, 7, 8, 33, 64, 65, 256)
# (ts_ctrl, N, dt) -> T, the sample count of `for (t = 0; t <= (N - 3) * ts_ctrl; t += dt)`
FIRST_HIT_SHAPES = ((0.2, 19, 0.05, 65), (0.2, 38, 0.11, 64), (0.1, 24, 0.1 / 3, 63), (1.0 / 3.0, 12, 0.05, 61),
                    (0.25, 20, 0.1 / 3, 128), (0.2, 35, 0.05, 129))
CLOCK_EXACT = ((0.2, 14, 0.05, 45), (0.2, 10, 0.1, 15))                         # t_{T-1} == tmax
CLOCK_OVERSHOOT = ((0.2, 7, 0.05, 16), (0.2, 8, 0.025, 40), (0.2, 8, 0.01, 100))  # t_T - tmax <= 4 ulp
GATE_DT = tuple(sorted({s[2] for s in FIRST_HIT_SHAPES + CLOCK_EXACT + CLOCK_OVERSHOOT}))
GATE_N = tuple(sorted({s[1] for s in FIRST_HIT_SHAPES + CLOCK_EXACT + CLOCK_OVERSHOOT}))
LOOKUP_SHAPES = ((1, 2, 1), (2, 1, 31), (40, 33, 32), (33, 40, 33), (2, 96, 64), (96, 1, 65), (48, 48, 95))
NONFINITE = (np.nan, np.inf, -np.inf, 1e300, -1e300)


@dataclass
class World:
    voxels: np.ndarray                      # uint8 [nx, ny, nz]: bit 0 inflated-occupied, bit 1 unknown, bit 2 occupied
    origin: np.ndarray
    res: float
    boxes: Optional[np.ndarray] = None      # (the layout of synth.World)


@dataclass
class GateCase:
    name: str
    world: World
    ts_ctrl: float
    N: int
    dt: float
    ctrl: np.ndarray                        # [B, N, 3]
    T: Optional[int] = None                 # the sample count the name promises
    marks: list = field(default_factory=list)       # per trajectory: the samples whose voxels are occupied
    obs_off: Optional[np.ndarray] = None    # int32 [B + 1]; None with obs: the list is shared
    obs: Optional[np.ndarray] = None        # [O, 9]
    exp_flag: Optional[np.ndarray] = None   # static gate
    exp_first: Optional[np.ndarray] = None
    exp_dyn: Optional[np.ndarray] = None    # dynamic gate
    exp_pt: Optional[np.ndarray] = None     # vigo_ctrl_occupancy
    exp_line: Optional[np.ndarray] = None
    ncr: float = 0.0                        # not_check_ratio (rebound loop only)
    notes: dict = field(default_factory=dict)

    @property
    def family(self):
        return self.name.split(":")[0]

    @property
    def B(self):
        return self.ctrl.shape[0]

    def obs_of(self, b):
        """trajectory b's obstacles [n, 9]"""
        if self.obs is None:
            return np.zeros((0, 9))
        if self.obs_off is None:
            return np.ascontiguousarray(self.obs)
        return np.ascontiguousarray(self.obs[self.obs_off[b]:self.obs_off[b + 1]])


# ---- the oracle's view of a case -------------------------------------------------------------------------------------
def duration(N, ts):
    return (N - 3) * ts


def sample_times(tmax, dt):
    """t_k of `for (t = 0; t <= tmax; t += dt)`"""
    O = ol.oracle()
    n = O.vgo_sample_times(float(tmax), float(dt), None, 0)
    t = np.zeros(n)
    O.vgo_sample_times(float(tmax), float(dt), ol._d(t), n)
    return t


def positions(ctrl_b, ts, times, deriv=0):
    O = ol.oracle()
    c = np.ascontiguousarray(ctrl_b, dtype=np.float64)
    out = np.zeros((len(times), 3))
    for k, t in enumerate(times):
        O.vgo_traj_eval(c.shape[0], ol._d(c), float(ts), int(deriv), float(t), ol._d(out[k]))
    return out


def voxel_of(world, p):
    """posToIndex in fp64: floor((p - origin) / res)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((np.asarray(p, dtype=np.float64) - world.origin) / world.res)


def oracle_static(case):
    O = ol.oracle()
    g, keep = ol.make_grid(case.world)
    flag, first = np.zeros(case.B, dtype=np.uint8), np.zeros(case.B, dtype=np.int32)
    for b in range(case.B):
        c = np.ascontiguousarray(case.ctrl[b])
        fi = C.c_int()
        flag[b] = O.vgo_traj_collision(C.byref(g), case.N, ol._d(c), case.ts_ctrl, case.dt, C.byref(fi))
        first[b] = fi.value
    return flag, first


def oracle_dynamic(case):
    O = ol.oracle()
    out = np.zeros(case.B, dtype=np.uint8)
    for b in range(case.B):
        c, o = np.ascontiguousarray(case.ctrl[b]), case.obs_of(b)
        out[b] = O.vgo_traj_dynamic_collision(case.N, ol._d(c), case.ts_ctrl, case.dt, len(o), ol._d(o) if len(o) else None)
    return out


def oracle_occupancy(world, ctrl):
    O = ol.oracle()
    g, keep = ol.make_grid(world)
    B, N = ctrl.shape[:2]
    pt, line = np.zeros((B, N), dtype=np.uint8), np.zeros((B, N), dtype=np.uint8)
    for b in range(B):
        c = np.ascontiguousarray(ctrl[b])
        O.vgo_ctrl_occupancy(C.byref(g), N, ol._d(c), ol._u(pt[b]), ol._u(line[b]))
    return pt, line


def oracle_line(world, q, p):
    g, keep = ol.make_grid(world)
    return ol.oracle().vgo_is_inflated_occupied_line(C.byref(g), ol._d(np.ascontiguousarray(q, dtype=np.float64)),
                                                     ol._d(np.ascontiguousarray(p, dtype=np.float64)))


def oracle_lookup(world, pts, bit):
    O = ol.oracle()
    g, keep = ol.make_grid(world)
    fn = O.vgo_is_inflated_occupied if bit == 0 else O.vgo_is_unknown
    p = np.ascontiguousarray(pts, dtype=np.float64)
    return np.array([fn(C.byref(g), ol._d(p[i])) for i in range(len(p))], dtype=np.uint8)


def numpy_lookup(world, pts, bit, reciprocal=False):
    """the contract of include/vigo.h in numpy: the voxel's bit, 1 outside the box (a coordinate that is not finite is
    outside).  reciprocal: the index from (p - origin) * (1 / res), which the lookups must NOT compute."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.asarray(pts, dtype=np.float64) - world.origin
        f = np.floor(d * (1.0 / world.res)) if reciprocal else np.floor(d / world.res)
    n = np.array(world.voxels.shape)
    inside = np.all((f >= 0) & (f < n), axis=-1)            # (NaN compares false)
    ic = np.where(inside[..., None], f, 0).astype(np.int64)
    v = (world.voxels[ic[..., 0], ic[..., 1], ic[..., 2]] >> bit) & 1
    return np.where(inside, v, 1).astype(np.uint8)


# ---- straight trajectories whose consecutive samples lie in different voxels ------------------------------------------
def empty_world(shape, res, origin):
    return World(np.zeros(shape, dtype=np.uint8), np.array(origin, dtype=np.float64), float(res))


def diagonal_batch(world, ts, N, dt, B, per_sample=0.55, lateral=0):
    """B trajectories along (1, 1, 0), `per_sample` voxels per axis and sample: x starts a quarter into its voxel and y
    three quarters, so every step of more than half a voxel crosses a face in x or in y.  Trajectory b flies in the
    z layer 1 + 2 b, `lateral` voxels further along x.  A uniform cubic spline over equidistant control points is the
    line c_1 + v t."""
    v = per_sample * world.res / dt
    i = np.arange(N) - 1
    ctrl = np.zeros((B, N, 3))
    for b in range(B):
        start = world.origin + np.array([6.25 + lateral * b, 6.75, 1.5 + 2 * b]) * world.res
        ctrl[b, :, 0] = start[0] + i * (v * ts)
        ctrl[b, :, 1] = start[1] + i * (v * ts)
        ctrl[b, :, 2] = start[2]
    return ctrl


def mark_samples(world, ctrl, ts, times, marks):
    """occupy (bit 0) the voxel of sample k of trajectory b for every k in marks[b]"""
    for b, ks in enumerate(marks):
        for k in ks:
            ijk = voxel_of(world, positions(ctrl[b], ts, times[k:k + 1])[0]).astype(int)
            world.voxels[ijk[0], ijk[1], ijk[2]] |= 1


def _origin(res, on_lattice):
    return np.array([-40, -30, -3]) * res if on_lattice else np.array([-4.73, -3.61, -0.37]) * (res / 0.1)


@lru_cache(maxsize=None)
def first_hit_cases():
    out = []
    for idx, (ts, N, dt, T) in enumerate(FIRST_HIT_SHAPES):
        res = RESOLUTIONS[idx % 4]
        world = empty_world((96, 96, 32), res, _origin(res, idx % 2 == 1))
        singles = sorted({k for k in (0, 1, 62, 63, 64, 65, T - 2, T - 1) if 0 <= k < T})
        marks = [(k,) for k in singles] + [p for p in ((63, 64), (62, 65)) if p[1] < T]
        ctrl = diagonal_batch(world, ts, N, dt, len(marks))
        times = sample_times(duration(N, ts), dt)
        mark_samples(world, ctrl, ts, times, marks)
        out.append(GateCase(f"A:first hit ts={ts:.4g} N={N} dt={dt:.4g} T={T}", world, ts, N, dt, ctrl, T=T, marks=marks,
                            exp_flag=np.ones(len(marks), dtype=np.uint8), exp_first=np.array([m[0] for m in marks], dtype=np.int32)))
    ts, N, dt, T = FIRST_HIT_SHAPES[0]
    for name, fill, first in (("all free", 0, -1), ("all occupied", 1, 0)):
        world = empty_world((96, 96, 32), 0.1, _origin(0.1, False))
        world.voxels[:] = fill
        out.append(GateCase(f"A:{name}", world, ts, N, dt, diagonal_batch(world, ts, N, dt, 3), T=T, marks=[()] * 3,
                            exp_flag=np.full(3, fill, dtype=np.uint8), exp_first=np.full(3, first, dtype=np.int32)))
    return out


@lru_cache(maxsize=None)
def clock_cases():
    """trajectory 0: the voxel of sample T - 1 alone is occupied; trajectory 1 meets nothing"""
    out = []
    for kind, shapes in (("ends on tmax", CLOCK_EXACT), ("next step passes tmax by ulps", CLOCK_OVERSHOOT)):
        for idx, (ts, N, dt, T) in enumerate(shapes):
            res = RESOLUTIONS[(idx + 1) % 4]
            world = empty_world((96, 96, 8), res, _origin(res, idx % 2 == 0))
            ctrl = diagonal_batch(world, ts, N, dt, 2)
            marks = [(T - 1,), ()]
            mark_samples(world, ctrl, ts, sample_times(duration(N, ts), dt), marks)
            out.append(GateCase(f"B:{kind} N={N} dt={dt:.4g} T={T}", world, ts, N, dt, ctrl, T=T, marks=marks,
                                exp_flag=np.array([1, 0], dtype=np.uint8), exp_first=np.array([T - 1, -1], dtype=np.int32),
                                notes={"kind": kind}))
    return out


@lru_cache(maxsize=None)
def ratio_case():
    """not_check_ratio = 1/3: the static gate of the rebound loop samples t <= (1 - ncr) * duration, T_static samples.
    Trajectory 0 meets its only occupied voxel at sample T_static - 1, trajectory 1 at sample T_static."""
    ts, N, dt, T = FIRST_HIT_SHAPES[0]
    ncr = 1.0 / 3.0
    t_static = len(sample_times((1.0 - ncr) * duration(N, ts), dt))
    world = empty_world((96, 96, 8), 0.1, _origin(0.1, False))
    ctrl = diagonal_batch(world, ts, N, dt, 2)
    marks = [(t_static - 1,), (t_static,)]
    mark_samples(world, ctrl, ts, sample_times(duration(N, ts), dt), marks)
    return GateCase(f"R:not_check_ratio 1/3, last static sample {t_static - 1}", world, ts, N, dt, ctrl, T=T, marks=marks,
                    exp_flag=np.array([1, 0], dtype=np.uint8), ncr=ncr, notes={"T_static": t_static})


# ---- C: spline evaluation ---------------------------------------------------------------------------------------------
@dataclass
class EvalCase:
    name: str
    ts_ctrl: float
    N: int
    ctrl: np.ndarray        # [3, N, 3]
    times: np.ndarray
    n_knots: int            # times[:n_knots] are the knots j * ts_ctrl, the next 2 * n_knots their two neighbours


def eval_times(ts, N, dt=0.05):
    dur = duration(N, ts)
    knots = np.array([j * ts for j in range(N - 2)])        # written as that product
    edge = [-0.0, -dt, dur, np.nextafter(dur, np.inf), np.nextafter(dur, -np.inf), dur + 1.0]
    return np.concatenate([knots, np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf), edge]), len(knots)


@lru_cache(maxsize=None)
def eval_cases():
    out = []
    for ts in TS_CTRL:
        for N in EVAL_N:
            rng = np.random.default_rng(1000 * N + int(ts * 1000))
            times, nk = eval_times(ts, N)
            out.append(EvalCase(f"C:eval ts={ts:.4g} N={N}", ts, N, rng.normal(size=(3, N, 3)), times, nk))
    return out


def oracle_eval(case, deriv):
    return np.stack([positions(case.ctrl[b], case.ts_ctrl, case.times, deriv) for b in range(case.ctrl.shape[0])])


# ---- D: coordinates that are not finite, or far away ------------------------------------------------------------------
@lru_cache(maxsize=None)
def nonfinite_case():
    """trajectory 5 j + v carries NONFINITE[v] in control point (0, 3, N - 1)[j], on axis (j + v) % 3.  The map is free
    and the clean trajectories stay inside it, so by the contract of include/vigo.h (outside the box is occupied) the
    bad point and the two lines that end in it are occupied and nothing else is.  Trajectory b's one obstacle sits on
    the clean trajectory's sample inside the bad point's spans, smaller than the sample spacing: a bad x or y keeps the
    sample away from it (no hit through a NaN); a bad z does not matter to the dynamic gate."""
    ts, N, dt = 0.2, 12, 0.05
    world = empty_world((96, 96, 32), 0.1, _origin(0.1, False))
    B = 15
    clean = diagonal_batch(world, ts, N, dt, B, lateral=3)
    ctrl = clean.copy()
    times = sample_times(duration(N, ts), dt)
    obs, where = np.zeros((B, 9)), []
    pt, line = np.zeros((B, N), dtype=np.uint8), np.zeros((B, N), dtype=np.uint8)
    dyn = np.zeros(B, dtype=np.uint8)
    for j, (i, k) in enumerate(((0, 1), (3, 6), (N - 1, 34))):
        for v, bad in enumerate(NONFINITE):
            b, axis = 5 * j + v, (j + v) % 3
            ctrl[b, i, axis] = bad
            where.append((i, axis, k))
            pt[b, i] = 1
            line[b, i] = 1 if i > 0 else 0
            if i + 1 < N:
                line[b, i + 1] = 1
            p = positions(clean[b], ts, times[k:k + 1])[0]
            obs[b] = [p[0], p[1], p[2], 0, 0, 0, 0.06, 0.06, 0.5]
            dyn[b] = 1 if axis == 2 else 0
    return GateCase("D:one coordinate NaN, inf or 1e300", world, ts, N, dt, ctrl, T=len(times), obs_off=np.arange(B + 1, dtype=np.int32),
                    obs=obs, exp_flag=np.ones(B, dtype=np.uint8), exp_dyn=dyn, exp_pt=pt, exp_line=line,
                    notes={"where": where, "clean": clean})


# ---- E: the dynamic gate ----------------------------------------------------------------------------------------------
def _obs(x, y, z, sx, sy):
    return [x, y, z, 0.0, 0.0, 0.0, sx, sy, 0.5]


def gate_distance(p, o):
    """the gate's distance of sample p from obstacle o, as BT.h:358-361 rounds it"""
    dx, dy = np.float64(p[0]) - np.float64(o[0]), np.float64(p[1]) - np.float64(o[1])
    return np.sqrt((dx * dx + dy * dy) + 0.0)


def _csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    rows = [r for l in lists for r in l]
    return off, (np.array(rows, dtype=np.float64).reshape(-1, 9) if rows else np.zeros((0, 9)))


@lru_cache(maxsize=None)
def dynamic_cases():
    ts, N, dt, T = FIRST_HIT_SHAPES[0]
    res = 0.1
    world = empty_world((96, 96, 32), res, _origin(res, False))
    times = sample_times(duration(N, ts), dt)
    small = 0.06                                                       # radius 0.03 < half the sample spacing (0.039)
    far = _obs(world.origin[0] + 9.0, world.origin[1] + 0.5, 0.0, 0.3, 0.3)
    out = []
    # lists
    B = 8
    ctrl = diagonal_batch(world, ts, N, dt, B, lateral=3)
    pos = [positions(ctrl[b], ts, times) for b in range(B)]
    hit = lambda b: _obs(*pos[b][5 + b], small, small)
    lists = [[], [hit(1)], [far], [far, hit(3), far], [], [hit(5)], [far, far], []]
    off, obs = _csr(lists)
    common = dict(world=world, ts_ctrl=ts, N=N, dt=dt, ctrl=ctrl, T=T, exp_flag=np.zeros(B, dtype=np.uint8))
    out.append(GateCase("E:lists, empty at the first, a middle and the last trajectory", obs_off=off, obs=obs,
                        exp_dyn=np.array([0, 1, 0, 1, 0, 1, 0, 0], dtype=np.uint8), **common))
    shared = np.array([hit(1), far, hit(3), hit(5), hit(0), hit(7)])
    exp = np.array([1, 1, 0, 1, 0, 1, 0, 1], dtype=np.uint8)
    out.append(GateCase("E:shared list", obs_off=None, obs=shared, exp_dyn=exp, **common))
    out.append(GateCase("E:copies of the shared list", obs_off=(np.arange(B + 1) * len(shared)).astype(np.int32),
                        obs=np.tile(shared, (B, 1)), exp_dyn=exp, **common))
    out.append(GateCase("E:no obstacles", obs_off=None, obs=None, exp_dyn=np.zeros(B, dtype=np.uint8), **common))
    # the edges of the hit test, a trajectory each
    names = ["size = 2 dist: not a hit", "size = 2 nextafter(dist): a hit", "large x tiny: the minimum decides", "tiny x large: the minimum decides",
             "50 m above: z is ignored", "sample 0 alone", "sample 63 alone", "sample 64 = T - 1 alone", "40 obstacles, the last one hits",
             "negative sizes"]
    B = len(names)
    ctrl = diagonal_batch(world, ts, N, dt, B, lateral=3)
    pos = [positions(ctrl[b], ts, times) for b in range(B)]
    side = np.array([0.05, -0.05, 0.0]) / np.sqrt(2.0)                 # 0.05 m off the line: sample k is the nearest by far
    lists = []
    for b, k in ((0, 20), (1, 20)):
        c = pos[b][k] + side
        d = gate_distance(pos[b][k], c)
        s = 2 * d if b == 0 else 2 * np.nextafter(d, np.inf)
        lists.append([_obs(c[0], c[1], c[2], s, s)])
    c = pos[2][30] + side
    lists.append([_obs(c[0], c[1], c[2], 10.0, 0.02)])
    c = pos[3][30] + side
    lists.append([_obs(c[0], c[1], c[2], 0.02, 10.0)])
    lists.append([_obs(pos[4][30][0], pos[4][30][1], pos[4][30][2] + 50.0, small, small)])
    for b, k in ((5, 0), (6, 63), (7, T - 1)):
        lists.append([_obs(*pos[b][k], small, small)])
    lists.append([_obs(far[0], far[1] + 0.1 * j, 0.0, 0.05, 0.05) for j in range(39)] + [_obs(*pos[8][10], small, small)])
    lists.append([_obs(*pos[9][12], -1.0, -1.0), _obs(*pos[9][40], -10.0, 3.0), _obs(*pos[9][41], 3.0, -10.0)])
    off, obs = _csr(lists)
    out.append(GateCase("E:edges of the hit test", world, ts, N, dt, ctrl, T=T, obs_off=off, obs=obs, exp_flag=np.zeros(B, dtype=np.uint8),
                        exp_dyn=np.array([0, 1, 0, 0, 1, 1, 1, 1, 1, 0], dtype=np.uint8),
                        notes={"names": names, "single": {5: 0, 6: 63, 7: T - 1}, "boundary": (20, 20), "spacing": 0.55 * res * np.sqrt(2.0)}))
    return out


# ---- F: vigo_ctrl_occupancy -------------------------------------------------------------------------------------------
@dataclass
class OccCase:
    name: str
    world: World
    ctrl: np.ndarray                         # [B, N, 3]
    exp_pt: Optional[np.ndarray] = None
    exp_line: Optional[np.ndarray] = None
    notes: dict = field(default_factory=dict)

    @property
    def family(self):
        return "F"


def line_walk(world, q, p, steps_delta=0, first=1):
    """isInflatedOccupiedLine of the dense map contract (include/vigo.h) in numpy: the ends, then probes s = first ..
    steps - 1, steps = int(dist / res) + steps_delta.  Returns (flag, steps, [s of the occupied probes])."""
    q, p = np.asarray(q, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if numpy_lookup(world, q, 0) or numpy_lookup(world, p, 0):
        return 1, 0, []
    d = p - q
    dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    with np.errstate(invalid="ignore", divide="ignore"):
        inc = d / dist * world.res
        steps = int(dist / world.res) + steps_delta
    hits = [s for s in range(first, steps) if numpy_lookup(world, q + s * inc, 0)]
    return (1 if hits else 0), steps, hits


def centre(world, i, j, k):
    return world.origin + (np.array([i, j, k]) + 0.5) * world.res


@lru_cache(maxsize=None)
def occupancy_cases():
    out = []
    res = 0.1
    # 75 trajectories of 7 points: 525 points over three 256-thread blocks.  Even trajectories lie at x voxel 3, odd
    # ones at x voxel 9, the plane x = 6 is a wall: the last point of b and the first of b + 1 face each other across it
    world = empty_world((12, 18, 4), res, _origin(res, False))
    world.voxels[6, :, :] = 1
    B, N = 75, 7
    ctrl = np.zeros((B, N, 3))
    for b in range(B):
        for i in range(N):                                       # up along y, and back: b ends where b + 1 starts
            ctrl[b, i] = centre(world, 3 if b % 2 == 0 else 9, 2 + 2 * (i if b % 2 == 0 else N - 1 - i), 1)
    out.append(OccCase("F:a wall between one trajectory's last point and the next one's first", world, ctrl,
                       exp_pt=np.zeros((B, N), dtype=np.uint8), exp_line=np.zeros((B, N), dtype=np.uint8)))
    # single lines (N = 2), a row of y each
    def rows(specs, shape=(24, 40, 4), origin_on=False):
        w = empty_world(shape, res, _origin(res, origin_on))
        lines = list(specs(w))
        c = np.zeros((len(lines), 2, 3))
        for b, (q, p, occ) in enumerate(lines):
            c[b, 0], c[b, 1] = q, p
            for ijk in occ:
                w.voxels[ijk] = 1
        return w, c
    def probes(w):
        along = lambda j, d: (centre(w, 3, j, 1), centre(w, 3, j, 1) + np.array(d) * res)
        return [along(2, [0, 0, 0]) + ([],),                      # zero length
                along(4, [8.3, 0, 0]) + ([(4, 4, 1)],),           # the probe s = 1 of 7
                along(6, [8.3, 0, 0]) + ([(10, 6, 1)],),          # s = steps - 1 = 7
                along(8, [0, 5.3, 0]) + ([(3, 9, 1)],),           # s = 1 along y
                along(16, [0, 0, 2.3]) + ([(3, 16, 2)],),         # the only probe, along z
                along(20, [-5.0, 0, 0]) + ([],),                  # an end outside the map
                along(22, [8.3, 0, 0]) + ([],)]                   # free all the way
    w, c = rows(probes)
    out.append(OccCase("F:zero length, one occupied probe at s = 1 and at s = steps - 1, an end outside", w, c,
                       exp_pt=np.array([[0, 0]] * 5 + [[0, 1], [0, 0]], dtype=np.uint8),
                       exp_line=np.array([[0, 0]] + [[0, 1]] * 5 + [[0, 0]], dtype=np.uint8),
                       notes={"one_probe": {1: 1, 2: 7, 3: 1, 4: 1}}))
    # lines of length m * res and one ulp either side: the voxel of probe m - 1 alone is occupied, so the flag is 1
    # exactly when int(dist / res) reaches m
    for which, nudge in (("m res", 0), ("m res - 1 ulp", -1), ("m res + 1 ulp", 1)):
        ms = list(range(2, 16))
        def specs(w, nudge=nudge, ms=ms):
            for r, m in enumerate(ms):
                q = centre(w, 3, 2 + 2 * r, 1)
                p = q + [m * res, 0, 0]
                if nudge:
                    p[0] = np.nextafter(p[0], np.inf * nudge)
                yield q, p, [(3 + m - 1, 2 + 2 * r, 1)]
        w, c = rows(specs, origin_on=(nudge == 1))
        out.append(OccCase(f"F:step count next to an integer, length {which}", w, c, notes={"m": ms}))
    # N = 1: no line at all
    w = empty_world((8, 8, 4), res, _origin(res, False))
    w.voxels[2, 2, 1] = 1
    c = np.stack([centre(w, 1, 1, 1), centre(w, 2, 2, 1), centre(w, 9, 2, 1), centre(w, 3, 3, 1), centre(w, 2, 2, 2)])[:, None, :]
    out.append(OccCase("F:N = 1", w, c, exp_pt=np.array([[0], [1], [1], [0], [0]], dtype=np.uint8), exp_line=np.zeros((5, 1), dtype=np.uint8)))
    return out


# ---- G: point lookups -------------------------------------------------------------------------------------------------
@dataclass
class LookupCase:
    name: str
    world: World
    pts: np.ndarray          # [Q, 3]
    n_face: int              # pts[:n_face] = origin + ijk * res, the next 2 * n_face one ulp below / above them
    pair: int                # index into RESOLUTIONS
    notes: dict = field(default_factory=dict)


def parity_world(shape, res, origin):
    """bit 0: the checkerboard (i + j + k) & 1, which every single-axis off-by-one flips; bit 1: the checkerboard of
    2-voxel blocks, which an off-by-two (or a slip into the neighbouring word for the 32nd voxel) flips"""
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    vox = ((i + j + k) & 1) | ((((i >> 1) + (j >> 1) + (k >> 1)) & 1) << 1)
    return World(vox.astype(np.uint8), np.array(origin, dtype=np.float64), float(res))


def lookup_origin(pair):
    res = RESOLUTIONS[pair]
    return np.array([-10, -4, 0]) * res if pair % 2 == 1 else np.array([-1.2345, 0.4567, -0.0789])


@lru_cache(maxsize=None)
def lookup_cases(per_shape=400):
    out = []
    for pair, res in enumerate(RESOLUTIONS):
        origin = lookup_origin(pair)
        for shape in LOOKUP_SHAPES:
            rng = np.random.default_rng(7919 * pair + sum(shape))
            w = parity_world(shape, res, origin)
            ijk = rng.integers(0, np.array(shape) + 1, size=(per_shape, 3))
            face = origin + ijk * res
            corner = origin + np.array(shape) * res
            inside = origin + 0.5 * res
            special = [origin, corner, [-0.0, -0.0, -0.0], [inside[0], inside[1], -0.0], np.nextafter(corner, -np.inf)]
            for bad in NONFINITE:
                for a in range(3):
                    p = inside.copy()
                    p[a] = bad
                    special.append(p)
            pts = np.concatenate([face, np.nextafter(face, -np.inf), np.nextafter(face, np.inf), np.array(special)])
            out.append(LookupCase(f"G:res={res:.4g} origin {'on' if pair % 2 else 'off'} the lattice, {shape[0]}x{shape[1]}x{shape[2]}", w, pts,
                                  per_shape, pair, notes={"special": len(special)}))
    return out


# ---- H: vigo_inflate_grid ---------------------------------------------------------------------------------------------
def dilate_reference(occ, r):
    """box dilation of a boolean grid by r = (rx, ry, rz) voxels, axis by axis"""
    ref = occ.copy()
    for axis, rr in enumerate(r):
        acc = ref.copy()
        for d in range(1, min(rr, ref.shape[axis] - 1) + 1):
            sl_to = [slice(None)] * 3
            sl_from = [slice(None)] * 3
            sl_to[axis] = slice(d, None)
            sl_from[axis] = slice(None, -d)
            acc[tuple(sl_to)] |= ref[tuple(sl_from)]
            acc[tuple(sl_from)] |= ref[tuple(sl_to)]
        ref = acc
    return ref


@dataclass
class InflateCase:
    name: str
    vox: np.ndarray
    r: tuple


@lru_cache(maxsize=None)
def inflate_cases():
    out = []
    def add(name, shape, r, occupied=None, seed=0):
        rng = np.random.default_rng(seed + sum(shape))
        vox = ((rng.random(shape) < 0.3).astype(np.uint8) * 2 + (rng.random(shape) < 0.5).astype(np.uint8)).astype(np.uint8)
        if occupied is None:
            vox |= (rng.random(shape) < 0.03).astype(np.uint8) * 4
            vox[shape[0] // 2, shape[1] // 2, shape[2] // 2] |= 4
        else:
            for ijk in occupied:
                vox[ijk] |= 4
        out.append(InflateCase(f"H:{name} {shape[0]}x{shape[1]}x{shape[2]} r={r}", vox, r))
    for nz in (33, 64, 70):
        add("rz = 31, one voxel in the second word", (5, 4, nz), (0, 0, 31), occupied=[(2, 1, 32)])
        add("rz = 31, sparse", (5, 4, nz), (1, 1, 31))
    add("rz >= nz", (4, 4, 8), (0, 0, 20))
    add("rx >= nx", (3, 9, 10), (5, 0, 0))
    add("ry >= ny", (9, 3, 10), (0, 7, 1))
    add("nx = 1", (1, 6, 40), (2, 2, 2))
    shape = (6, 5, 70)
    for ijk in ((0, 0, 0), (5, 4, 69), (3, 2, 31), (3, 2, 32)):
        add(f"one voxel at {ijk}", shape, (1, 1, 3), occupied=[ijk])
    return out


INFLATE_REFUSED = ((4, 4, 40), (1, 1, 32))          # rz = 32: VIGO_ERR_UNSUPPORTED, bytes unchanged


def gate_cases():
    """every case the gates run on (families A, B, D, E)"""
    return first_hit_cases() + clock_cases() + [nonfinite_case()] + dynamic_cases()
