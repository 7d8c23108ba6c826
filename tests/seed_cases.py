"""Cases of the seed-path stage (vigo_seed_paths / vigo_seed_paths_host, csrc/vigo_seed_core.hpp), named and seeded, shared
by the CPU and the GPU tests: two workloads of 64 start/goal pairs (the open world of test_seed_chain_batch_equals_solo,
a pillar world), crafted single trajectories with explicit polynomials on one crafted world, waypoint cases the facade's
own steps can express, ctypes wrappers of the twin and of the facade's harness entries (host/src/cabi_host.cpp), and a
Python restatement of the rules that also records every distance it compares with a threshold — check_margins() asserts
none lies within 1e-9 relative of it, so that libm's power and the exact one cannot disagree on an integer output."""
import ctypes as C
import math
import os
from dataclasses import dataclass, field

import numpy as np

from trajectory_planner_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB = os.path.join(ROOT, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
OK, NO_SPACING, GOAL_OCCUPIED, TOO_SHORT, DEFERRED, BAD_INPUT = range(6)
ORIGIN = np.array([-3.0, -3.0, 0.0])
RES = 0.1
CPD = 0.25                       # bsplineTraj's control_point_distance
MAX_TRIES = 4                    # of the crafted cases (the workloads run the default, 16)
POINT_CAP = 160
SENTINEL_I, SENTINEL_D = -77, -7.5e77
OUT_KEYS = ("status", "tries", "dt", "final_time", "seed_n", "seed", "fit_n", "fit", "prev_seed", "prev_fit")


def capacity():
    n = C.c_int32(0)
    assert _lib.load().vigo_seed_capacity(C.byref(n)) == 0
    return int(n.value)


@dataclass
class World:
    vox: np.ndarray
    origin: np.ndarray = field(default_factory=lambda: ORIGIN.copy())
    res: float = RES


def open_world():
    return World(np.zeros((60, 60, 20), np.uint8))


def pillar_world(seed=5):
    """60 x 60 x 20 voxels of 0.1 m: inflated-occupied pillars (some unknown as well), as test_gpu_occmap_batch builds them"""
    rng = np.random.default_rng(seed)
    vox = np.zeros((60, 60, 20), np.uint8)
    for _ in range(25):
        c = rng.integers(3, 57, size=2)
        s = rng.integers(1, 4, size=2)
        vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], :] |= int(rng.choice([1, 3, 3]))
    return World(vox)


def craft_world():
    """120 x 60 x 20 voxels from (-3, -3, 0): open but for a wall across y in [-0.5, 0.5) at x in [-1.0, -0.8) and a block
    at x in [2.0, 2.4) on the same band (the occupied goal)"""
    vox = np.zeros((120, 60, 20), np.uint8)
    vox[20:22, 25:35, :] = 1
    vox[50:54, 25:35, :] = 1
    return World(vox)


def workload_pairs(which):
    """64 start/goal pairs: 'open' as test_seed_chain_batch_equals_solo draws them, 'pillar' across the pillar world"""
    rng = np.random.default_rng(8 if which == "open" else 9)
    return np.concatenate([rng.uniform([-2.5, -2.5, 0.8], [-1.0, 2.5, 1.4], size=(64, 1, 3)),
                           rng.uniform([1.0, -2.5, 0.8], [2.5, 2.5, 1.4], size=(64, 1, 3))], 1)


def workload_world(which):
    return open_world() if which == "open" else pillar_world()


# ---- one trajectory ----------------------------------------------------------------------------------------------------
@dataclass
class Traj:
    name: str
    knots: np.ndarray            # [K + 1]
    coeffs: np.ndarray           # [K, 3, deg + 1]
    duration: float
    dt0: float = 0.25
    cpd: float = CPD
    max_len: float = 1000.0
    prev_seed: float = 0.0
    prev_fit: float = 0.0
    expect: dict = field(default_factory=dict)     # what the case is crafted to give: status, tries, samples (of the last try)


def line(name, p0, v, knots, duration=None, jump=None, **kw):
    """p(t) = p0 + v t over the knots, degree 7; jump[i]: an offset added to segment i (a sample on an inner knot shows
    which segment it took)"""
    knots = np.asarray(knots, float)
    K = len(knots) - 1
    cf = np.zeros((K, 3, 8))
    for i in range(K):
        cf[i, :, 0] = np.asarray(p0, float) + np.asarray(v, float) * knots[i] + (0.0 if jump is None else np.asarray(jump[i], float))
        cf[i, :, 1] = v
    return Traj(name, knots, cf, float(knots[-1] if duration is None else duration), **kw)


def clock(dt, j):
    t = 0.0
    for _ in range(j):
        t = t + dt
    return t


def crafted():
    """name -> Traj, on craft_world().  Free lines run along y = 1, the ones meant to meet the wall / the block along y = 0."""
    cap = capacity()
    cs = []
    # sample counts 1 .. 5 at 1 m/s: seeds of 2, 3, 4, 5, 6 poses — fillPath's 2- and 3-pose branches, then none
    for n in range(1, 6):
        cs.append(line(f"samples_{n}", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 0.25 * (n - 1) + 0.1], expect=dict(status=OK, tries=1, samples=n)))
    # fillPath's branch for 4 or more poses: the head's rule 3 cuts the 6-pose seed to 3 points (prev 0, max_path_length 1),
    # the search's did not (prev 100)
    cs.append(line("fill_whole_seed", [-2.45, 1.02, 1.03], [6.6, 0, 0], [0, 1.1], cpd=2.0, max_len=1.0, prev_seed=100.0,
                   expect=dict(status=OK, tries=1, samples=5, seed_n=6, fit_n=6)))
    for n in (63, 64, 65, cap):          # either side of the lane stride; the capacity itself
        cs.append(line(f"samples_{n}", [-2.45, 1.02, 1.03], [0.00173 if n > 100 else 0.0173, 0, 0], [0, 0.25 * (n - 1)], expect=dict(status=OK, tries=1, samples=n)))
    cs.append(line("capacity_plus_1", [-2.45, 1.02, 1.03], [0.001, 0, 0], [0, 0.25 * cap], expect=dict(status=DEFERRED)))
    t10 = clock(0.1, 10)                 # dt divides the duration on the accumulated clock: the last sample has t == duration
    cs.append(line("dt_divides", [-2.45, 1.02, 1.03], [1.3, 0, 0], [0, t10], dt0=0.1, expect=dict(status=OK, tries=1, samples=11)))
    cs.append(line("dt_divides_not", [-2.45, 1.02, 1.03], [1.3, 0, 0], [0, math.nextafter(t10, 0.0)], dt0=0.1, expect=dict(status=OK, tries=1, samples=10)))
    cs.append(line("on_inner_knot", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 1.0, 2.0], jump=[[0, 0, 0], [0, 0.05, 0]], expect=dict(status=OK, tries=1, samples=9)))
    cs.append(line("before_first_knot", [0.02, 0.03, 0.04], [0.46, 0, 0], [0.5, 2.0], expect=dict(status=OK, tries=1, samples=9)))
    cs.append(line("one_try", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 1.6], expect=dict(status=OK, tries=1)))
    cs.append(line("two_tries", [-2.45, 1.02, 1.03], [1.6, 0, 0], [0, 1.6], expect=dict(status=OK, tries=2)))
    cs.append(line("max_tries", [-2.45, 1.02, 1.03], [2.6, 0, 0], [0, 1.6], expect=dict(status=OK, tries=MAX_TRIES)))
    cs.append(line("one_try_too_many", [-2.45, 1.02, 1.03], [3.2, 0, 0], [0, 1.6], expect=dict(status=NO_SPACING, tries=MAX_TRIES)))
    # 0.26 m a sample: the exit past 2.1 m comes at 2.34 m after a free stretch of 2.08 (10 points, 11 poses); the wall
    # resets the stretch, the exit waits for another 1.56 m behind it
    V = [1.04, 0, 0]
    cs.append(line("past_max_length", [-2.45, 1.02, 1.03], V, [0, 4.6], max_len=2.1, expect=dict(status=OK, tries=1, seed_n=11)))
    cs.append(line("past_max_length_wall", [-2.45, 0.02, 1.03], V, [0, 4.0], max_len=1.1, expect=dict(status=OK, tries=1)))
    cs.append(line("goal_occupied", [-0.45, 0.02, 1.03], V, [0, 2.6], expect=dict(status=GOAL_OCCUPIED, tries=1, fit_n=0)))
    cs.append(line("prev_above_max_seed", [-2.45, 1.02, 1.03], V, [0, 4.6], max_len=2.1, prev_seed=3.05, expect=dict(status=OK, tries=1)))
    cs.append(line("prev_above_max_fit", [-2.45, 1.02, 1.03], V, [0, 4.6], max_len=2.1, prev_fit=2.25, expect=dict(status=OK, tries=1)))
    cs.append(line("prev_above_max_both", [-2.45, 1.02, 1.03], V, [0, 4.6], max_len=1.1, prev_seed=3.05, prev_fit=2.15, expect=dict(status=OK, tries=1)))
    cs.append(line("negative_duration", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 1.0], duration=-1.0, expect=dict(status=TOO_SHORT, tries=1, samples=0)))
    cs.append(line("nan_knot", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, float("nan"), 2.0], duration=2.0, expect=dict(status=BAD_INPUT)))
    cs.append(line("inf_dt", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 1.0], dt0=float("inf"), expect=dict(status=BAD_INPUT)))
    cs.append(line("negative_dt", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 1.0], dt0=-0.25, expect=dict(status=BAD_INPUT)))
    cs.append(line("nan_duration", [-2.45, 1.02, 1.03], [1.0, 0, 0], [0, 1.0], duration=float("nan"), expect=dict(status=BAD_INPUT)))
    cs.append(line("stalled_clock", [-2.45, 1.02, 1.03], [1e-20, 0, 0], [0, 1e18], dt0=1.0, expect=dict(status=BAD_INPUT)))
    return {c.name: c for c in cs}


def pack(trajs):
    """Traj list -> the arrays of one call (vigo_traj_point_check's layout)"""
    T = len(trajs)
    seg_off = np.zeros(T + 1, np.int32)
    for t, c in enumerate(trajs):
        seg_off[t + 1] = seg_off[t] + len(c.knots) - 1
    S = int(seg_off[-1])
    coeffs = np.zeros((S, 3, 8))
    knots = np.zeros(S + T)
    for t, c in enumerate(trajs):
        coeffs[seg_off[t]:seg_off[t + 1]] = c.coeffs
        knots[seg_off[t] + t:seg_off[t + 1] + t + 1] = c.knots
    per = {k: np.array([getattr(c, k) for c in trajs], float) for k in ("duration", "dt0", "cpd", "max_len", "prev_seed", "prev_fit")}
    return dict(T=T, S=S, seg_off=seg_off, coeffs=coeffs, knots=knots, **per)


def blank_outputs(T, point_cap=POINT_CAP):
    o = {k: np.full(T, SENTINEL_I, np.int32) for k in ("status", "tries", "seed_n", "fit_n")}
    o.update({k: np.full(T, SENTINEL_D) for k in ("dt", "final_time", "prev_seed", "prev_fit")})
    o["seed"] = np.full((T, point_cap, 3), SENTINEL_D)
    o["fit"] = np.full((T, point_cap, 3), SENTINEL_D)
    return o


def twin(world, a, pow_mode, max_tries=MAX_TRIES, point_cap=POINT_CAP, cap=0):
    """vigo_seed_paths_host on the arrays of pack() -> (rc, outputs pre-filled with sentinels)"""
    lib = _lib.load()
    o = blank_outputs(a["T"], max(point_cap, 1))
    vox = np.ascontiguousarray(world.vox)
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = lib.vigo_seed_paths_host(*vox.shape, (C.c_double * 3)(*world.origin), float(world.res), P(vox), pow_mode, cap, a["T"], a["S"], 7,
                                  P(a["seg_off"]), P(a["coeffs"]), P(a["knots"]), P(a["duration"]), P(a["dt0"]), P(a["cpd"]), P(a["max_len"]),
                                  P(a["prev_seed"]), P(a["prev_fit"]), max_tries, point_cap, *[P(o[k]) for k in OUT_KEYS])
    return rc, o


# ---- the rules in Python -----------------------------------------------------------------------------------------------
def norm(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def occupied(world, p):
    f = [math.floor((p[a] - world.origin[a]) / world.res) for a in range(3)]
    if any(not (0 <= f[a] < world.vox.shape[a]) for a in range(3)):
        return True
    return bool(world.vox[int(f[0]), int(f[1]), int(f[2])] & 1)


def line_occupied(world, q, p):
    if occupied(world, q) or occupied(world, p):
        return True
    d = [p[a] - q[a] for a in range(3)]
    dist = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    if dist == 0.0:
        return False
    inc = [d[a] / dist * world.res for a in range(3)]
    for s in range(1, int(dist / world.res)):
        if occupied(world, [q[a] + s * inc[a] for a in range(3)]):
            return True
    return False


def sample(c, t, power):
    t = min(t, c.duration)
    for i in range(len(c.knots) - 1):
        if c.knots[i] <= t <= c.knots[i + 1]:
            lt = t - c.knots[i]
            p = [0.0, 0.0, 0.0]
            for d in range(c.coeffs.shape[2]):
                pw = power(lt, d)
                for a in range(3):
                    p[a] = p[a] + float(c.coeffs[i, a, d]) * pw
            return p
    return [0.0, 0.0, 0.0]


def adjust(world, pts, prev, max_len, log):
    """rule 3 -> (length of the adjusted prefix, prev afterwards)"""
    if not pts:
        return 0, prev
    limit = max(prev, max_len)
    total, min_length, exceed = 0.0, 0.0, False
    for i in range(len(pts) - 1):
        total = norm(pts[i + 1], pts[0])
        log.append((total, limit))
        if total >= limit:
            exceed = True
        occ = line_occupied(world, pts[i], pts[i + 1])
        if exceed and not occ:
            log.append((min_length, 1.5))
            if min_length >= 1.5:
                return i + 2, total
        min_length = 0.0 if occ else min_length + norm(pts[i + 1], pts[i])
    return len(pts), total


def restate(world, c, max_tries=MAX_TRIES, point_cap=POINT_CAP, cap=None, power=math.pow, log=None):
    """The stage for one Traj -> dict like one row of the twin's outputs (absent keys: not written), 'samples' added"""
    log = [] if log is None else log
    cap = capacity() if cap is None else cap
    reset = dict(tries=0, dt=c.dt0, final_time=0.0, seed_n=0, fit_n=0, prev_seed=c.prev_seed, prev_fit=c.prev_fit, seed=[], fit=[])
    if not all(map(math.isfinite, [c.duration, c.dt0, *c.knots])) or not c.dt0 > 0:
        return dict(status=BAD_INPUT, **reset)
    dt, prev, tries, found = c.dt0, c.prev_seed, 0, False
    while tries < max_tries:
        if c.duration > 0 and dt <= math.ldexp(1.0, math.frexp(c.duration)[1] - 1 - 53):
            return dict(status=BAD_INPUT, **reset)
        if c.duration / dt > cap + 8:
            return dict(status=DEFERRED)
        pts, t = [], 0.0
        while t <= c.duration:
            pts.append(sample(c, t, power))
            t = t + dt
            if len(pts) > cap:
                return dict(status=DEFERRED)
        tries += 1
        n, prev = adjust(world, pts, prev, c.max_len, log)
        steps = [norm(pts[i], pts[i + 1]) for i in range(n - 1)]
        log += [(s, 1.5 * c.cpd) for s in steps]
        if not any(s > c.cpd * 1.5 for s in steps):
            found = True
            break
        dt = dt * 0.8
    r = dict(tries=tries, dt=dt, final_time=0.0, seed_n=0, fit_n=0, prev_seed=prev, prev_fit=c.prev_fit, seed=[], fit=[], samples=len(pts))
    if not found:
        return dict(status=NO_SPACING, **r)
    if n == 0:
        return dict(status=TOO_SHORT, **r)
    kept = [pts[0]]
    for p in pts[1:n]:
        d = norm(p, kept[-1])
        log.append((d, 0.8 * c.cpd))
        if d >= c.cpd * 0.8:
            kept.append(p)
    seed = kept + [kept[-1]]
    if len(seed) > point_cap:
        return dict(status=DEFERRED)
    r.update(final_time=float(n - 1) * dt, seed=seed, seed_n=len(seed))
    if occupied(world, seed[-1]):
        return dict(status=GOAL_OCCUPIED, **r)
    m, r["prev_fit"] = adjust(world, seed, c.prev_fit, c.max_len, log)
    fit = seed[:m]
    if m < 4:
        if len(seed) == 2:
            ps, pf = seed
            fit = [ps, [(pf[a] - ps[a]) / 3.0 + ps[a] for a in range(3)], [2.0 * (pf[a] - ps[a]) / 3.0 + ps[a] for a in range(3)], pf]
        elif len(seed) == 3:
            ps, pm, pf = seed
            fit = [ps, [(ps[a] + pm[a]) / 2.0 for a in range(3)], pm, [(pm[a] + pf[a]) / 2.0 for a in range(3)], pf]
        else:
            fit = seed
    if len(fit) > point_cap:
        return dict(status=DEFERRED)
    r.update(fit=fit, fit_n=len(fit))
    return dict(status=OK, **r)


def pow_bound(c, t):
    """16 * 2^-52 * sum_d |c_d| t^d per coordinate for the sample at clock value t: one ulp per power and eight roundings of
    the sum, doubled — how far the sample moves between libm's power and the correctly rounded one"""
    t = min(t, c.duration)
    for i in range(len(c.knots) - 1):
        if c.knots[i] <= t <= c.knots[i + 1]:
            lt = t - c.knots[i]
            return 16 * 2.0 ** -52 * (np.abs(c.coeffs[i]) * lt ** np.arange(c.coeffs.shape[2])).sum(1)
    return np.zeros(3)


def point_bounds(c, dt, pts):
    """pts [n, 3]: poses of a seed made with libm's power from Traj c on the clock of dt.  Each is one of the samples
    p(t_j), bit for bit; returns [n, 3], pose k's own bound pow_bound(c, t_j) at the t_j of the sample it is."""
    ts, t = [], 0.0
    while t <= c.duration:
        ts.append(t)
        t = t + dt
    S = np.array([sample(c, t, math.pow) for t in ts]).reshape(len(ts), 3)
    out = np.zeros((len(pts), 3))
    for k, p in enumerate(pts):
        d = np.abs(S - p).max(1)
        j = int(d.argmin())
        assert d[j] == 0.0, (c.name, k, d[j])                # the pose IS a sample of this clock
        out[k] = pow_bound(c, ts[j])
    return out


def fit_bounds(seed_b, fit_n):
    """the bounds of the curve-fit points from the seed poses' [seed_n, 3]: a prefix of the seed (or the seed whole), or
    fillPath's points, linear in their two parents — the 2-pose branch's thirds, the 3-pose branch's means"""
    n = len(seed_b)
    if fit_n == 4 and n == 2:
        return np.array([seed_b[0], (2 * seed_b[0] + seed_b[1]) / 3, (seed_b[0] + 2 * seed_b[1]) / 3, seed_b[1]])
    if fit_n == 5 and n == 3:
        return np.array([seed_b[0], (seed_b[0] + seed_b[1]) / 2, seed_b[1], (seed_b[1] + seed_b[2]) / 2, seed_b[2]])
    assert fit_n <= n
    return seed_b[:fit_n]


def check_margins(log):
    """no compared distance within 1e-9 relative of its threshold"""
    for v, thr in log:
        assert abs(v - thr) > 1e-9 * max(abs(thr), abs(v)), (v, thr)


def assert_row(o, t, want, what=""):
    """row t of the twin's / the kernel's outputs against restate()'s dict, bit for bit; keys a status does not write keep
    their sentinels"""
    assert o["status"][t] == want["status"], (what, o["status"][t], want["status"])
    if want["status"] == DEFERRED:
        for k in OUT_KEYS[1:]:
            assert np.all(o[k][t] == (SENTINEL_I if o[k].dtype == np.int32 else SENTINEL_D)), (what, k)
        return
    for k in ("tries", "seed_n", "fit_n"):
        assert o[k][t] == want[k], (what, k, o[k][t], want[k])
    for k in ("dt", "final_time", "prev_seed", "prev_fit"):
        assert np.float64(o[k][t]).view(np.uint64) == np.float64(want[k]).view(np.uint64), (what, k, o[k][t], want[k])
    for k, n in (("seed", want["seed_n"]), ("fit", want["fit_n"])):
        got = o[k][t, :n]
        assert np.array_equal(got.view(np.uint64), np.array(want[k], float).reshape(n, 3).view(np.uint64)), (what, k)
        assert np.all(o[k][t, n:] == SENTINEL_D), (what, k, "rows past the count were written")


def assert_same_outputs(a, b, what=""):
    """two output dicts bit for bit, every array whole (sentinels included)"""
    for k in OUT_KEYS:
        x, y = a[k], b[k]
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), (what, k, np.argwhere(x != y)[:5])


# ---- the facade's own steps (libtrajectory_planner_vigo.so, no GPU) ---------------------------------------------------
POLY_CFG = None


def poly_cfg():
    from test_occmap_planner import cfg_vec
    return np.ascontiguousarray(cfg_vec(desired_velocity=1.0, desired_acceleration=1.0), dtype=np.float64)


BSP_CFG = np.array([0.5, 0.0, 2.0, 2.0, 2.0, 2.0])


def facade_steps(world, paths, max_len=1000.0, dt0=None, prev_seed=None, prev_fit=None, max_tries=16, point_cap=POINT_CAP):
    """vigo_host_seed_steps for waypoint paths (list of [W, 3]) -> (Traj list holding the polynomials the steps sampled,
    outputs dict in the twin's keys plus 'found' / 'fit_ok' / 'fit_wrote')"""
    L = C.CDLL(HOST_LIB)
    Pn, seg_cap = len(paths), 8
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
    wp = np.ascontiguousarray(np.concatenate(paths), dtype=np.float64)
    z = lambda x: np.zeros(Pn) if x is None else np.ascontiguousarray(x, dtype=np.float64)
    dt0, prev_seed, prev_fit = z(dt0), z(prev_seed), z(prev_fit)
    K = np.zeros(Pn, np.int32)
    knots, coeffs, dur, dt0_out = np.zeros((Pn, seg_cap + 1)), np.zeros((Pn, seg_cap, 3, 8)), np.zeros(Pn), np.zeros(Pn)
    flags, vals = np.zeros((Pn, 4), np.int32), np.zeros((Pn, 5))
    o = blank_outputs(Pn, point_cap)
    vox = np.ascontiguousarray(world.vox)
    D = lambda a: a.ctypes.data_as(_dp)
    I = lambda a: a.ctypes.data_as(_ip)
    L.vigo_host_seed_steps.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _ip, _dp, _dp, _dp, C.c_double, _dp, _dp,
                                       _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_int, _ip, _dp, _ip, _dp, _ip, _dp]
    rc = L.vigo_host_seed_steps(*vox.shape, D(np.ascontiguousarray(world.origin)), float(world.res), vox.ctypes.data_as(C.c_void_p), Pn, I(off),
                                D(wp), D(poly_cfg()), D(BSP_CFG), float(max_len), D(dt0), D(prev_seed), D(prev_fit), max_tries, seg_cap, I(K),
                                D(knots), D(coeffs), D(dur), D(dt0_out), point_cap, I(flags), D(vals), I(o["seed_n"]), D(o["seed"]),
                                I(o["fit_n"]), D(o["fit"]))
    assert rc == 0, rc
    trajs = [Traj(f"path_{i}", knots[i, :K[i] + 1].copy(), coeffs[i, :K[i]].copy(), float(dur[i]), dt0=float(dt0_out[i]), cpd=float(vals[i, 4]),
                  max_len=float(max_len), prev_seed=float(prev_seed[i]), prev_fit=float(prev_fit[i])) for i in range(Pn)]
    o.update(tries=flags[:, 1].copy(), dt=vals[:, 0].copy(), final_time=vals[:, 1].copy(), prev_seed=vals[:, 2].copy(), prev_fit=vals[:, 3].copy(),
             found=flags[:, 0].copy(), fit_ok=flags[:, 2].copy(), fit_wrote=flags[:, 3].copy())
    return trajs, o


def waypoint_cases():
    """(name, waypoints, max_path_length, prev_seed, prev_fit) on craft_world(): what the facade's planners can express of
    the crafted list — paths of a few samples for the fillPath branches, the early exit past max_path_length with and
    without the wall, an occupied goal, previous lengths above max_path_length in either phase and both"""
    W = lambda *p: np.array(p, float)
    cs = [(f"short_{int(100 * d)}", W([-2.45, 1.02, 1.03], [-2.45 + d, 1.02, 1.03]), 1000.0, 0.0, 0.0) for d in (0.07, 0.21, 0.33, 0.58, 0.87, 1.13)]
    cs += [("past_max_length", W([-2.45, 1.02, 1.03], [2.15, 1.22, 1.03]), 2.1, 0.0, 0.0),
           ("past_max_length_wall", W([-2.45, 0.02, 1.03], [1.85, 0.12, 1.03]), 1.1, 0.0, 0.0),
           ("goal_occupied", W([-0.45, 0.02, 1.03], [2.15, 0.04, 1.03]), 1000.0, 0.0, 0.0),
           ("prev_above_max_seed", W([-2.45, 1.02, 1.03], [2.15, 1.22, 1.03]), 2.1, 3.05, 0.0),
           ("prev_above_max_fit", W([-2.45, 1.02, 1.03], [2.15, 1.22, 1.03]), 2.1, 0.0, 2.25),
           ("prev_above_max_both", W([-2.45, 1.02, 1.03], [2.15, 1.22, 1.03]), 1.1, 3.05, 2.15),
           ("three_waypoints", W([-2.45, 1.02, 1.03], [0.15, 1.62, 1.23], [2.15, 1.22, 1.03]), 1000.0, 0.0, 0.0)]
    return cs
