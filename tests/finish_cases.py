"""Shared by tests/test_finish_core.py (CPU: vigo_traj_finish_host against the restatement, and the restatement against
the compiled reference where it is built), tests/test_gpu_finish.py (the kernel against both) and tools/time_finish.py:
the named, seeded cases of the plan's last stage (csrc/vigo_finish_core.hpp) and a literal restatement of its rule in
Python.  numpy and the CPU oracle only; no GPU, no torch.

  count      n = 7, 8 (the derivative splines have 6 / 5 and 7 / 6 points), 64 and 65 inside Ns = 65, a mixed row set
  clock      durations that sit on the clock: every t_k exact and t_8 == duration; ten additions of 0.1 below 1.0
  stride_dt  sample counts 1, 63, 64, 65, 128, 129: either side of the 64-lane stride of the output loop
  stride_ts  the same counts of the strict ts clock: either side of the stride of the maxima's loop
  degenerate no motion, a straight evenly spaced line, one NaN coordinate, a row of NaN
  limit      the velocity limit binds, the acceleration limit binds, both factors are the same bits
  status     CAPACITY (S_cap = n_samp - 1) and INVALID_N (counts 6, Ns + 1, 0) next to valid neighbours
  batch      B = 1, 3, 65

A case's rows are padded with NaN beyond their counts: code that reads past a row's points does not get the expected
bits.  expected(case) is the restatement; it asserts what the case's name promises before anything uses the case."""
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import oracle_lib as ol

OK, CAPACITY, INVALID_N = 0, 1, 2
SENTINEL = -7.25e33        # what the sample rows hold before a call; no case produces it
STRIDE_COUNTS = (1, 63, 64, 65, 128, 129)


@dataclass
class FinishCase:
    name: str
    ts_ctrl: float
    ts: float
    dt: float
    ctrl: np.ndarray                        # [B, Ns, 3], NaN beyond a row's count
    limits: np.ndarray                      # [B, 2] max_vel, max_acc
    n_pts: Optional[np.ndarray] = None      # int32 [B]; None: every row has Ns
    S_cap: int = 0                          # 0: the largest sample count of the case + 2
    promise: dict = field(default_factory=dict)   # trajectory -> {field: value} the name stands for

    @property
    def family(self):
        return self.name.split(":")[0]

    @property
    def B(self):
        return self.ctrl.shape[0]

    @property
    def Ns(self):
        return self.ctrl.shape[1]

    def count(self, b):
        return self.Ns if self.n_pts is None else int(self.n_pts[b])

    def row(self, b):
        return np.ascontiguousarray(self.ctrl[b, :self.count(b)])


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def oracle_eval(c, ts_ctrl, deriv, t):
    out = np.zeros(3)
    ol.oracle().vgo_traj_eval(c.shape[0], ol._d(c), float(ts_ctrl), int(deriv), float(t), ol._d(out))
    return out


def norm3(v):
    v0, v1, v2 = float(v[0]), float(v[1]), float(v[2])
    s = (v0 * v0 + v1 * v1) + v2 * v2
    return math.sqrt(s)


def restate_one(c, ts_ctrl, ts, dt, max_vel, max_acc, ev=oracle_eval):
    """One trajectory by the serial loops of BT.cpp:1116-1137 and :1502-1518: dict of factor, factorVel, factorAcc, maxV,
    maxA, K (samples of the strict ts loop), pos [n_samp, 3], vel [n_samp, 3], vnorms."""
    n = c.shape[0]
    duration = (n - 3) * ts_ctrl
    maxV = maxA = 0.0
    vnorms = []
    t = 0.0
    while t < duration:
        nv = norm3(ev(c, ts_ctrl, 1, t))
        if nv > maxV:
            maxV = nv
        na = norm3(ev(c, ts_ctrl, 2, t))
        if na > maxA:
            maxA = na
        vnorms.append(nv)
        t += ts
    with np.errstate(divide="ignore", invalid="ignore"):
        factorVel = float(np.float64(max_vel) / np.float64(maxV))
        factorAcc = float(np.sqrt(np.float64(max_acc) / np.float64(maxA)))
    factor = factorAcc if factorAcc < factorVel else factorVel
    pos, vel = [], []
    t, i = 0.0, 0
    while t <= duration:
        pos.append(ev(c, ts_ctrl, 0, t))
        vel.append(ev(c, ts_ctrl, 1, float(i) * dt))
        i += 1
        t += dt
    # (a NaN sample is stored as the one quiet NaN: its sign and payload are the implementation's, not the rule's)
    one_nan = lambda a: np.where(np.isnan(a), np.float64(np.nan), a)
    return {"factor": factor, "factorVel": factorVel, "factorAcc": factorAcc, "maxV": maxV, "maxA": maxA, "K": len(vnorms),
            "pos": one_nan(np.array(pos).reshape(-1, 3)), "vel": one_nan(np.array(vel).reshape(-1, 3)), "vnorms": np.array(vnorms)}


_expected = {}


def expected(case, ev=oracle_eval):
    """The outputs of vigo_traj_finish for the case, sample rows pre-filled with SENTINEL: dict of factor [B], max [B,2],
    n [B], pos / vel [B,S_cap,3], status [B], S_cap, one (the per-trajectory restatements, None for INVALID_N)."""
    key = (case.name, ev is oracle_eval)
    if key in _expected:
        return _expected[key]
    B = case.B
    one = []
    for b in range(B):
        n = case.count(b)
        one.append(restate_one(case.row(b), case.ts_ctrl, case.ts, case.dt, case.limits[b, 0], case.limits[b, 1], ev)
                   if 7 <= n <= case.Ns else None)
    S_cap = case.S_cap or max(len(o["pos"]) for o in one if o is not None) + 2
    e = {"factor": np.full(B, np.nan), "max": np.full((B, 2), np.nan), "n": np.zeros(B, dtype=np.int32),
         "pos": np.full((B, S_cap, 3), SENTINEL), "vel": np.full((B, S_cap, 3), SENTINEL), "status": np.full(B, INVALID_N, dtype=np.int32),
         "S_cap": S_cap, "one": one}
    for b, o in enumerate(one):
        if o is None:
            continue
        m = len(o["pos"])
        e["factor"][b], e["max"][b], e["n"][b] = o["factor"], (o["maxV"], o["maxA"]), m
        e["status"][b] = CAPACITY if m > S_cap else OK
        e["pos"][b, :min(m, S_cap)] = o["pos"][:S_cap]
        e["vel"][b, :min(m, S_cap)] = o["vel"][:S_cap]
    check_promises(case, e)
    _expected[key] = e
    return e


def check_promises(case, e):
    """what the case's name says, asserted on the restatement"""
    for b, want in case.promise.items():
        o = e["one"][b]
        for k, v in want.items():
            if k == "status":
                got = int(e["status"][b])
            elif k == "n_samp":
                got = int(e["n"][b])
            elif k == "equal_velocities":
                got = len(set(o["vnorms"].view(np.uint64).tolist())) == 1 and o["K"] > 1
            elif k == "factor_is":
                got, v = bits(o["factor"]), bits(o[v])
            elif k == "factors_equal":
                got = bits(o["factorVel"]) == bits(o["factorAcc"])
            elif k == "binds":
                got = "vel" if o["factorVel"] < o["factorAcc"] else ("acc" if o["factorAcc"] < o["factorVel"] else "both")
            elif k == "finite_maxima":
                got = math.isfinite(o["maxV"]) and math.isfinite(o["maxA"]) and o["maxV"] > 0.0 and o["maxA"] > 0.0
            elif k == "nan_samples":
                got = bool(np.isnan(o["vnorms"]).any()) and not bool(np.isnan(o["vnorms"]).all())
            else:
                got = o[k]
            assert got == v, f"{case.name}, trajectory {b}: {k} is {got!r}, the case needs {v!r}"


def bits(x):
    return int(np.float64(x).view(np.uint64))


# ---- builders --------------------------------------------------------------------------------------------------------
def random_rows(rng, counts, Ns):
    """[B, Ns, 3]: a random walk of control points per row, NaN beyond the row's count"""
    ctrl = np.full((len(counts), Ns, 3), np.nan)
    for b, n in enumerate(counts):
        if 0 < n <= Ns:
            steps = rng.uniform(-0.3, 0.3, (n, 3)) + np.array([0.25, 0.05, 0.0])
            ctrl[b, :n] = rng.uniform(-2.0, 2.0, 3) + np.cumsum(steps, axis=0)
    return ctrl


def random_limits(rng, B):
    return np.stack([rng.uniform(0.5, 3.0, B), rng.uniform(0.5, 4.0, B)], axis=1)


def plain_count(step, duration, strict):
    k, t = 0, 0.0
    while (t < duration) if strict else (t <= duration):
        k += 1
        t += step
    return k


def make(name, rng, counts, Ns, ts_ctrl=0.2, ts=0.1, dt=0.1, mixed=None, **kw):
    mixed = (len(set(counts)) > 1 or counts[0] != Ns) if mixed is None else mixed
    return FinishCase(name, ts_ctrl, ts, dt, random_rows(rng, counts, Ns), random_limits(rng, len(counts)),
                      np.array(counts, dtype=np.int32) if mixed else None, **kw)


MIXED_COUNTS = (7, 32, 9, 64, 31, 8)
_cases = []


def cases():
    if _cases:
        return _cases
    rng = np.random.default_rng(20261020)
    out = []
    # count
    out.append(make("count:n7", rng, [7, 7], 7, promise={0: {"K": plain_count(0.1, 4 * 0.2, True)}}))
    out.append(make("count:n8", rng, [8, 8, 8], 8))
    out.append(make("count:n64_n65_in_65", rng, [64, 65, 65, 64], 65))
    out.append(make("count:mixed_in_64", rng, list(MIXED_COUNTS), 64))
    # clock
    out.append(make("clock:exact_t8_is_duration", rng, [7, 7], 7, ts_ctrl=0.25, ts=0.125, dt=0.125, promise={0: {"K": 8, "n_samp": 9}}))
    t10 = 0.0
    for _ in range(10):
        t10 += 0.1
    assert t10 == 0.9999999999999999 and t10 < (8 - 3) * 0.2 == 1.0
    out.append(make("clock:ten_tenths_below_one", rng, [8, 8], 8, ts_ctrl=0.2, ts=0.1, dt=0.1, promise={0: {"K": 11, "n_samp": 11}}))
    # either side of the 64-lane stride, on each clock (n = 19 at ts_ctrl 0.2: duration 3.2)
    dur = (19 - 3) * 0.2
    for m in STRIDE_COUNTS:
        dt = 2.0 * dur if m == 1 else dur / (m - 0.5)
        assert plain_count(dt, dur, False) == m
        out.append(make(f"stride_dt:{m}", rng, [19, 19], 19, dt=dt, promise={0: {"n_samp": m}, 1: {"n_samp": m}}))
    for m in STRIDE_COUNTS:
        ts = 2.0 * dur if m == 1 else dur / (m - 0.5)
        assert plain_count(ts, dur, True) == m
        out.append(make(f"stride_ts:{m}", rng, [19, 19], 19, ts=ts, dt=0.4, promise={0: {"K": m}, 1: {"K": m}}))
    # degenerate motion, ts_ctrl = 0.25
    lim = np.array([[1.5, 2.0]])
    inf = float("inf")
    still = np.tile(np.array([0.3, -1.1, 0.9]), (1, 9, 1))
    out.append(FinishCase("degenerate:still", 0.25, 0.1, 0.1, still, lim.copy(), promise={0: {"maxV": 0.0, "maxA": 0.0, "factor": inf}}))
    line = np.array([0.5, 0.0, 0.0])[None, None, :] * np.arange(10)[None, :, None] + np.array([1.0, 2.0, 0.5])
    out.append(FinishCase("degenerate:line", 0.25, 0.125, 0.1, line, lim.copy(),
                          promise={0: {"equal_velocities": True, "maxA": 0.0, "factorAcc": inf, "factor_is": "factorVel"}}))
    nan_mid = random_rows(rng, [12], 12)
    nan_mid[0, 6, 1] = np.nan
    out.append(FinishCase("degenerate:nan_mid", 0.25, 0.1, 0.1, nan_mid, lim.copy(), promise={0: {"nan_samples": True, "finite_maxima": True}}))
    out.append(FinishCase("degenerate:nan_row", 0.25, 0.1, 0.1, np.full((1, 9, 3), np.nan), lim.copy(),
                          promise={0: {"maxV": 0.0, "maxA": 0.0, "factor": inf}}))
    # which limit binds: the limits from the trajectory's own maxima
    base = random_rows(rng, [14], 14)
    o = restate_one(np.ascontiguousarray(base[0]), 0.2, 0.1, 0.1, 1.0, 1.0)
    for tag, mv, ma in (("vel", o["maxV"] * 0.5, o["maxA"] * 4.0), ("acc", o["maxV"] * 2.0, o["maxA"] * 0.25), ("both", o["maxV"] * 2.0, o["maxA"] * 4.0)):
        out.append(FinishCase(f"limit:{tag}", 0.2, 0.1, 0.1, base.copy(), np.array([[mv, ma]]),
                              promise={0: {"binds": tag, **({"factors_equal": True, "factor": 2.0} if tag == "both" else {})}}))
    # statuses
    cap = make("status:capacity", rng, [8, 20, 9], 20)
    cap.S_cap = plain_count(0.1, (20 - 3) * 0.2, False) - 1
    cap.promise = {0: {"status": OK}, 1: {"status": CAPACITY, "n_samp": cap.S_cap + 1}, 2: {"status": OK}}
    out.append(cap)
    out.append(make("status:invalid_n", rng, [9, 6, 12, 13, 10, 0, 7], 12, mixed=True,
                    promise={0: {"status": OK}, 1: {"status": INVALID_N}, 2: {"status": OK}, 3: {"status": INVALID_N}, 4: {"status": OK},
                             5: {"status": INVALID_N}, 6: {"status": OK}}))
    # batch sizes
    out.append(make("batch:1", rng, [11], 11))
    out.append(make("batch:3", rng, [9, 16, 12], 16))
    out.append(make("batch:65", rng, [int(v) for v in rng.integers(7, 25, 65)], 24, mixed=True))
    out.append(make("batch:65_uniform", rng, [10] * 65, 10))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    _cases.extend(out)
    return _cases


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ---- the facade's stage (host/src/cabi_host.cpp) -----------------------------------------------------------------------
def plan_batch_finish(world, path_off, xyz, no_device=-1, small_step=-1, step=0.0, with_paths=True, yaw=True, reps=1, pose_cap=160, cfg=None):
    """makePlanBatch (with_paths: the overload that returns trajectories) with setDeviceEpilogue off (slot 0) and on (slot
    1), `reps` rounds over off, then on -> dict of per-slot arrays; totals[slot] = (planners the device call decided,
    planners on the host route, device groups).  Planner no_device sits on a device ordinal that does not exist, planner
    small_step gets bspline_traj/timestep = step, a group of its own (< 0: none).  Needs a GPU."""
    import plan_batch as pb
    n = len(path_off) - 1
    device, timestep = np.full(n, -1), np.full(n, np.nan)
    device[[no_device] if no_device >= 0 else []] = 63
    timestep[[small_step] if small_step >= 0 else []] = step
    r = pb.plan_batch(world, path_off, xyz, [(0, 16384, pb.BY_CALL), (pb.EPILOGUE, 16384, pb.BY_CALL)], [0, 1] * reps, outputs=("ok", "factor", "poses"),
                      cfg=cfg, with_paths=with_paths, yaw=yaw, planner_device=device, planner_timestep=timestep, pose_cap=pose_cap)
    return dict(totals=pb.stat(r, "epilogueDecided", "epilogueHost", "epilogueGroups"), total_ms=r["slot_seconds"][:, :, 2] * 1e3, switches=r["switches"],
                **{k: r[k] for k in ("ok", "factor", "n_poses", "pos", "quat")})
