"""Shared by tests/test_corridor_cases.py (CPU: routing census, trajectory-mode proof obligations),
tests/test_gpu_corridor_cases.py (device against oracle) and tools/fuzz_corridor.py: the named, seeded inputs written to
break k_corridor's certificates (csrc/vigo_corridor_core.hpp) — boundary huggers, box / map_resolution pairs on either
side of the fast path, degrees 0, 3, 5, 7, 9 and 15 (the lowest and the highest the entry accepts), sample counts around the kernel's thresholds, segments scaled to
either side of the span-length thresholds, tiles too large for the LDS, and cancelling polynomials that the float filter
rejects by the thousand — and the same families chained into whole trajectories.  Pure numpy; no GPU, no oracle.

A segment case is (world, metric bounds or None, box, map_res, deg, coeffs, n_samp, delT); a trajectory case carries
[(knots, coeffs [K, 3, deg + 1], delT, endpoint)] in the layout of vigo_traj_corridor_check.  Every segment has a tag
that says which family it comes from; which route of the kernel it takes is predicted by segment_route()
(tests/corridor_restatement.py) and counted by the census."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from corridor_restatement import segment_route

CFG_BOX = (0.4, 0.4, 0.2)         # cfg collision_box / map_resolution
CFG_RES = 0.2
SPAN_BATCH = 64 * 256             # samples of one batch of spans (kBlock spans of 64)


@dataclass
class World:
    name: str
    voxels: np.ndarray            # uint8 [nx, ny, nz]: bit 1 unknown, bit 2 occupied
    origin: np.ndarray
    res: float
    bounds: Optional[tuple]       # interior metric bounds (bmin, bmax) or None: the grid's own

    @property
    def grid(self):
        return tuple(self.voxels.shape), np.asarray(self.origin, np.float64), float(self.res)

    @property
    def metric(self):
        if self.bounds is not None:
            return self.bounds
        return np.asarray(self.origin, np.float64), self.origin + np.array(self.voxels.shape) * self.res


@dataclass
class Case:
    name: str
    world: World
    bounds: Optional[tuple]
    box: tuple
    map_res: float
    deg: int
    coeffs: np.ndarray            # [S, 3, deg + 1]
    n_samp: np.ndarray            # int32 [S]
    delT: np.ndarray              # [S]
    tags: list = field(default_factory=list)      # per segment: the family it comes from

    @property
    def group(self):
        return self.name.split(":")[0]


@dataclass
class TrajCase:
    name: str
    world: World
    bounds: Optional[tuple]
    box: tuple
    map_res: float
    deg: int
    trajs: list                   # [(knots [K + 1], coeffs [K, 3, deg + 1], delT, endpoint [3])]
    tags: Optional[list] = None   # per trajectory, where the census looks for it by name


# ---- worlds ----------------------------------------------------------------------------------------------------------
def make_world(name, seed, n, nz, res, bounded):
    """n x n x nz cells, origin on the key lattice, pillars (occupied) and 8^3 bricks of unknown"""
    rng = np.random.default_rng(seed)
    vox = np.zeros((n, n, nz), dtype=np.uint8)
    for _ in range(n // 5):
        c = rng.integers(2, n - 2, size=2)
        s = rng.integers(1, 4, size=2)
        vox[max(c[0] - s[0], 0):c[0] + s[0], max(c[1] - s[1], 0):c[1] + s[1], 0:rng.integers(nz // 4, nz)] |= 4
    unk = rng.random((n // 8, n // 8, (nz + 7) // 8)) < 0.03
    vox[np.repeat(np.repeat(np.repeat(unk, 8, 0), 8, 1), 8, 2)[:, :, :nz]] |= 2
    origin = np.array([np.round(-n / 2) * res, np.round(-n / 2) * res, np.round(-0.5 / res) * res])
    # free space around the default pose (0, 0, 0) of a trajectory's samples before its first knot
    c0 = np.round(-origin / res).astype(int)
    r = int(np.ceil(0.7 / res))
    vox[max(c0[0] - r, 0):c0[0] + r, max(c0[1] - r, 0):c0[1] + r, max(c0[2] - r, 0):c0[2] + r] = 0
    if n == 96 and res == 0.1:
        # two walls with free space in front of them, for cancelling(): the lattice point that rides the wall's face sees
        # an occupied voxel below the face and a free one above it
        vox[24:40, 40:56, :] = 0
        vox[40:56, 37:50, :] = 0
        vox[26:30, 44:52, :] |= 4
        vox[44:52, 37:41, :] |= 4
    bounds = None
    if bounded:
        top = origin + np.array(vox.shape) * res
        bounds = (origin + np.array([0.43, 0.37, 0.21]), top - np.array([0.39, 0.41, 0.23]))
    return World(name, vox, origin, res, bounds)


_worlds = {}


def worlds():
    """res 0.1 and 0.05; 48 and 96 cells per side; nz a multiple of 32 and not; with and without interior bounds"""
    if not _worlds:
        for w in (make_world("A: 96x96x24 @ 0.1", 1, 96, 24, 0.1, False), make_world("B: 96x96x64 @ 0.05", 2, 96, 64, 0.05, False),
                  make_world("C: 48x48x32 @ 0.1, bounded", 3, 48, 32, 0.1, True),
                  make_world("D: 96x96x40 @ 0.05, bounded", 4, 96, 40, 0.05, True)):
            _worlds[w.name[0]] = w
    return _worlds


# ---- box / map_resolution pairs --------------------------------------------------------------------------------------
BOXES = [
    ("cfg", CFG_BOX, CFG_RES),
    ("multiples 1-2-3 of 0.1", (0.1, 0.2, 0.3), 0.1),
    ("multiples 2-1-3 of 0.2", (0.4, 0.2, 0.6), 0.2),
    ("multiples 2-3-1 of 0.25", (0.5, 0.75, 0.25), 0.25),
    ("multiples 3-1-2 of 0.05", (0.15, 0.05, 0.1), 0.05),
    ("non-multiple / 0.2", (0.55, 0.47, 0.23), 0.2),
    ("non-multiple / 0.25", (0.33, 0.61, 0.17), 0.25),
    ("non-multiple / 0.45", (0.5, 0.95, 0.3), 0.45),
    ("non-multiple / 0.05", (0.12, 0.17, 0.08), 0.05),
    ("more than 3 cells on x only", (0.9, 0.4, 0.2), 0.2),
    ("4 cells on y exactly", (0.4, 0.8, 0.2), 0.2),
    ("just under 4 cells on x", (0.8 - 1e-9, 0.4, 0.2), 0.2),
]


# ---- segment families ------------------------------------------------------------------------------------------------
def _extent(world, box, margin=0.15):
    """where a pose's box stays inside the metric bounds"""
    bmin, bmax = world.metric
    half = np.array(box) / 2 + margin
    return np.asarray(bmin) + half, np.asarray(bmax) - half


def smooth(rng, world, box, deg, n, speed=1.0, dur=None):
    """a chord with a bounded bend, n samples over U(1, 5) s (the family of synth.make_corridor_segments)"""
    lo, hi = _extent(world, box)
    p0 = rng.uniform(lo, hi)
    dur = float(rng.uniform(1.0, 5.0)) if dur is None else dur
    d = rng.normal(size=3)
    d[2] *= 0.1
    d /= np.linalg.norm(d)
    length = rng.uniform(0.3, 0.5 * float(np.min((hi - lo)[:2]))) * speed
    c = np.zeros((3, deg + 1))
    c[:, 0] = p0
    if deg >= 1:
        c[:, 1] = d * length / dur
    for k in range(2, deg + 1):
        amp = rng.uniform(-0.2, 0.2, size=3) / (k - 1) * speed
        amp[2] *= 0.2
        c[:, k] = amp / dur ** k
    return c, int(n), dur / max(int(n), 1)


def hugger(rng, world, box, map_res, deg, n, axis, against, creep, slow_elsewhere, place=None):
    """lattice point i of `axis` rides a voxel face / the metric bound / the grid's last cell while the pose creeps"""
    c, n, dT = smooth(rng, world, box, deg, n, speed=0.02 if slow_elsewhere else 1.0)
    dims, origin, res = world.grid
    bmin, bmax = world.metric
    nlat = int(box[axis] / map_res + 1e-9)
    i = int(rng.integers(0, nlat + 1))
    if against == "face":
        target = origin[axis] + res * float(rng.integers(3, dims[axis] - 3))
    elif against == "bound":
        target = float(bmax[axis]) if rng.random() < 0.5 else float(bmin[axis])
        i = nlat if target == float(bmax[axis]) else 0
    else:                                                      # the last cell of the grid: its lower face
        target = origin[axis] + res * (dims[axis] - 1)
    c[axis, :] = 0.0
    c[axis, 0] = target + box[axis] / 2 - i * map_res + float(rng.choice([0.0, 1e-7, -1e-7, 3e-6, -3e-6]))
    if deg >= 1:
        c[axis, 1] = creep * float(rng.choice([-1.0, 1.0]))
    if place is not None:
        # (cell, offset, start on the other axes): lattice point 0 starts `offset` from the lower face of `cell` and creeps upwards
        cell, offset, start = place
        c[:, 0] = start
        c[axis, 0] = origin[axis] + res * cell + box[axis] / 2 + offset
        c[axis, 1] = abs(creep)
    return c, n, dT


def shifted_chebyshev(deg):
    """power-basis coefficients of T_deg(2 x - 1), x in [0, 1]: they alternate in sign and sum to 1 in absolute value ~ 5.83^deg / 2"""
    P = np.polynomial.Chebyshev.basis(deg).convert(kind=np.polynomial.Polynomial)
    return P(np.polynomial.Polynomial([-1.0, 2.0])).coef


def cancelling(world, box, map_res, deg, n, amp, dur, axis=0, backwards=False, cell=30):
    """a pose that stays within `amp` of a voxel face on `axis`, built from coefficients ~1e11 times larger that cancel:
    A = sum |c_d| T^d exceeds |x| by orders of magnitude, the filter's E = 2^-46 A reaches the spacing of the floats,
    and the flicker across the face keeps the samples away from the span certificates.  backwards: for a clock that
    runs towards -dur (delT < 0)."""
    dims, origin, res = world.grid
    lo, hi = _extent(world, box)
    c = np.zeros((3, deg + 1))
    c[:, 0] = 0.5 * (lo + hi)
    face = origin[axis] + res * cell
    cheb = shifted_chebyshev(deg)
    sgn = -1.0 if backwards else 1.0
    c[axis, :] = amp * cheb / (sgn * dur) ** np.arange(deg + 1)
    c[axis, 0] += face + box[axis] / 2
    dT = dur / (n - 1)
    return c, int(n), -dT if backwards else dT


def diagonal(rng, world, box, k):
    """a long, slow, nearly diagonal segment across the whole map: its tile is the map"""
    lo, hi = _extent(world, box)
    n = int(rng.integers(15000, 20000))
    dur = float(rng.uniform(3.0, 5.0))
    a = np.array([lo[0], lo[1] if k % 2 == 0 else hi[1], rng.uniform(lo[2], hi[2])]) + rng.uniform(0, 0.1, 3) * [1, 1 if k % 2 == 0 else -1, 0]
    b = np.array([hi[0], hi[1] if k % 2 == 0 else lo[1], rng.uniform(lo[2], hi[2])]) - rng.uniform(0, 0.1, 3) * [1, 1 if k % 2 == 0 else -1, 0]
    c = np.zeros((3, 8))
    c[:, 0] = a
    c[:, 1] = (b - a) / dur * 0.9
    c[:, 2] = (b - a) / dur ** 2 * 0.1
    return c, n, dur / n


def _route_scale(c, n, dT, box, map_res, world, factor):
    """scale the moving part of c so that lipmax * factor sits at a quarter voxel: -> c(scale)"""
    r = segment_route(c, n, dT, box, map_res, world.grid)
    s = r["cell"] / (r["lipmax"] * factor)
    out = c.copy()
    out[:, 1:] *= s
    return out


def _case(name, world, box, map_res, deg, segs):
    coeffs = np.ascontiguousarray(np.stack([s[0] for s in segs]))
    return Case(name, world, world.bounds, tuple(box), float(map_res), deg, coeffs, np.array([s[1] for s in segs], np.int32),
                np.array([s[2] for s in segs], np.float64), [s[3] for s in segs])


def _tag(seg, tag):
    return seg[0], seg[1], seg[2], tag


def segment_cases():
    W = worlds()
    out = []
    # -- sample counts around the kernel's thresholds: 16 (a chunk), 512 (lane per sample / spans), 64 x 256 (a batch)
    rng = np.random.default_rng(101)
    segs = []
    for n in (0, 1, 15, 16, 17, 511, 512, 513, 1025, SPAN_BATCH - 1, SPAN_BATCH, SPAN_BATCH + 1, 2 * SPAN_BATCH + 63):
        segs.append(_tag(smooth(rng, W["A"], CFG_BOX, 7, n, speed=0.5), f"count {n}"))
    for n in (511, 512, 513, 1025, 3000):
        segs.append(_tag(smooth(rng, W["A"], CFG_BOX, 7, n), f"count {n}"))
    out.append(_case("counts: around 16, 512 and a batch of spans", W["A"], CFG_BOX, CFG_RES, 7, segs))

    # -- routing edges: lipmax just either side of the thresholds that choose S1 = 64 / 32 / 16 / none, and everything PASS 0 refuses
    for wname, seed in (("A", 102), ("D", 103)):
        rng = np.random.default_rng(seed)
        w = W[wname]
        segs = []
        for factor, names in ((32.0, ("S1 64", "S1 32")), (16.0, ("S1 32", "S1 16")), (8.0, ("S1 16", "S1 none"))):
            for k in range(3):
                c, n, dT = smooth(rng, w, CFG_BOX, 7, int(rng.integers(1500, 3000)))
                for side, nm in zip((1.0 - 1e-3, 1.0 + 1e-3), names):
                    segs.append((_route_scale(c, n, dT, CFG_BOX, CFG_RES, w, factor / side), n, dT, f"edge {nm} (x{factor:g}, {side - 1:+.0e})"))
        for k in range(2):
            c, n, dT = smooth(rng, w, CFG_BOX, 7, 2000)
            c[:, 1:] *= 40.0
            segs.append((c, n, dT, "fast"))
        c, n, dT = smooth(rng, w, CFG_BOX, 7, 2500)
        c[0, 1] = 1.5 * (w.metric[1][0] - w.metric[0][0]) / (n * dT)
        segs.append((c, n, dT, "leaves the map"))
        c, n, dT = smooth(rng, w, CFG_BOX, 7, 2500)
        c[1, 0] = w.origin[1] - 0.35
        c[1, 1] = abs(c[1, 1]) + 0.3
        segs.append((c, n, dT, "starts outside"))
        c, n, dT = smooth(rng, w, CFG_BOX, 7, 2500)
        c[:, 1:] = 0.0
        segs.append((c, n, dT, "stationary"))
        for nm, f in (("clock 0", lambda d: 0.0), ("clock negative", lambda d: -d), ("clock x 1e-9", lambda d: d * 1e-9),
                      ("clock below 2^-1000", lambda d: 1e-305), ("clock NaN", lambda d: np.nan), ("clock infinite", lambda d: np.inf),
                      ("clock 1e300", lambda d: 1e300)):
            c, n, dT = smooth(rng, w, CFG_BOX, 7, 1500)
            segs.append((c, n, f(dT), nm))
        for val in (np.nan, np.inf, -np.inf, 1e300, 1e39, -4e38, 1e20, 3.4028234e38):
            c, n, dT = smooth(rng, w, CFG_BOX, 7, int(rng.choice([400, 1500])))
            c[int(rng.integers(0, 3)), int(rng.integers(0, 8))] = val
            segs.append((c, n, dT, f"coefficient {val:g}"))
        out.append(_case(f"routing: {wname}", w, CFG_BOX, CFG_RES, 7, segs))

    # -- huggers: every axis, against faces, the metric bound and the last cell, creep 0 .. 1e-3 m/s
    for wname, bi, seed in (("C", 0, 104), ("D", 4, 105), ("A", 2, 106), ("B", 5, 107)):
        rng = np.random.default_rng(seed)
        w = W[wname]
        _, box, mres = BOXES[bi]
        segs = []
        for axis in range(3):
            for j, creep in enumerate((0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3)):
                for against in (("face", "bound") if j % 2 == 0 else ("face", "rim")):
                    slow = bool((j + axis) % 2)
                    n = int(rng.choice([400, 1200, 3000]))
                    segs.append(_tag(hugger(rng, w, box, mres, 7, n, axis, against, creep, slow),
                                     f"hugger {'xyz'[axis]} {against} creep {creep:g}{' slow' if slow else ''}"))
        for k in range(4):
            segs.append(_tag(smooth(rng, w, box, 7, 2000), "smooth"))
        out.append(_case(f"huggers: {wname} / {BOXES[bi][0]}", w, box, mres, 7, segs))

    # -- every box / map_res pair, degrees 3, 5, 9 with the non-default ones
    for bi, (bname, box, mres) in enumerate(BOXES):
        rng = np.random.default_rng(200 + bi)
        w = W["ABCD"[bi % 4]]
        deg = 7 if bi == 0 else (3, 5, 9)[bi % 3]
        segs = []
        for n in (300, 700, 2000, 2000, 5000, 5000):
            segs.append(_tag(smooth(rng, w, box, deg, n, speed=0.6), "smooth"))
        for axis in range(3):
            segs.append(_tag(hugger(rng, w, box, mres, deg, 1500, axis, "face", (1e-6, 1e-4, 0.0)[axis], True), f"hugger {'xyz'[axis]} face"))
        c, n, dT = smooth(rng, w, box, deg, 1500)
        c[:, 1:] *= 40.0
        segs.append((c, n, dT, "fast"))
        c, n, dT = smooth(rng, w, box, deg, 1500)
        c[0, 1] = 1.5 * (w.metric[1][0] - w.metric[0][0]) / (n * dT)
        segs.append((c, n, dT, "leaves the map"))
        out.append(_case(f"boxes: {bname}, degree {deg}", w, box, mres, deg, segs))

    # -- the lowest and the highest degree the entry accepts
    for deg, seed in ((0, 301), (15, 302)):
        rng = np.random.default_rng(seed)
        for bi, wname in ((0, "A"), (3, "C")):
            _, box, mres = BOXES[bi]
            w = W[wname]
            segs = [_tag(smooth(rng, w, box, deg, n, speed=0.5), "smooth") for n in (1, 100, 512, 600, 1500, 1500, 2500, 2500)]
            if deg == 0:
                segs += [_tag(smooth(rng, w, box, deg, 700), "stationary") for _ in range(8)]
            else:
                segs += [_tag(hugger(rng, w, box, mres, deg, 1200, a, "face", 1e-5, True), f"hugger {'xyz'[a]} face") for a in range(3)]
            out.append(_case(f"degrees: {deg} / {BOXES[bi][0]} / {wname}", w, box, mres, deg, segs))

    # -- a tile too large for the LDS under a segment slow enough for certificates: long diagonals at resolution 0.05
    rng = np.random.default_rng(401)
    w = W["B"]
    _, box, mres = BOXES[5]
    lo, hi = _extent(w, box)
    segs = [(*diagonal(rng, w, box, k), "long diagonal") for k in range(6)]
    segs += [_tag(smooth(rng, w, box, 7, 3000), "smooth") for _ in range(3)]
    out.append(_case("tile: too large for the LDS", w, box, mres, 7, segs))

    # -- filter rejections: cancelling polynomials of the highest degree about a voxel face
    w = W["A"]
    _, box, mres = BOXES[5]                                  # (a non-multiple box: the counts cannot vary, every piece is decided or open)
    segs = [
        (*cancelling(w, box, mres, 15, 3000, 2e-7, 3.0), "cancelling: modest"),
        (*cancelling(w, box, mres, 15, 20000, 1e-4, 4.0), "cancelling: many"),
        (*cancelling(w, box, mres, 15, 20000, 3e-5, 4.0, axis=1, cell=41), "cancelling: many, y"),
        (*cancelling(w, box, mres, 15, 500, 1e-4, 2.0), "cancelling: n <= 512"),
        (*cancelling(w, box, mres, 15, 2000, 2e-7, 2.0, backwards=True), "cancelling: clock negative, modest"),
        (*cancelling(w, box, mres, 15, 3000, 1e-4, 2.0, backwards=True), "cancelling: clock negative, many"),
    ]
    rng = np.random.default_rng(501)
    segs += [_tag(smooth(rng, w, box, 15, 1500), "smooth") for _ in range(4)]
    for k in range(2):                                       # (in the free space in front of the first wall)
        c, n, dT = smooth(rng, w, box, 15, 600, speed=0.0)
        c[:, 0] = [w.origin[0] + 0.1 * (34 + k), 0.0, 0.6]
        segs.append((c, n, dT, "stationary, free"))
    out.append(_case("filter: rejections by the exact-power queue", w, box, mres, 15, segs))
    for c in out:
        assert len(c.n_samp) <= 40 and c.n_samp.max() <= 2 * SPAN_BATCH + 63, c.name
    return out


# ---- trajectories ----------------------------------------------------------------------------------------------------
def _eval(c, t):
    return (c * t ** np.arange(c.shape[1])).sum(-1)


def chain(rng, world, box, deg, durs, speed=0.3, k0=0.0, first=None):
    """len(durs) segments end to end (segment i + 1 starts where segment i ends) -> (knots, coeffs, endpoint)"""
    cs = []
    for i, dur in enumerate(durs):
        c, _, _ = smooth(rng, world, box, deg, 100, speed=speed, dur=dur) if (first is None or i > 0) else (first.copy(), 0, 0)
        if i > 0:
            c[:, 0] = _eval(cs[-1], durs[i - 1])
        cs.append(c)
    knots = k0 + np.concatenate([[0.0], np.cumsum(durs)])
    return knots, np.stack(cs), _eval(cs[-1], durs[-1])


def traj_cases():
    W = worlds()
    out = []
    rng = np.random.default_rng(601)
    # -- plain: 1 to 6 segments, a few hundred samples each; delT does not divide the durations
    for wname, bi, deg in (("A", 0, 7), ("C", 2, 5), ("D", 8, 7)):
        w = W[wname]
        _, box, mres = BOXES[bi]
        trajs = []
        for K in (1, 2, 3, 4, 5, 6):
            durs = rng.uniform(0.6, 2.0, size=K)
            kn, co, ep = chain(rng, w, box, deg, durs)
            trajs.append((kn, co, float(rng.choice([0.0137, 0.0049, 0.0101])), ep))
        # samples exactly on the knots: binary fractions
        kn, co, ep = chain(rng, w, box, deg, [0.5, 0.75, 1.25, 0.5])
        trajs.append((kn, co, 2.0 ** -8, ep))
        kn, co, ep = chain(rng, w, box, deg, [1.0, 1.0, 2.0])
        trajs.append((kn, co, 2.0 ** -10, ep))                    # 1024 / 2048 samples per run: certified spans, cut on the knots
        out.append(TrajCase(f"plain {wname} / {BOXES[bi][0]} / degree {deg}", w, w.bounds, box, mres, deg, trajs))
    # -- one long hugging trajectory and slow company: runs of thousands of samples
    for wname, bi in (("A", 0), ("D", 4)):
        w = W[wname]
        _, box, mres = BOXES[bi]
        trajs = []
        for axis, creep in ((0, 1e-6), (1, 1e-4), (2, 1e-7)):
            h, _, _ = hugger(rng, w, box, mres, 7, 100, axis, "face", creep, True)
            kn, co, ep = chain(rng, w, box, 7, [14.0, 9.0], speed=0.05, first=h)
            trajs.append((kn, co, 0.004, ep))
        out.append(TrajCase(f"long huggers {wname} / {BOXES[bi][0]}", w, w.bounds, box, mres, 7, trajs))
    # -- large knots: the drift of the subtracted clock dominates 2 E; huggers whose creep per sample is of its order
    for wname, bi, k0, dT in (("A", 0, 1000.0, 0.004), ("C", 5, 4096.0, 0.008)):
        w = W[wname]
        _, box, mres = BOXES[bi]
        trajs = []
        for axis, creep in ((0, 1e-7), (1, 3e-7), (2, 0.0))[:3 if k0 < 2000 else 2]:
            # (world A: the first one against the wall of make_world — occupied below the face, free above it — starting
            # 0.2 um below the face and crossing it at 0.1 um/s, a few float spacings over the run)
            place = (30, -2e-7, [0.0, 0.0, 0.6]) if wname == "A" and axis == 0 else None
            h, _, _ = hugger(rng, w, box, mres, 7, 100, axis, "face", creep, True, place=place)
            kn, co, ep = chain(rng, w, box, 7, [4.5, 6.0, 2.5], speed=0.05, k0=k0 + 0.37 * axis, first=h)
            trajs.append((kn, co, dT, ep))
        kn, co, ep = chain(rng, w, box, 7, [5.0, 5.0], speed=0.3, k0=k0)
        trajs.append((kn, co, dT, ep))
        out.append(TrajCase(f"large knots {k0:g} {wname} / {BOXES[bi][0]}", w, w.bounds, box, mres, 7, trajs))
    # -- a box of more than 3 map cells on one axis: every run is PASS 1's
    w = W["A"]
    _, box, mres = BOXES[9]
    trajs = []
    for K in (1, 2, 3, 4, 5, 6):
        kn, co, ep = chain(rng, w, box, 3, rng.uniform(0.6, 3.0, size=K))
        trajs.append((kn, co, 0.004, ep))
    out.append(TrajCase(f"box {BOXES[9][0]} A / degree 3", w, w.bounds, box, mres, 3, trajs))
    # -- non-finite and huge coefficients: the runs that carry them are PASS 1's, and nonfinite_collides decides their poses
    trajs = []
    for j, val in enumerate((np.nan, np.inf, -np.inf, 1e300, 1e39, -4e38, 1e20, 3.4028234e38, np.nan, 1e300)):
        kn, co, ep = chain(rng, w, CFG_BOX, 7, [float(rng.uniform(0.8, 1.6)), float(rng.uniform(1.0, 3.0))])
        co[1 if j < 8 else 0, int(rng.integers(0, 3)), 7 if val == 1e300 else int(rng.integers(0, 8))] = val
        if j == 3:
            kn = np.array([0.0, kn[1], kn[1] + 40.0])        # 1e300 t^7 overflows late in the run
        trajs.append((kn, co, 0.004 if j != 3 else 0.05, ep if j != 5 else np.array([np.nan, 0.0, 1.0])))
    out.append(TrajCase("non-finite coefficients A / cfg", w, w.bounds, CFG_BOX, CFG_RES, 7, trajs))
    # -- cancelling polynomials on a run: the exact-power queue in trajectory mode, from the sample clock fl(t - k[i])
    _, box, mres = BOXES[5]
    trajs = []
    for nm, n, amp, dur, axis, cell in (("modest", 3000, 2e-7, 3.0, 0, 30), ("many, y", 20000, 3e-5, 4.0, 1, 41), ("many", 20000, 1e-4, 4.0, 0, 30),
                                        ("n <= 512", 500, 1e-4, 2.0, 0, 30)):
        c1, n1, dT = cancelling(w, box, mres, 15, n, amp, dur, axis=axis, cell=cell)
        c0, _, _ = smooth(rng, w, box, 15, 100, speed=0.3, dur=0.75)
        trajs.append((np.array([0.0, 0.75, 0.75 + dur]), np.stack([c0, c1]), dT, _eval(c1, dur), f"cancelling: {nm}"))
    out.append(TrajCase("cancelling runs A / non-multiple / 0.2 / degree 15", w, w.bounds, box, mres, 15, [t[:4] for t in trajs]))
    out[-1].tags = [t[4] for t in trajs]
    # -- a tile too large for the LDS under runs slow enough for certificates
    w = W["B"]
    trajs = []
    for k in range(2):
        c, n, dT = diagonal(rng, w, box, k)
        trajs.append((np.array([0.0, n * dT]), c[None], dT, _eval(c, n * dT)))
    out.append(TrajCase("tile B / non-multiple / 0.2", w, w.bounds, box, mres, 7, trajs))
    return out


def face_poses(world, box, map_res, rng, count=60):
    """poses whose lattice points sit exactly on voxel faces, the metric bounds and the grid's rim, +- one float ulp"""
    dims, origin, res = world.grid
    bmin, bmax = world.metric
    lo, hi = _extent(world, box)
    pts = []
    for _ in range(count):
        p = rng.uniform(lo, hi)
        axis = int(rng.integers(0, 3))
        nlat = int(box[axis] / map_res + 1e-9)
        i = int(rng.integers(0, nlat + 1))
        kind = int(rng.integers(0, 4))
        target = (origin[axis] + res * float(rng.integers(1, dims[axis])), float(bmin[axis]), float(bmax[axis]),
                  origin[axis] + res * dims[axis])[kind]
        x = np.float32(target + box[axis] / 2 - i * map_res)
        for v in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
            q = p.copy()
            q[axis] = float(v)
            pts.append(q)
    return np.array(pts)
