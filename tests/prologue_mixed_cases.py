"""Shared by tests/test_prologue_mixed_core.py (CPU, the host twins per count), tests/test_gpu_prologue_mixed.py (the
_mixed entries against the uniform entries per count), tests/test_gpu_prologue_mixed_facade.py and
tools/time_mixed_prologue.py (makePlanBatch under BatchOptions::mixedPrologue, at the end of this file): batches of
trajectories of DIFFERENT control-point counts on one world, in rows of Ns control points.

The crafted world is tests/pathsearch_cases.py's (48 x 48 x 24 voxels at 0.1 m, a 16 x 16 x 8 node pool) with one
obstacle per lane, so that a trajectory of any count meets exactly the obstacle of its lane:
    y = -1.2   a block around x = 0            one search around it
    y =  0.0   a cage around x = 0             a closed cell: the search into it fails, the merge with the next segment
    y = +1.2   a wall of 1.8 m across the lane no way round inside the pool: VIGO_PATHS_FAILED
    y = -2.1   nothing
Every count 7, 8, 12, 31, 32, 33, 40, 64, 65, 120 has a trajectory on every lane, a "last point" trajectory (the only
occupied control point is endIdx - 1 of ITS count and the call's not_check_ratio: the (start, N - 1) segment and its
duplicate) and the two largest counts a zigzag (more than VIGO_MAX_COLLISION_SEGS segments at 120: VIGO_PATHS_DEFERRED).
A trajectory of 7 control points can own no segment (endIdx = 3: the scan looks at control point 3 alone, closes nothing
and endIdx - 1 < 3), nor can one of 8 under not_check_ratio 0.3 (endIdx = 3 again); those rows are in the batch all the
same.  Rows are interleaved over the counts, B is odd.  Cases are named and seeded (the seed jitters every line off the
voxel boundaries)."""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import pathsearch_cases as pc
import reguide_cases as rc
from plan_batch import ASTAR as M_ASTAR, GUIDES1 as M_GUIDES1, MIXED_BATCHES as M_MIXED_BATCHES, PROLOGUE as M_PROLOGUE, REGUIDE1 as M_REGUIDE1  # noqa: F401

COUNTS = (7, 8, 12, 31, 32, 33, 40, 64, 65, 120)
NCRS = (0.0, 0.3)
LANE_BLOCK, LANE_CAGE, LANE_WALL, LANE_FREE = -1.2, 0.0, 1.2, -2.1
CRAFTED_SEED = 0x9E0106
DERIVED_COUNTS = (18, 23, 27, 32)
BAD_COUNTS = (6, 0, -1, None, 2 ** 31 - 1)                 # None: Ns + 1


def end_idx(N, ncr):
    return int((N - 4) - ncr * (N - 6))                    # findCollisionSeg's endIdx (csrc/vigo_pathsearch_core.hpp)


def crafted_world():
    vox = np.zeros((48, 48, 24), dtype=np.uint8)
    pc._block(vox, -0.2, 0.2, LANE_BLOCK - 0.3, LANE_BLOCK + 0.3)
    pc._cage(vox, 0.0)
    vox[pc._vi(-0.1):pc._vi(0.1), pc._vi(LANE_WALL - 0.9):pc._vi(LANE_WALL + 0.9), :] |= 1
    return vox, np.array([-2.4, -2.4, 0.0]), 0.1


def _lane_line(N, y, rng):
    """N control points along the lane, centred on x = 0: 0.14 m apart, closer when N of them would leave the world"""
    s = min(0.14, 4.2 / (N - 1))
    c = np.zeros((N, 3))
    c[:, 0] = -0.5 * (N - 1) * s + s * np.arange(N) + rng.uniform(-0.03, 0.03)
    c[:, 1], c[:, 2] = y + rng.uniform(-0.02, 0.02), 1.0
    return c


def _last_point_line(N, ncr, rng):
    """control point endIdx - 1 inside the block, its neighbours 0.3 m away on either side (free), the rest further out"""
    e1 = end_idx(N, ncr) - 1
    if e1 < 3:
        return None
    x = np.zeros(N)
    x[e1] = rng.uniform(-0.1, 0.1)
    s = min(0.14, 1.7 / max(e1 - 1, 1))
    for i in range(e1 - 1, -1, -1):
        x[i] = x[i + 1] - (0.3 if i == e1 - 1 else s)
    for i in range(e1 + 1, N):
        x[i] = x[i - 1] + (0.3 if i == e1 + 1 else 0.14)
    c = np.zeros((N, 3))
    c[:, 0], c[:, 1], c[:, 2] = x, LANE_BLOCK + rng.uniform(-0.02, 0.02), 1.0
    return c


def _zigzag_line(N, rng):
    c = np.zeros((N, 3))
    c[:, 0], c[:, 1], c[:, 2] = rng.uniform(-0.05, 0.05), LANE_BLOCK, 1.0
    c[0::2, 0] = -0.6
    return c


@dataclass
class MixedCase:
    name: str
    vox: np.ndarray
    origin: np.ndarray
    res: float
    cfg: np.ndarray
    ncr: float
    names: List[str]                 # per row
    rows: List[np.ndarray]           # per row its control points [n_b, 3]
    Ns: Optional[int] = None         # the row stride (default: the largest count)
    step_: Optional[float] = None

    def __post_init__(self):
        self.Ns = max(len(r) for r in self.rows) if self.Ns is None else self.Ns

    @property
    def B(self):
        return len(self.rows)

    @property
    def n_pts(self):
        return np.array([len(r) for r in self.rows], dtype=np.int32)

    @property
    def pool(self):
        return tuple(2 * int(self.cfg[3 + a] / self.res) for a in range(3))

    def counts(self):
        return sorted(set(int(n) for n in self.n_pts))

    def rows_of(self, n):
        return [b for b in range(self.B) if len(self.rows[b]) == n]

    def padded(self, poison=False):
        """ctrl [B, Ns, 3]: zeros beyond the counts, or (poison) NaN on the even rows and finite points inside the block of
        the y = -1.2 lane on the odd rows"""
        ctrl = np.zeros((self.B, self.Ns, 3))
        for b, r in enumerate(self.rows):
            ctrl[b, :len(r)] = r
            if poison:
                ctrl[b, len(r):] = np.nan if b % 2 == 0 else self.poison_point()
        return ctrl

    def poison_point(self):
        return np.array([0.03, LANE_BLOCK, 1.0]) if self.name.startswith("crafted") else _occupied_point(self)

    def uniform(self, n, ctrl=None):
        """the rows of count n as a pathsearch_cases.Workload of N = n (ctrl: a padded array to cut them from)"""
        idx = self.rows_of(n)
        c = np.stack([self.rows[b] for b in idx]) if ctrl is None else np.ascontiguousarray(ctrl[idx][:, :n])
        return idx, pc.Workload(f"{self.name}, count {n}", self.vox, self.origin, self.res, np.ascontiguousarray(c), self.cfg, ncr=self.ncr)

    def subset(self, idx, name=None, Ns=None):
        return MixedCase(name or self.name, self.vox, self.origin, self.res, self.cfg, self.ncr, [self.names[b] for b in idx],
                         [self.rows[b] for b in idx], Ns, self.step_)


def _occupied_point(case):
    """the centre of an occupied voxel well inside the grid (the derived batch's poison)"""
    occ = np.argwhere(case.vox[4:-4, 4:-4, 4:-4] & 1)
    return case.origin + (occ[len(occ) // 2] + 4 + 0.5) * case.res


def crafted_case(ncr, counts=COUNTS, seed=CRAFTED_SEED):
    vox, origin, res = crafted_world()
    rng = np.random.default_rng(seed + int(round(100 * ncr)))
    per_count = []
    for n in counts:
        lines = [(f"{n} points, block lane", _lane_line(n, LANE_BLOCK, rng)), (f"{n} points, cage lane", _lane_line(n, LANE_CAGE, rng)),
                 (f"{n} points, wall lane", _lane_line(n, LANE_WALL, rng)), (f"{n} points, free lane", _lane_line(n, LANE_FREE, rng))]
        last = _last_point_line(n, ncr, rng)
        lines.append((f"{n} points, last point", last if last is not None else _lane_line(n, LANE_BLOCK, rng)))
        if n in sorted(counts)[-2:]:
            lines.append((f"{n} points, zigzag", _zigzag_line(n, rng)))
        per_count.append(lines)
    names, rows = [], []
    while any(per_count):                                  # interleaved: neighbouring rows differ in count
        for q in per_count:
            if q:
                nm, c = q.pop(0)
                names.append(nm)
                rows.append(c)
    if len(rows) % 2 == 0:                                 # an odd B
        names.append(f"{counts[0]} points, free lane again")
        rows.append(_lane_line(counts[0], LANE_FREE, rng))
    return MixedCase(f"crafted, not_check_ratio {ncr}", vox, origin, res, pc.CRAFTED_CFG, ncr, names, rows)


def derived_case(n=63, ncr=0.0):
    """reguide_cases.derived_batch's trajectories (pipeline world, 32 control points, moved as by a solve) cut to the counts
    of DERIVED_COUNTS in turn -> (MixedCase, the reguide_cases.Case they were cut from)"""
    base = rc.derived_batch(n)
    rows = [np.ascontiguousarray(base.ctrl[b, :DERIVED_COUNTS[b % len(DERIVED_COUNTS)]]) for b in range(n)]
    m = MixedCase(f"derived, not_check_ratio {ncr}", base.vox, base.origin, base.res, base.cfg, ncr,
                  [f"derived {b}, cut to {len(rows[b])}" for b in range(n)], rows)
    return m, base


# ---- the host twins, per count -------------------------------------------------------------------------------------------
def twin_segments_per_count(lib, case, ctrl=None):
    """vigo_host_collision_segs_core per count -> per row (status, segments [k, 2])"""
    out = [None] * case.B
    for n in case.counts():
        idx, w = case.uniform(n, ctrl)
        r, seg_off, seg, st = pc.twin_segments(lib, w)
        assert r == 0
        for k, b in enumerate(idx):
            out[b] = (int(st[k]), seg[seg_off[k]:seg_off[k + 1]].copy())
    return out


def twin_paths_per_count(lib, case, cap=None, search_path_cap=512):
    """vigo_host_path_search_core per count -> per row (status, segments, [paths], counts[2])"""
    out = [None] * case.B
    for n in case.counts():
        idx, w = case.uniform(n)
        t = pc.twin(lib, w, cap=pc.shipped() if cap is None else cap, search_path_cap=search_path_cap)
        assert t.rc == 0
        for k, b in enumerate(idx):
            out[b] = t.of(k) + (t.counts[k].copy(),)
    return out


# ---- the re-guide: states, weights and guides per row -----------------------------------------------------------------
@dataclass
class ReguideRows:
    state: np.ndarray                # int32 [B, STATE_INTS]
    weights: np.ndarray              # [B, 4]
    pairs: List[dict]                # per row {control point: [(point, direction), ...]}

    def csr(self, case, rows=None, stride=None):
        """the guide CSR of the rows `rows` (default: all) in rows of `stride` (default: the case's Ns) -> (off, pv)"""
        rows = range(case.B) if rows is None else rows
        stride = case.Ns if stride is None else stride
        off, pv = [0], []
        for b in rows:
            for i in range(stride):
                pv += [np.concatenate([np.asarray(p, dtype=float), np.asarray(d, dtype=float)]) for p, d in self.pairs[b].get(i, [])]
                off.append(len(pv))
        return np.array(off, dtype=np.int32), (np.array(pv).reshape(-1, 6) if pv else np.zeros((0, 6)))

    def uniform(self, case, n):
        """the rows of count n as a reguide_cases.Case of N = n"""
        idx = case.rows_of(n)
        off, pv = self.csr(case, idx, n)
        return idx, rc.Case(f"{case.name}, count {n}", case.vox, case.origin, case.res, case.cfg, np.stack([case.rows[b] for b in idx]), off, pv,
                            np.ascontiguousarray(self.weights[idx]), np.ascontiguousarray(self.state[idx]), case.ncr, case.step_)


def reguide_rows(lib, case):
    """a state for every row, by its index: 0 no previous segments and no guides; 1 the scanned segments as the previous
    ones with a near guide on every control point they hold (no list: NOT_REQUIRED); 2 the same with far guides (listed:
    the new pairs go behind the old); 3 not eligible (ACTIVE), with guides.  fail_count, gate_dynamic and weights vary."""
    segs = twin_segments_per_count(lib, case)
    B = case.B
    per_row, pairs = [], []
    for b in range(B):
        kind, c = (0 if "zigzag" in case.names[b] else b % 4), case.rows[b]           # (a zigzag is eligible: DEFERRED at 120)
        sg = [tuple(int(x) for x in s) for s in segs[b][1]][:rc.MAX_SEGS] if kind else []
        per_row.append(sg)
        pp = {}
        for f, s in sg:
            for i in range(max(f, 0), min(s, len(c) - 1) + 1):
                pp[i] = [rc._near(c, i)] if kind == 1 else [rc._far(c, i)] if kind == 2 else [rc._far(c, i), rc._near(c, i)]
        pairs.append(pp)
    st = rc.make_state(B, per_row)
    st[:, rc.S_FAIL] = np.arange(B) % 3
    st[:, rc.S_GATE_DYNAMIC] = (np.arange(B) % 5 == 0)
    st[[b for b in range(B) if b % 4 == 3 and "zigzag" not in case.names[b]], rc.S_STATUS] = rc.RB_ACTIVE
    w = np.ones((B, 4))
    w[:, 0], w[:, 3] = 2.0 ** (np.arange(B) % 3), 1.0 + (np.arange(B) % 2)
    return ReguideRows(st, w, pairs)


# ---- makePlanBatch under mixedPrologue (needs a GPU) -----------------------------------------------------------------
# of plan_batch.STAT_NAMES; guidesAstarDecided: the sum of the two
COUNT_NAMES = ("prologueGroups", "reguideGroups", "prologueDecided", "prologueHost", "reguideDecided", "reguideHost", "guidesAstarDecided", "solveBatches")


def plan_batch_mixed_prologue(world, path_off, xyz, mask, reps=1, budget=16384, cfg=None):
    """makePlanBatch under the options of `mask` with mixedPrologue off (slot 0) and on (slot 1), `reps` rounds over off,
    then on, fresh planners every run -> dict of per-slot arrays; seconds [2, reps, 3]: prologue, chains, the whole call"""
    import plan_batch as pb
    r = pb.plan_batch(world, path_off, xyz, [(mask, budget, pb.BY_CALL), (mask | pb.MIXED_PROLOGUE, budget, pb.BY_CALL)], [0, 1] * reps,
                      outputs=("ok", "solver", "ncp", "ctrl", "segs", "guides", "paths", "poses"), cfg=cfg, with_paths=True, pose_cap=512)
    counts = {k: pb.stat(r, "guidesDecided") + pb.stat(r, "astarDecided") if k == "guidesAstarDecided" else pb.stat(r, k) for k in COUNT_NAMES}
    return dict(counts=counts, seconds=r["slot_seconds"], switches=r["switches"], mixed_prologue_default=(r["switches"] >> 8) & 1,
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_seg", "segs", "n_guides", "guides", "n_path_pts", "paths", "n_poses", "pos", "quat")})
