"""The case families of tests/gate_cases.py are about what their names say: asserted here from the inputs and the CPU
oracle alone (no device).  Sample counts, the marked voxel's uniqueness among earlier samples, the lane order of the
pairs, the clocks' last steps, the boundary constructions of the dynamic gate, the step-count and reciprocal
sensitivity counts, and that every expectation fixed by construction is the oracle's too.  A minimum per family keeps a
later edit from hollowing one out."""
import numpy as np

import gate_cases as gc
from trajectory_planner_amd import synth


def _accumulate(dt, n):
    """t_0 .. t_n of the k-fold sum t += dt"""
    t, out = 0.0, [0.0]
    for _ in range(n):
        t = t + dt
        out.append(t)
    return out


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def _check_marks(c):
    """T is the promised count; each marked voxel is met by no earlier sample of its trajectory and by no sample of
    another; the oracle's verdict is the construction's"""
    tmax = gc.duration(c.N, c.ts_ctrl)
    times = gc.sample_times(tmax, c.dt)
    assert len(times) == c.T, (c.name, len(times))
    acc = _accumulate(c.dt, c.T)
    assert acc[c.T - 1] <= tmax < acc[c.T] and np.array_equal(times, acc[:c.T])
    vox = [gc.voxel_of(c.world, gc.positions(c.ctrl[b], c.ts_ctrl, times)) for b in range(c.B)]
    n = np.array(c.world.voxels.shape)
    for b in range(c.B):
        assert np.all((vox[b] >= 0) & (vox[b] < n)), (c.name, b)                      # the trajectory stays inside the map
        for k in c.marks[b]:
            assert not np.any(np.all(vox[b][:k] == vox[b][k], axis=1)), (c.name, b, k)
            for other in range(c.B):
                assert other == b or not np.any(np.all(vox[other] == vox[b][k], axis=1)), (c.name, b, k, other)
    assert int((c.world.voxels & 1).sum()) == len({(b, tuple(vox[b][k])) for b in range(c.B) for k in c.marks[b]}) or c.world.voxels.all()
    flag, first = gc.oracle_static(c)
    assert np.array_equal(flag, c.exp_flag), c.name
    if c.exp_first is not None:
        assert np.array_equal(first, c.exp_first), (c.name, first)


def test_first_hit_family():
    cases = gc.first_hit_cases()
    assert [c.T for c in cases[:6]] == [65, 64, 63, 61, 128, 129]
    singles = pairs = 0
    for c in cases:
        _check_marks(c)
        for b, m in enumerate(c.marks):
            if len(m) == 1:
                singles += 1
                assert c.exp_first[b] == m[0]
            elif len(m) == 2:
                pairs += 1
                a, z = m
                assert a < z and a % 64 > z % 64 and c.exp_first[b] == a               # the earlier sample on the higher lane
    marked = {m[0] for c in cases for m in c.marks if len(m) == 1}
    assert {0, 1, 62, 63, 64, 65} <= marked
    assert all(c.T - 1 in {m[0] for m in c.marks if len(m) == 1} for c in cases[:6])   # a hit at T - 1 alone, per shape
    assert singles >= 33 and pairs >= 5
    assert {tuple(c.exp_first) for c in cases[6:]} == {(-1, -1, -1), (0, 0, 0)}


def test_clock_family():
    cases = gc.clock_cases()
    exact = [c for c in cases if c.notes["kind"] == "ends on tmax"]
    over = [c for c in cases if c.notes["kind"] != "ends on tmax"]
    assert len(exact) >= 2 and len(over) >= 3
    for c in cases:
        _check_marks(c)
        assert c.marks[0] == (c.T - 1,) and c.exp_first[0] == c.T - 1
        tmax = gc.duration(c.N, c.ts_ctrl)
        acc = _accumulate(c.dt, c.T)
        if c in exact:
            assert acc[c.T - 1] == tmax, c.name                                        # bit for bit
        else:
            assert acc[c.T - 1] < tmax < acc[c.T] and _ulps(acc[c.T], tmax) <= 4, (c.name, _ulps(acc[c.T], tmax))


def test_ratio_case():
    c = gc.ratio_case()
    tmax = gc.duration(c.N, c.ts_ctrl)
    bound = (1.0 - c.ncr) * tmax                                                       # BT.h:313
    acc = _accumulate(c.dt, c.T)
    ts = c.notes["T_static"]
    assert acc[ts - 1] <= bound < acc[ts] and ts < c.T
    assert c.marks == [(ts - 1,), (ts,)]
    _check_marks(c.__class__(**{**c.__dict__, "exp_flag": np.array([1, 1], dtype=np.uint8)}))   # the full clock meets both


def test_eval_family():
    cases = gc.eval_cases()
    assert {c.ts_ctrl for c in cases} == set(gc.TS_CTRL) and {c.N for c in cases} == set(gc.EVAL_N)
    assert len(cases) == len(gc.TS_CTRL) * len(gc.EVAL_N)
    inexact = 0
    for c in cases:
        nk = c.n_knots
        dur = gc.duration(c.N, c.ts_ctrl)
        assert nk == c.N - 2 and c.ctrl.shape == (3, c.N, 3)
        assert all(c.times[j] == j * c.ts_ctrl for j in range(nk)) and c.times[nk - 1] == dur
        assert np.all(c.times[nk:2 * nk] < c.times[:nk]) and np.all(c.times[2 * nk:3 * nk] > c.times[:nk])
        edge = c.times[3 * nk:]
        assert np.signbit(edge[0]) and edge[0] == 0.0 and edge[1] < 0 and edge[2] == dur and edge[3] > dur > edge[4] and edge[5] == dur + 1.0
        # the lower span at an exact knot: the value at knot j is the one approached from below, and (a cubic spline is
        # continuous) the next double above evaluates in the upper span to nearly the same point
        inexact += sum(1 for j in range(1, nk) if (j * c.ts_ctrl) / c.ts_ctrl != j or (j * c.ts_ctrl - (j - 1) * c.ts_ctrl) != c.ts_ctrl)
    assert inexact >= 100                                                              # knot arithmetic that does round
    small = [c for c in cases if c.N <= 8]
    for c in small:
        ref = gc.oracle_eval(c, 0)
        assert np.all(np.isfinite(ref))
        assert np.array_equal(ref[:, 3 * c.n_knots], ref[:, 0]) and np.array_equal(ref[:, 3 * c.n_knots + 1], ref[:, 0])      # clamped at 0
        assert np.array_equal(ref[:, 3 * c.n_knots + 5], ref[:, c.n_knots - 1])                                               # and at dur


def test_nonfinite_family():
    c = gc.nonfinite_case()
    assert c.B == 15 and len(c.notes["where"]) == 15
    seen = set()
    clean = c.notes["clean"]
    times = gc.sample_times(gc.duration(c.N, c.ts_ctrl), c.dt)
    n = np.array(c.world.voxels.shape)
    for b, (i, axis, k) in enumerate(c.notes["where"]):
        bad = ~np.isfinite(c.ctrl[b]) | (np.abs(c.ctrl[b]) >= 1e300)
        assert bad.sum() == 1 and bad[i, axis] and i in (0, 3, c.N - 1)
        seen.add((i, repr(float(c.ctrl[b, i, axis]))))
        v = gc.voxel_of(c.world, clean[b])
        assert np.all((v >= 0) & (v < n))                                              # the clean points are inside, and free
        # the obstacle's sample lies in the spans the bad point shapes, and is the only one the obstacle reaches
        assert (i - 3) * c.ts_ctrl < times[k] < (i + 1) * c.ts_ctrl
        d = [gc.gate_distance(p, c.obs[b]) for p in gc.positions(clean[b], c.ts_ctrl, times)]
        assert d[k] == 0.0 and sorted(d)[1] > c.obs[b, 6] / 2
    assert len(seen) == 15 and not c.world.voxels.any()
    pt, line = gc.oracle_occupancy(c.world, c.ctrl)
    assert np.array_equal(pt, c.exp_pt) and np.array_equal(line, c.exp_line)          # the contract's verdict is the oracle's
    assert c.exp_pt.sum() == 15 and c.exp_line.sum() == 5 + 10 + 5
    flag, first = gc.oracle_static(c)
    assert np.array_equal(flag, c.exp_flag)
    dyn = gc.oracle_dynamic(c)
    assert np.array_equal(dyn, c.exp_dyn) and dyn.sum() == 5
    cl = gc.GateCase(c.name, c.world, c.ts_ctrl, c.N, c.dt, clean, obs_off=c.obs_off, obs=c.obs)
    assert gc.oracle_dynamic(cl).all() and not gc.oracle_static(cl)[0].any()           # without the bad coordinate: hit, and free


def test_dynamic_family():
    cases = {c.name.split(":")[1]: c for c in gc.dynamic_cases()}
    assert len(cases) >= 5
    for c in cases.values():
        assert np.array_equal(gc.oracle_dynamic(c), c.exp_dyn), c.name
        flag, first = gc.oracle_static(c)
        assert not flag.any() and np.all(first == -1)
        assert len(gc.sample_times(gc.duration(c.N, c.ts_ctrl), c.dt)) == c.T
    lists = cases["lists, empty at the first, a middle and the last trajectory"]
    n = np.diff(lists.obs_off)
    assert n[0] == 0 and n[-1] == 0 and n[4] == 0 and n.max() >= 3 and 0 < lists.exp_dyn.sum() < lists.B
    shared, copies, none = cases["shared list"], cases["copies of the shared list"], cases["no obstacles"]
    assert shared.obs_off is None and shared.obs is not None and none.obs is None and none.obs_off is None
    assert np.array_equal(copies.obs, np.tile(shared.obs, (copies.B, 1))) and np.array_equal(np.diff(copies.obs_off), np.full(copies.B, len(shared.obs)))
    assert np.array_equal(shared.exp_dyn, copies.exp_dyn) and not np.array_equal(shared.exp_dyn, lists.exp_dyn) and 0 < shared.exp_dyn.sum() < shared.B
    e = cases["edges of the hit test"]
    times = gc.sample_times(gc.duration(e.N, e.ts_ctrl), e.dt)
    pos = [gc.positions(e.ctrl[b], e.ts_ctrl, times) for b in range(e.B)]
    # the strict boundary: dist - size is 0 at one sample (no hit), negative one ulp further (hit); no other sample is closer
    for b, want in ((0, 0), (1, 1)):
        o = e.obs_of(b)[0]
        k = e.notes["boundary"][b]
        d = np.array([gc.gate_distance(p, o) for p in pos[b]])
        size = min(o[6] / 2, o[7] / 2)
        assert int(np.argmin(d)) == k and (d - size < 0).sum() == want
        assert (d[k] - size == 0.0) if b == 0 else (size == np.nextafter(d[k], np.inf))
    # the minimum of the two sizes: the larger alone would hit
    for b in (2, 3):
        o = e.obs_of(b)[0]
        d = np.array([gc.gate_distance(p, o) for p in pos[b]])
        assert (d - min(o[6], o[7]) / 2 < 0).sum() == 0 and (d - max(o[6], o[7]) / 2 < 0).sum() > 0
    assert sorted((e.obs_of(2)[0][6] > 1, e.obs_of(3)[0][6] > 1)) == [False, True]   # both orders
    assert e.obs_of(4)[0][2] - pos[4][30][2] == 50.0 and e.exp_dyn[4] == 1
    # one sample alone inside
    for b, k in e.notes["single"].items():
        o = e.obs_of(b)[0]
        d = np.array([gc.gate_distance(p, o) for p in pos[b]])
        assert list(np.nonzero(d - min(o[6], o[7]) / 2 < 0)[0]) == [k] and min(o[6], o[7]) / 2 < e.notes["spacing"] / 2
    assert set(e.notes["single"].values()) == {0, 63, 64} and e.T - 1 == 64
    o = e.obs_of(8)
    hits = [any(gc.gate_distance(p, r) - min(r[6], r[7]) / 2 < 0 for p in pos[8]) for r in o]
    assert len(o) == 40 and hits == [False] * 39 + [True]
    assert np.all(e.obs_of(9)[:, 6:8].min(axis=1) < 0) and e.exp_dyn[9] == 0 and gc.gate_distance(pos[9][12], e.obs_of(9)[0]) == 0.0


def test_occupancy_family():
    cases = gc.occupancy_cases()
    assert len(cases) >= 6
    for c in cases:
        pt, line = gc.oracle_occupancy(c.world, c.ctrl)
        if c.exp_pt is not None:
            assert np.array_equal(pt, c.exp_pt), c.name
        if c.exp_line is not None:
            assert np.array_equal(line, c.exp_line), c.name
        assert not line[:, 0].any()
        for b in range(c.ctrl.shape[0]):                                               # the numpy walk is the oracle's
            for i in range(1, c.ctrl.shape[1]):
                assert gc.line_walk(c.world, c.ctrl[b, i - 1], c.ctrl[b, i])[0] == line[b, i], (c.name, b, i)
    wall = cases[0]
    B, N = wall.ctrl.shape[:2]
    assert (B, N) == (75, 7) and B * N > 2 * 256                                       # trajectories straddle the blocks' borders
    assert {(256 * j) % N for j in (1, 2)} != {0}
    crossing = [gc.oracle_line(wall.world, wall.ctrl[b, N - 1], wall.ctrl[b + 1, 0]) for b in range(B - 1)]
    assert all(v == 1 for v in crossing) and not wall.exp_line.any()                   # a kernel reading p - 3 at i = 0 would see the wall
    # own lines do walk: two voxels apart, a probe in between
    assert gc.line_walk(wall.world, wall.ctrl[0, 0], wall.ctrl[0, 1])[1] >= 2
    probes = cases[1]
    assert np.array_equal(probes.ctrl[0, 0], probes.ctrl[0, 1]) and probes.exp_line[0, 1] == 0
    for b, s in probes.notes["one_probe"].items():
        flag, steps, hits = gc.line_walk(probes.world, probes.ctrl[b, 0], probes.ctrl[b, 1])
        assert flag == 1 and hits == [s] and s in (1, steps - 1)
    assert {1} <= set(probes.notes["one_probe"].values()) and any(gc.line_walk(probes.world, probes.ctrl[b, 0], probes.ctrl[b, 1])[1] - 1 == s > 1
                                                                   for b, s in probes.notes["one_probe"].items())
    assert gc.line_walk(probes.world, probes.ctrl[1, 0], probes.ctrl[1, 1], first=2)[0] == 0   # a walk from s = 2 misses it
    # the step count next to an integer: how many lines change their flag when steps changes by one
    sensitive, below, reached = 0, 0, 0
    for c in cases:
        if "step count" not in c.name:
            continue
        for b, m in enumerate(c.notes["m"]):
            q, p = c.ctrl[b, 0], c.ctrl[b, 1]
            flag, steps, hits = gc.line_walk(c.world, q, p)
            assert steps in (m - 1, m) and flag == (1 if steps == m else 0)
            below += steps == m - 1
            reached += steps == m
            if gc.line_walk(c.world, q, p, steps_delta=-1)[0] != flag or gc.line_walk(c.world, q, p, steps_delta=1)[0] != flag:
                sensitive += 1
    assert sensitive >= 20 and below >= 3 and reached >= 3, (sensitive, below, reached)
    one = cases[-1]
    assert one.ctrl.shape[1] == 1 and one.exp_pt.sum() == 2


def test_lookup_family():
    cases = gc.lookup_cases()
    assert {c.world.voxels.shape[2] for c in cases} == {1, 31, 32, 33, 64, 65, 95}
    assert {1, 2} <= {c.world.voxels.shape[0] for c in cases} and {1, 2} <= {c.world.voxels.shape[1] for c in cases}
    faces, sensitive, total = [0] * 4, [0] * 4, 0
    for c in cases:
        w, nf = c.world, c.n_face
        assert w.res == gc.RESOLUTIONS[c.pair]
        on = np.all(np.round(w.origin / w.res) * w.res == w.origin)
        assert on == (c.pair % 2 == 1)
        i, j, k = np.meshgrid(*[np.arange(n) for n in w.voxels.shape], indexing="ij")
        assert np.array_equal(w.voxels & 1, ((i + j + k) & 1).astype(np.uint8))       # every single-axis off-by-one flips bit 0
        assert np.array_equal(np.nextafter(c.pts[:nf], -np.inf), c.pts[nf:2 * nf]) and np.array_equal(np.nextafter(c.pts[:nf], np.inf), c.pts[2 * nf:3 * nf])
        for bit in (0, 1):
            ref = gc.oracle_lookup(w, c.pts, bit)
            assert np.array_equal(ref, gc.numpy_lookup(w, c.pts, bit)), (c.name, bit)
            with np.errstate(invalid="ignore", over="ignore"):
                assert np.array_equal(ref, synth.lookup(w, c.pts, bit)), (c.name, bit)  # the second CPU reference
            fin = np.all(np.isfinite(c.pts) & (np.abs(c.pts) < 1e299), axis=1)
            assert (~fin).sum() == 15 and np.all(ref[~fin] == 1)                       # not finite, or far away: outside
        total += len(c.pts)
        sp = c.pts[3 * nf:]
        assert np.array_equal(sp[0], w.origin) and gc.numpy_lookup(w, sp[0], 0) == (w.voxels[0, 0, 0] & 1)
        assert gc.numpy_lookup(w, sp[1], 0) == 1 and gc.numpy_lookup(w, sp[1], 1) == 1   # the upper corner is outside
        assert np.all(np.signbit(sp[2])) and np.signbit(sp[3][2])
        face = c.pts[:nf]
        a, b = gc.voxel_of(w, face), np.floor((face - w.origin) * (1.0 / w.res))
        n = np.array(w.voxels.shape)
        inmap = np.all((a >= 0) & (a < n), axis=1)
        faces[c.pair] += nf
        sensitive[c.pair] += int((inmap & np.any(a != b, axis=1)).sum())
    assert min(faces) >= 1000 and min(sensitive) >= 100, (faces, sensitive)
    assert total >= 4 * 3000


def test_inflate_family():
    cases = gc.inflate_cases()
    assert len(cases) >= 12
    names = " ".join(c.name for c in cases)
    for word in ("rz = 31", "rz >= nz", "rx >= nx", "ry >= ny", "nx = 1", "(0, 0, 0)", "(5, 4, 69)", "(3, 2, 31)", "(3, 2, 32)"):
        assert word in names
    assert {c.vox.shape[2] for c in cases if c.r[2] == 31} == {33, 64, 70}
    for c in cases:
        occ = (c.vox & 4) != 0
        ref = gc.dilate_reference(occ, c.r)
        assert occ.any() and ref.sum() > occ.sum()
        # dilate_reference against the definition: a voxel is set when an occupied one lies within r on every axis
        idx = np.argwhere(occ)
        want = np.zeros_like(occ)
        for i, j, k in idx:
            want[max(i - c.r[0], 0):i + c.r[0] + 1, max(j - c.r[1], 0):j + c.r[1] + 1, max(k - c.r[2], 0):k + c.r[2] + 1] = True
        assert np.array_equal(ref, want), c.name
    one = next(c for c in cases if "second word" in c.name and c.vox.shape[2] == 70)
    ref = gc.dilate_reference((one.vox & 4) != 0, one.r)
    assert ref[2, 1, 1] and ref[2, 1, 63] and not ref[2, 1, 0] and not ref[2, 1, 64]  # carries into both neighbouring words
    shape, r = gc.INFLATE_REFUSED
    assert r[2] == 32
