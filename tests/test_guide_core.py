"""-m "not gpu": the guide assignment the kernel runs (csrc/vigo_guide_core.hpp), compiled for the host.
  mode 0 (std::atan2) == the facade's assignGuidePointsSemiCircle, bit for bit: the core is the reference's step;
  vigo_atan2 within 2 ulp of libm's atan2 (the routine's design bound), exact on the sign and zero cases;
  mode 1 (vigo_atan2, the device's twin) against mode 0: the same offsets, decisions that differ on at most 0.5 % of the
  pairs, and on the agreeing pairs a deviation within 4 x the deviation of a libm nudged by +-2 ulp (modes 2 / 3);
  deferral beyond the kernel's path buffer, and that buffer against the pipeline workload."""
import math

import numpy as np
import pytest

import guide_cases as gc
from trajectory_planner_amd import synth


@pytest.fixture(scope="module")
def lib():
    return gc.host_lib()


@pytest.fixture(scope="module")
def workloads(lib):
    w1, world, status = gc.pipeline_workload(lib)
    w2, _, _ = gc.pipeline_workload(lib, synth.SEED_BASE + 77)
    w3, names = gc.crafted_workload()
    return dict(first=(w1, world), second=(w2, world), crafted=(w3, names))


def test_mode_0_is_the_facades_step_bit_for_bit(lib, workloads):
    for key in ("first", "second", "crafted"):
        w = workloads[key][0]
        rc, off, pv, _, st, _ = gc.core(lib, w, 0)
        assert rc == 0 and (st == gc.OK).all()
        f_off, f_pv = gc.facade(lib, w)
        assert np.array_equal(off, f_off), w.name
        assert pv.shape == f_pv.shape and np.array_equal(gc.bits(pv), gc.bits(f_pv)), w.name
        print(f"\n{w.name}: {w.B} trajectories, {len(w.seg)} segments, {len(pv)} pairs: mode 0 == the facade's step")
    w, world = workloads["first"]
    assert len(w.seg) >= 400                     # about 800 segments are expected
    # ... and the facade's step on these inputs is what its own pipeline appends (synth.host_guides on the control points)
    _, status, n_seg, goff, gpv = synth.host_guides(world, w.N, ctrl=w.ctrl)
    rc, off, pv, _, _, _ = gc.core(lib, w, 0)
    assert np.array_equal(off, goff) and np.array_equal(gc.bits(pv), gc.bits(gpv))


def test_crafted_cases_hit_what_they_are_for(lib, workloads):
    w, names = workloads["crafted"]
    rc, off, pv, unk, st, dec = gc.core(lib, w, 0)
    N = w.N
    cnt = lambda b: np.diff(off[b * N:(b + 1) * N + 1])
    b = names.index("line collisions at the clip bounds")
    c = cnt(b)
    # (3,4) -> 3,4,5; (N-5,N-4) -> N-6..N-4 clipped; (2,3) -> 3,4; (N-4,N-3) -> N-5,N-4: nothing on 2 or N-3
    assert c[2] == 0 and c[N - 3] == 0 and c[3] == 2 and c[4] == 2 and c[5] == 1 and c[N - 4] == 2 and c[N - 5] == 2 and c[N - 6] == 1
    b = names.index("segment ending at N - 1")
    assert cnt(b)[N - 6:N - 1].tolist() == [1] * 5 and cnt(b)[N - 1] == 0
    b = names.index("failed searches: the very first, a zero diff, a stale guide point")
    s = w.pairs_of(off, b)
    found = dec[s][:, 0]
    # (pairs are listed per control point: 5, 6 | 10, 11, 12 | 15, 16 | 19 .. 22)
    assert found[0] == 0 and not pv[s][:2, :3].any()                             # the very first search fails: the zero guide point
    assert np.isnan(pv[s][0, 3:]).all() and not np.isnan(pv[s][1:]).any()        # control point 5 sits on it: 0 / 0
    assert found[2:5].all() and (found[5:] == 0).all()
    assert np.array_equal(gc.bits(pv[s][5:, :3]), np.tile(gc.bits(pv[s][4, :3]), (len(found) - 5, 1)))   # the stale point is carried
    assert unk.max() <= 1


def test_vigo_atan2_is_within_2_ulp_of_libm(lib):
    import ctypes as C
    rng = np.random.default_rng(20261017)
    n = 1 << 20
    mag = lambda: 10.0 ** rng.uniform(-300, 300, n) * rng.choice([-1.0, 1.0], n)
    y, x = mag(), mag()
    # half of them with comparable magnitudes (otherwise nearly every quotient under- or overflows to an axis)
    x[: n // 2] = y[: n // 2] * rng.choice([-1.0, 1.0], n // 2) * np.exp(rng.uniform(-12, 12, n // 2))
    exact = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, -1.5), (-0.0, -1.5), (0.0, 2.0), (3.0, 0.0), (-3.0, 0.0), (3.0, -0.0),
             (1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0), (math.inf, 1.0), (1.0, math.inf), (1.0, -math.inf), (math.inf, math.inf),
             (-math.inf, -math.inf), (1e-300, 1e300), (1e300, 1e-300), (5e-324, 1.0), (0.046875, 1.0), (1.0, 0.046875)]
    y = np.concatenate([y, [e[0] for e in exact]])
    x = np.concatenate([x, [e[1] for e in exact]])
    out = np.zeros_like(y)
    dp = C.POINTER(C.c_double)
    assert lib.vigo_host_atan2(len(y), y.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    ref = np.arctan2(y, x)
    assert all(math.atan2(a, b) == r for a, b, r in zip(y[-len(exact):], x[-len(exact):], ref[-len(exact):]))   # numpy's is libm's
    ulp = np.spacing(np.abs(ref))
    err = np.abs(out - ref) / ulp
    print(f"\nvigo_atan2 against libm atan2 on {len(y)} inputs: largest difference {err.max():.3f} ulp, {(err > 1).mean() * 100:.4f} % above 1 ulp")
    assert err.max() <= 2.0
    assert np.array_equal(np.signbit(out), np.signbit(ref))
    for k in range(10):                                  # the zero, pi and pi/2 cases: exactly
        i = len(y) - len(exact) + k
        assert gc.bits(out[i:i + 1])[0] == gc.bits(ref[i:i + 1])[0], exact[k]
    nan = np.array([np.nan, 1.0]), np.array([1.0, np.nan])
    o2 = np.zeros(2)
    lib.vigo_host_atan2(2, nan[0].ctypes.data_as(dp), nan[1].ctypes.data_as(dp), o2.ctypes.data_as(dp))
    assert np.isnan(o2).all()


def _compare(lib, w, mode, base):
    """mode against mode 0 -> (pairs, pairs whose decision differs, the largest deviation on the agreeing pairs)"""
    rc, off, pv, _, _, dec = gc.core(lib, w, mode)
    assert rc == 0 and np.array_equal(off, base[0])
    differ = (dec != base[2]).any(axis=1)
    both = ~differ
    d = np.abs(pv[both] - base[1][both])
    d = d[np.isfinite(d)]                                # (a NaN direction is a NaN in every mode)
    assert np.array_equal(np.isnan(pv), np.isnan(base[1]))
    return len(pv), int(differ.sum()), float(d.max()) if d.size else 0.0


def test_mode_1_against_mode_0(lib, workloads):
    pairs = diff1 = diffn = 0
    dev1 = devn = 0.0
    for key in ("first", "second", "crafted"):
        w = workloads[key][0]
        rc, off, pv, _, _, dec = gc.core(lib, w, 0)
        base = (off, pv, dec)
        n, d2, e2 = _compare(lib, w, 2, base)
        _, d3, e3 = _compare(lib, w, 3, base)
        _, d1, e1 = _compare(lib, w, 1, base)            # (offsets identical: asserted inside)
        print(f"\n{w.name}: {n} pairs; decisions that differ from mode 0: +2 ulp {d2}, -2 ulp {d3}, vigo_atan2 {d1}; largest deviation on "
              f"agreeing pairs: +2 ulp {e2:.3e}, -2 ulp {e3:.3e}, vigo_atan2 {e1:.3e}")
        pairs += n
        diffn = max(diffn, 0) + max(d2, d3)
        diff1 += d1
        devn, dev1 = max(devn, e2, e3), max(dev1, e1)
    print(f"\nall workloads: {pairs} pairs; decisions differ: neighbours {diffn} ({diffn / pairs * 100:.3f} %), vigo_atan2 {diff1} "
          f"({diff1 / pairs * 100:.3f} %); deviation: neighbours' floor {devn:.3e}, vigo_atan2 {dev1:.3e} ({dev1 / devn if devn else 0:.2f} x)")
    assert diffn <= 0.0025 * pairs        # precondition: the workloads are not at libm's mercy
    assert diff1 <= 0.005 * pairs
    assert dev1 <= 4 * devn


def test_deferral_and_the_shipped_capacity(lib, workloads):
    cap = gc.capacity()
    w, names = gc.crafted_workload(long_path=cap + 1)
    rc, off, pv, unk, st, dec = gc.core(lib, w, 1, path_cap=cap)
    assert rc == 0
    b = names.index("a path longer than the device buffer")
    assert st[b] == gc.DEFERRED and (np.delete(st, b) == gc.OK).all()
    assert off[b * w.N] == off[(b + 1) * w.N]                                   # it owns no pairs
    rc, off0, pv0, _, st0, _ = gc.core(lib, w, 1)                              # nothing deferred: the others are unchanged
    assert (st0 == gc.OK).all()
    for k in range(w.B):
        if k != b:
            assert np.array_equal(gc.bits(pv[w.pairs_of(off, k)]), gc.bits(pv0[w.pairs_of(off0, k)])), names[k]
            assert np.array_equal(np.diff(off[k * w.N:(k + 1) * w.N + 1]), np.diff(off0[k * w.N:(k + 1) * w.N + 1]))
    # exactly the capacity is taken
    w2, _ = gc.crafted_workload(long_path=cap)
    assert (gc.core(lib, w2, 1, path_cap=cap)[4] == gc.OK).all()
    # too little room: refused, nothing written
    total = int(off0[-1])
    rc, o, p, u, s, d = gc.core(lib, w, 1, pair_cap=total - 1)
    assert rc == -1 and (o == -7).all() and (p == -7.0).all() and (u == 7).all() and (s == -7).all()
    assert gc.core(lib, w, 1, pair_cap=total)[0] == 0
    # condition of the GPU parity test (it must not pass by deferring): at most 2 % of the pipeline trajectories have a
    # path longer than the shipped buffer
    wp = workloads["first"][0]
    longest = np.array([max([0] + [wp.path_off[k + 1] - wp.path_off[k] for k in range(wp.seg_off[t], wp.seg_off[t + 1])]) for t in range(wp.B)])
    over = longest > cap
    print(f"\npath points per segment on the pipeline batch: median {int(np.median(np.diff(wp.path_off)))}, largest {int(longest.max())}; "
          f"capacity {cap}; trajectories over it: {over.mean() * 100:.2f} %")
    assert over.mean() <= 0.02
