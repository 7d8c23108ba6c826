"""-m "not gpu": the re-guide step of the rebound loop on the host.  csrc/vigo_reguide_core.hpp around the path-search
and guide twins (vigo_host_rebound_reguide_core) with libm's atan2 and unbounded capacities equals the facade's own
bsplineTraj::reboundStep (vigo_host_reguide_facade) bit for bit on the crafted cases and the derived batch of
tests/reguide_cases.py: segments, merged pairs, weights, failCount, needOptimize, paths.  The header's rules equal a
Python restatement of isReguideRequired on seeded random flags, segments and guide tests.  With vigo_atan2 (the
kernels' arithmetic) every discrete outcome stays and the pairs move by no more than libm's own neighbours move them."""
import numpy as np
import pytest

import reguide_cases as rc

N_DERIVED = 128


@pytest.fixture(scope="module")
def lib():
    return rc.host_lib()


@pytest.fixture(scope="module")
def derived():
    return rc.derived_batch(N_DERIVED)


@pytest.fixture(scope="module")
def derived_truth(lib, derived):
    return rc.facade(lib, derived)


def _equal_facade(c, t, f, label):
    """twin result t (unbounded, libm) against the facade's f on every trajectory the twin did not defer or skip"""
    N = c.N
    for b in range(c.B):
        s = int(t.status[b])
        tag = f"{label} [{b}]"
        if s in (rc.DEFERRED, rc.SKIPPED):
            assert np.array_equal(t.state[b], c.state[b]) and np.array_equal(rc.bits(t.weights[b]), rc.bits(c.weights[b])), tag
            assert all(np.array_equal(rc.bits(x), rc.bits(c.gpv[c.goff[b * N + i]:c.goff[b * N + i + 1]])) for i, x in enumerate(t.pairs_of(b, N))), tag
            continue
        n = int(f.state[b, rc.S_NSEG])
        assert n <= rc.MAX_SEGS and int(t.state[b, rc.S_NSEG]) == n, tag
        assert np.array_equal(t.state[b, rc.S_SEG:rc.S_SEG + 2 * n], f.state[b, rc.S_SEG:rc.S_SEG + 2 * n]), tag
        assert int(t.state[b, rc.S_FAIL]) == int(f.state[b, rc.S_FAIL]), tag
        assert np.array_equal(rc.bits(t.weights[b]), rc.bits(f.weights[b])), tag
        assert int(t.state[b, rc.S_STATUS]) == rc.RB_ACTIVE and int(t.state[b, rc.S_SOLVE_FIRST]) == int(f.status[b]) == 1, tag
        # what the entry leaves alone
        for col in (rc.S_GATE_STATIC, rc.S_GATE_DYNAMIC, rc.S_ROUNDS, rc.S_LBFGS):
            assert t.state[b, col] == c.state[b, col], tag
        assert np.array_equal(t.state[b, rc.S_SEG + 2 * n:], c.state[b, rc.S_SEG + 2 * n:]), tag
        assert int(t.state[b, rc.S_FAIL]) == int(c.state[b, rc.S_FAIL]) + (0 if s == rc.DONE else 1), tag
        tp, fp = t.pairs_of(b, N), f.pairs_of(b, N)
        assert all(x.shape == y.shape and np.array_equal(rc.bits(x), rc.bits(y)) for x, y in zip(tp, fp)), tag
        grown = sum(len(x) for x in tp) - int(c.goff[(b + 1) * N] - c.goff[b * N])
        assert (grown > 0) == (s == rc.DONE) or (s == rc.DONE and grown == 0), tag
        if s == rc.DONE:
            a, e = t.paths_of(b), f.paths_of(b)
            assert len(a) == len(e) >= 1 and all(x.shape == y.shape and np.array_equal(rc.bits(x), rc.bits(y)) for x, y in zip(a, e)), tag
        else:
            assert len(t.paths_of(b)) == 0 and len(f.paths_of(b)) == 0, tag


def test_crafted_cases_equal_the_facade_step(lib):
    seen = set()
    for c in rc.crafted_cases():
        t = rc.twin(lib, c, 0, rc.UNBOUNDED)
        assert t.rc == 0, c.name
        if c.expect is not None:
            assert int(t.status[0]) == c.expect, (c.name, t.status)
        seen.add(int(t.status[0]))
        _equal_facade(c, t, rc.facade(lib, c), c.name)
        # the shipped capacities decide the same on these small worlds
        assert np.array_equal(rc.twin(lib, c, 0, rc.shipped()).status, t.status), c.name
    assert seen == {rc.DONE, rc.SEARCH_FAILED, rc.NOT_REQUIRED, rc.DEFERRED, rc.SKIPPED}


def test_crafted_details(lib):
    cases = {c.name: c for c in rc.crafted_cases()}
    t = rc.twin(lib, cases["a control point that already carries 5 pairs"], 0, rc.UNBOUNDED)
    assert len(t.pairs_of(0, 32)[15]) == 6 and np.array_equal(rc.bits(t.pairs_of(0, 32)[15][:5]), rc.bits(cases["a control point that already carries 5 pairs"].gpv[1:6]))
    t = rc.twin(lib, cases["the endIdx - 1 duplicate"], 0, rc.UNBOUNDED)
    n = int(t.state[0, rc.S_NSEG])
    seg = t.state[0, rc.S_SEG:rc.S_SEG + 2 * n].reshape(-1, 2)
    assert n >= 2 and any(seg[k][0] == seg[k + 1][0] for k in range(n - 1)), seg           # collisionSeg_ keeps the second push of the segment
    t = rc.twin(lib, cases["gate_dynamic set, re-guided"], 0, rc.UNBOUNDED)
    assert list(t.weights[0]) == [1.0, 1.0, 1.0, 16.0]
    t = rc.twin(lib, cases["gate_dynamic set, search failed"], 0, rc.UNBOUNDED)
    assert list(t.weights[0]) == [2.0, 1.0, 1.0, 2.0] and int(t.state[0, rc.S_FAIL]) == 4
    t = rc.twin(lib, cases["a merge taken inside the re-guide list"], 0, rc.UNBOUNDED)
    assert int(t.status[0]) == rc.DONE and int(t.state[0, rc.S_NSEG]) == 2 and len(t.paths_of(0)) == 1
    # the guide step's own deferral: the path search succeeds, the path is longer than the kernel's buffer
    c = rc.long_path_case()
    t = rc.twin(lib, c, 1, rc.shipped())
    assert int(t.status[0]) == rc.DEFERRED and np.array_equal(t.state, c.state) and len(t.paths_of(0)) == 1
    assert len(t.paths_of(0)[0]) > rc.shipped()["guide_path_cap"]
    assert int(rc.twin(lib, c, 1, dict(rc.shipped(), guide_path_cap=1 << 30)).status[0]) == rc.DONE


def test_derived_batch_equals_the_facade_step_and_covers_the_outcomes(lib, derived, derived_truth):
    c, f = derived, derived_truth
    # the conditions on the workload, on the facade reference alone
    N = c.N
    grown = np.array([int(f.off[(b + 1) * N] - f.off[b * N]) - int(c.goff[(b + 1) * N] - c.goff[b * N]) for b in range(c.B)])
    failed_more = f.state[:, rc.S_FAIL] > c.state[:, rc.S_FAIL]
    reguided = grown > 0
    assert not (reguided & failed_more).any()
    t = rc.twin(lib, c, 0, rc.UNBOUNDED)
    assert t.rc == 0
    _equal_facade(c, t, f, c.name)
    assert (t.status != rc.SKIPPED).all() and (t.status == rc.DEFERRED).sum() == 0
    assert np.array_equal(t.status == rc.DONE, reguided | ((t.status == rc.DONE) & ~failed_more))
    n_failed = int((t.status == rc.SEARCH_FAILED).sum())
    n_crafted_failed = sum(1 for k in rc.crafted_cases() if k.expect == rc.SEARCH_FAILED)
    print(f"\n{c.name}: re-guided {int(reguided.sum())}, not required {int((t.status == rc.NOT_REQUIRED).sum())}, search failed {n_failed} "
          f"(+ {n_crafted_failed} crafted)")
    assert reguided.sum() >= 8 and (t.status == rc.NOT_REQUIRED).sum() >= 8 and n_failed + n_crafted_failed >= 8
    # under the shipped capacities at most 10 % of the trajectories that require a re-guide are deferred
    s = rc.twin(lib, c, 0, rc.shipped())
    required = t.status != rc.NOT_REQUIRED
    deferred = s.status == rc.DEFERRED
    print(f"shipped capacities: {int(deferred.sum())} of {int(required.sum())} required re-guides deferred")
    assert not (deferred & ~required).any() and deferred.sum() <= 0.10 * required.sum()
    assert np.array_equal(s.status[~deferred], t.status[~deferred])


def _restated_is_reguide_required(N, ncr, pt, ln, prev, need):
    """isReguideRequired (BT.cpp:573-608) with findCollisionSeg, compareCollisionSeg and findCollisionSegIndex, restated"""
    seg, prev_has, start = [], False, 3
    v = (N - 3 - 1) - ncr * (N - 2 * 3)
    end_idx = int(v)
    for i in range(3, end_idx + 1):
        has = bool(pt[i])
        if has != prev_has:
            if has:
                start = i - 1
            else:
                seg.append((start, i))
        if has and i == end_idx - 1:
            seg.append((start, N - 1))
        if i != 3 and not prev_has and not has and ln[i]:
            seg.append((i - 1, i))
        prev_has = has
    inside = lambda segs, i: any(f <= i <= s for f, s in segs)
    fresh, over = [], []
    for f, s in seg:
        pts = list(range(f + 1, s)) + (list(range(f, s + 1)) if s - f - 1 == 0 else [])
        for i in pts:
            (over if inside(prev, i) else fresh).append(i)
    index = lambda i: next((k for k, (f, s) in enumerate(seg) if f <= i <= s), -1)
    idx = {index(i) for i in fresh} | {index(i) for i in over if need[i]}
    idx.discard(-1)
    return seg, sorted(idx)


def test_rules_equal_the_restatement_on_random_inputs(lib):
    rng = np.random.default_rng(0xC0FFEE)
    yes = 0
    for trial in range(1500):
        N = int(rng.integers(7, 61))
        ncr = float(rng.choice([0.0, 0.0, 0.2, 0.5, 1.0]))
        p = rng.choice([0.1, 0.3, 0.6])
        pt = (rng.random(N) < p).astype(np.uint8)
        if trial % 3 == 0:                                # runs of occupied points: longer segments
            pt = np.repeat((rng.random(N // 3 + 1) < p), 3)[:N].astype(np.uint8)
        ln = (rng.random(N) < 0.3).astype(np.uint8)
        prev = []
        for _ in range(int(rng.integers(0, 5))):
            f = int(rng.integers(0, N - 1))
            prev.append((f, int(rng.integers(f + 1, min(N, f + 8)))))
        need = (rng.random(N) < rng.choice([0.0, 0.2, 1.0])).astype(np.uint8)
        seg, idx = _restated_is_reguide_required(N, ncr, pt, ln, prev, need)
        n, got_seg, listed = rc.rules(lib, N, ncr, pt, ln, prev, need)
        assert n == len(seg) and [tuple(s) for s in got_seg] == seg, trial
        assert list(np.nonzero(listed)[0]) == idx, (trial, seg, prev)
        # the yes/no of k_rebound_decide: any compared control point that is fresh or needs a new guide
        asks = any((not any(f <= i <= s for f, s in prev)) or need[i]
                   for f, s in seg for i in (list(range(f + 1, s)) + (list(range(f, s + 1)) if s - f == 1 else [])))
        assert asks == (len(idx) > 0), trial
        yes += asks
    assert 300 < yes < 1400
    # more segments than the caller's room: the count alone
    pt = np.zeros(120, dtype=np.uint8)
    pt[4::2] = 1
    n, _, listed = rc.rules(lib, 120, 0.0, pt, np.zeros(120, dtype=np.uint8), [], np.ones(120, dtype=np.uint8))
    assert n > rc.MAX_SEGS and listed is None


def _pair_floor(lib, c, base):
    """how far libm's own neighbours (atan2 nudged by +-2 ulp, the method of tests/test_guide_core.py) move the pairs of the
    re-guided trajectories: the largest absolute difference"""
    worst = 0.0
    for mode in (2, 3):
        t = rc.twin(lib, c, mode, rc.UNBOUNDED)
        assert np.array_equal(t.status, base.status) and np.array_equal(t.off, base.off)
        worst = max(worst, float(np.nanmax(np.abs(t.pv - base.pv))) if len(base.pv) else 0.0)
    return worst


def test_device_arithmetic_keeps_every_outcome(lib, derived):
    for c in rc.crafted_cases() + [derived]:
        a, d = rc.twin(lib, c, 0, rc.UNBOUNDED), rc.twin(lib, c, 1, rc.UNBOUNDED)
        assert np.array_equal(a.status, d.status) and np.array_equal(a.state, d.state) and np.array_equal(rc.bits(a.weights), rc.bits(d.weights)), c.name
        assert np.array_equal(a.off, d.off) and np.array_equal(a.path_off, d.path_off) and np.array_equal(rc.bits(a.path), rc.bits(d.path)), c.name
        assert np.array_equal(np.isnan(a.pv), np.isnan(d.pv)), c.name
        if len(a.pv):
            floor = _pair_floor(lib, c, a)
            diff = float(np.nanmax(np.abs(a.pv - d.pv))) if np.isfinite(a.pv).any() else 0.0
            assert diff <= max(floor, 1e-15), (c.name, diff, floor)


def test_error_contract_of_the_twin(lib):
    c = rc.crafted_cases()[1]
    good = rc.twin(lib, c, 1, rc.shipped())
    assert good.rc == 0
    g = int(good.off[-1])

    def untouched(r, fill=-7):
        return ((r.raw["off"] == fill).all() and (r.raw["pv"] == float(fill)).all() and (r.raw["status"] == fill).all() and
                (r.raw["path_seg_off"] == fill).all() and (r.raw["path"] == float(fill)).all() and np.array_equal(r.raw["state"], c.state) and
                np.array_equal(r.raw["weights"], c.weights))

    assert untouched(rc.twin(lib, c, 1, rc.shipped(), pair_cap=g - 1))
    assert rc.twin(lib, c, 1, rc.shipped(), pair_cap=g - 1).rc == -1 and rc.twin(lib, c, 1, rc.shipped(), pair_cap=g).rc == 0
    assert untouched(rc.twin(lib, c, 1, rc.shipped(), seg_cap=0)) and untouched(rc.twin(lib, c, 1, rc.shipped(), point_cap=3))
    assert rc.twin(lib, c, 1, rc.shipped(), seg_cap=0, want_paths=False).rc == 0
    bad = rc.Case(c.name, c.vox, c.origin, c.res, c.cfg, c.ctrl, c.goff.copy(), c.gpv, c.weights, c.state)
    bad.goff[16] = bad.goff[15] - 1
    assert untouched(rc.twin(lib, bad, 1, rc.shipped())) and rc.twin(lib, bad, 1, rc.shipped()).rc == -1
    bad.ncr = 1.5
    bad.goff = c.goff
    assert untouched(rc.twin(lib, bad, 1, rc.shipped()))
    # nothing beyond the totals
    r = good
    assert (r.raw["pv"][g:] == -7.0).all() and (r.raw["unk"][g:] == (-7 & 0xFF)).all()
    S = int(r.path_seg_off[1])
    assert (r.raw["path_off"][S + 1:] == -7).all() and (r.raw["path"][r.path_off[S]:] == -7.0).all()
