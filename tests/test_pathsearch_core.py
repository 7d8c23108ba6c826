"""-m "not gpu": findCollisionSeg and pathSearch as the kernels run them (csrc/vigo_pathsearch_core.hpp around the device's
search core, compiled for the host: vigo_host_path_search_core).
  With unbounded capacities the twin equals the facade's own host pipeline (vigo_host_prologue_paths) on statuses,
  seg_off, seg, path_off and path (bits as uint64) on the two pipeline batches and on the crafted cases;
  its segments equal the Python restatement of tests/test_prologue_restatement.py on that file's random worlds;
  with the shipped capacities (vigo_astar_capacity) the deferred trajectories are exactly the owners of consulted searches
  that are over capacity, and at most 2 % of each pipeline batch — a condition, not a measurement."""
import ctypes as C

import numpy as np
import pytest

import astar_cases as ac
import pathsearch_cases as pc
from test_prologue_restatement import DenseMap, _world, collision_segments, reference_prologue
from trajectory_planner_amd import synth


@pytest.fixture(scope="module")
def lib():
    return pc.host_lib()


@pytest.fixture(scope="module")
def pipeline():
    return [pc.pipeline_workload(), pc.pipeline_workload(synth.SEED_BASE + 77)]


def test_unbounded_twin_is_the_facades_pipeline_bit_for_bit(lib, pipeline):
    for w in pipeline:
        t, f = pc.twin(lib, w), pc.facade(lib, w)
        assert t.rc == 0 and pc.same(t, f), w.name
        assert len(t.seg) >= 400 and (t.status == pc.OK).all()
        assert (t.counts[:, 0] == t.counts[:, 1]).all()           # nothing is left undecided without a capacity
        rc, seg_off, seg, st = pc.twin_segments(lib, w)
        assert rc == 0 and (st == pc.OK).all() and int(seg_off[-1]) >= len(t.seg)
        print(f"\n{w.name}: {w.B} trajectories, {len(t.seg)} segments, {len(t.path)} path points: twin == facade")


def test_crafted_cases(lib):
    seen = {}
    for name, w in pc.crafted_workloads():
        t = pc.twin(lib, w)
        assert t.rc == 0, name
        st, seg, paths = t.of(0)
        seen[name] = (st, [tuple(s) for s in seg], t.counts[0].tolist())
        print(f"{name}: status {st}, segments {seen[name][1]}, searches run / decided {seen[name][2]}")
        for s, p in zip(seg, paths):                              # a path leaves from a control point and ends on one
            assert len(p) >= 2 and any(np.array_equal(p[0], c) for c in w.ctrl[0]) and any(np.array_equal(p[-1], c) for c in w.ctrl[0])
        if w.seg_off is None:
            assert pc.same(t, pc.facade(lib, w)), name            # the facade's own steps, bit for bit
            rc, _, scanned, _ = pc.twin_segments(lib, w)
            m = DenseMap(w.vox, w.origin, w.res)
            c = w.ctrl[0]
            assert rc == 0 and [tuple(s) for s in scanned] == collision_segments(w.N, lambda i: m.occ(c[i]), lambda i: m.occ_line(c[i - 1], c[i])), name
            seen[name] += ([tuple(s) for s in scanned],)
    st = lambda k: seen[k][0]
    assert seen["no segments"][:2] == (pc.OK, []) and seen["no segments"][2] == [0, 0]
    assert st("one block, one search") == pc.OK and len(seen["one block, one search"][1]) == 1
    k = "a failed last segment"
    assert st(k) == pc.FAILED and len(seen[k][3]) == 1 and seen[k][2] == [1, 1]
    k = "a merge taken"
    a, b = seen[k][3]
    assert st(k) == pc.OK and seen[k][1] == [(a[0], b[1])] and seen[k][2] == [3, 3] and b[0] - a[1] <= 2
    k = "a merge taken while another segment stays unmerged"
    s0, a, b = seen[k][3]
    assert st(k) == pc.OK and seen[k][1] == [(a[0], b[1])] and seen[k][2] == [4, 4]      # (s0 is dropped; its path stays path 0)
    wk = dict(pc.crafted_workloads())[k]
    p0 = pc.twin(lib, wk).of(0)[2][0]
    assert np.array_equal(p0[0], wk.ctrl[0][s0[0]]) and np.array_equal(p0[-1], wk.ctrl[0][s0[1]])
    k = "a failed first choice with gap > 2"
    a, b = seen[k][3]
    assert st(k) == pc.FAILED and b[0] - a[1] > 2 and seen[k][2] == [2, 2]
    k = "a second choice that fails too"
    assert st(k) == pc.FAILED and seen[k][2][0] >= 3 and seen[k][3][1][0] - seen[k][3][0][1] <= 2
    k = "the endIdx - 1 duplicate segment"
    a, b = seen[k][3]
    assert st(k) == pc.OK and a[0] == b[0] and a[1] == pc.CRAFTED_N - 1 and b[1] == pc.CRAFTED_N - 4 and seen[k][1] == [a, b]
    k = "a line-only segment"
    assert st(k) == pc.OK and seen[k][1] == [(11, 12)]
    k = "a supplied list that differs from the scanned one"
    assert st(k) == pc.OK and seen[k][1] == [(13, 19), (20, 22)] and seen[k][2] == [2, 2]
    k = "a supplied list of more than VIGO_MAX_COLLISION_SEGS segments"
    assert seen[k] == (pc.DEFERRED, [], [0, 0])
    # the supplied list's paths are the host A*'s own between those control points
    w = dict(pc.crafted_workloads())["a supplied list that differs from the scanned one"]
    alib = ac.host_lib()
    _, _, paths = pc.twin(lib, w).of(0)
    for (f, s), p in zip(w.seg, paths):
        host, _ = ac.host_astar(alib, ac.Case("", w.vox, w.origin, w.res, w.pool, w.cfg[1], w.cfg[2], w.res, w.ctrl[0][f], w.ctrl[0][s]))
        assert np.array_equal(p[1:-1], host[1:]) and np.array_equal(p[0], w.ctrl[0][f]) and np.array_equal(p[-1], w.ctrl[0][s])


def test_more_scanned_segments_than_the_state_holds_are_deferred(lib):
    w = pc.zigzag_workload()
    rc, seg_off, seg, st = pc.twin_segments(lib, w)
    assert rc == 0 and st.tolist() == [pc.DEFERRED] and seg_off.tolist() == [0, 0]
    t = pc.twin(lib, w)
    assert t.rc == 0 and t.status.tolist() == [pc.DEFERRED] and len(t.seg) == 0 and t.counts[0].tolist() == [0, 0]
    m = DenseMap(w.vox, w.origin, w.res)
    c = w.ctrl[0]
    assert len(collision_segments(w.N, lambda i: m.occ(c[i]), lambda i: m.occ_line(c[i - 1], c[i]))) > pc.MAX_SEGS
    w60 = pc.zigzag_workload(N=60)                                 # fewer points: the same shape fits
    rc, seg_off, seg, st = pc.twin_segments(lib, w60)
    assert rc == 0 and st.tolist() == [pc.OK] and 20 < seg_off[1] <= pc.MAX_SEGS


def test_not_check_ratio(lib):
    for ncr in (0.0, 0.3, 0.77, 1.0):
        for name, w in pc.crafted_workloads():
            if w.seg_off is not None:
                continue
            w.ncr = ncr
            rc, _, scanned, st = pc.twin_segments(lib, w)
            m = DenseMap(w.vox, w.origin, w.res)
            c = w.ctrl[0]
            want = collision_segments(w.N, lambda i: m.occ(c[i]), lambda i: m.occ_line(c[i - 1], c[i]), ncr)
            assert rc == 0 and [tuple(s) for s in scanned] == want, (name, ncr)
            t = pc.twin(lib, w)
            if t.status[0] == pc.OK and t.counts[0, 0] == len(want):          # (no merge: the segments are the scanned ones)
                assert [tuple(s) for s in t.seg] == want, (name, ncr)
    w = dict(pc.crafted_workloads())["the endIdx - 1 duplicate segment"]
    w.ncr = 0.3
    assert len(pc.twin_segments(lib, w)[2]) == 0                   # (the scan now ends before the block)
    for bad in (-0.1, 1.5, float("nan")):
        w.ncr = bad
        assert pc.twin_segments(lib, w)[0] == -1 and pc.twin(lib, w).rc == -1


@pytest.mark.parametrize("seed", range(2))
def test_segments_equal_the_python_restatement(lib, seed):
    """the random worlds of tests/test_prologue_restatement.py: findCollisionSeg and the pathSearch part of reference_prologue"""
    rng = np.random.default_rng(500 + seed)
    compared = 0
    for case in range(5):
        vox, origin = _world(rng)
        y0, y1 = rng.uniform(-2.5, 2.5, size=2)
        pts = np.stack([np.linspace(-4.0, 4.0, 33), np.linspace(y0, y1, 33), np.full(33, 1.0)], axis=1)
        c = np.ascontiguousarray(synth.fit_control_points(pts[None])[0])
        cfg = np.array([0.5, 0.7, 1.3, 4.0, 4.0, 4.0])
        w = pc.Workload(f"random {seed}/{case}", vox, origin, 0.1, np.ascontiguousarray(c[None]), cfg)
        m = DenseMap(vox, origin, 0.1)
        rc, _, scanned, _ = pc.twin_segments(lib, w)
        assert rc == 0 and [tuple(s) for s in scanned] == collision_segments(len(c), lambda i: m.occ(c[i]), lambda i: m.occ_line(c[i - 1], c[i]))
        ref = reference_prologue(vox, origin, 0.1, c, cfg)
        t = pc.twin(lib, w)
        assert t.rc == 0
        if ref is None:
            assert t.status[0] == pc.FAILED and len(t.seg) == 0, (seed, case)
            continue
        segs, paths, _ = ref
        st, seg, tp = t.of(0)
        assert st == pc.OK and [tuple(s) for s in seg] == segs[:len(paths)], (seed, case)
        for p, q in zip(tp, paths):
            assert np.array_equal(p, np.array(q)), (seed, case)
        compared += len(segs) > 0
    assert compared >= 1


def _consulted_over_capacity(lib, w, t_unbounded, cap):
    """owners of a consulted search that the kernels' table or heap cannot hold: the predicate of
    tests/test_gpu_astar.py::_over_capacity (host search pushes more nodes than max_nodes, or its open set outgrows
    the heap), on the searches the unbounded walk consulted — every path's search (found) and, for a failed trajectory,
    none (every consulted search of these batches is found: the trajectories are plannable)"""
    alib = ac.host_lib()
    owners = np.zeros(w.B, dtype=bool)
    for b in range(w.B):
        _, seg, paths = t_unbounded.of(b)
        for p in paths:
            _, hs = ac.host_astar(alib, ac.Case("", w.vox, w.origin, w.res, w.pool, w.cfg[1], w.cfg[2], w.res, p[0], p[-1]))
            if hs[4] > cap["max_nodes"] or hs[2] > cap["heap_cap"]:
                owners[b] = True
    return owners


def test_shipped_capacities_defer_the_owners_of_over_capacity_searches_and_at_most_2_percent(lib, pipeline):
    cap = pc.shipped()
    for w in pipeline:
        full, t = pc.twin(lib, w), pc.twin(lib, w, cap=cap)
        assert t.rc == 0
        deferred = t.status == pc.DEFERRED
        share = deferred.mean()
        print(f"\n{w.name}: {int(deferred.sum())} of {w.B} trajectories deferred under the shipped capacities ({share * 100:.2f} %)")
        # no merges in these batches: every consulted search is a first choice, found, and is a path of the unbounded walk
        assert (full.counts[:, 0] == np.diff(full.seg_off)).all()
        assert np.array_equal(deferred, _consulted_over_capacity(lib, w, full, cap)), w.name
        assert share <= 0.02, w.name
        for b in np.nonzero(~deferred)[0]:                         # what is not deferred is the unbounded result
            a, c = t.of(b), full.of(b)
            assert a[0] == c[0] and np.array_equal(a[1], c[1]) and all(np.array_equal(pc.bits(x), pc.bits(y)) for x, y in zip(a[2], c[2])), b
        assert (np.diff(t.seg_off)[deferred] == 0).all() and (t.counts[deferred, 1] < t.counts[deferred, 0]).all()
