"""-m gpu: the prologue and re-guide entries for mixed control-point counts — vigo_collision_segs_mixed,
vigo_path_search_mixed, vigo_guide_assign_mixed, vigo_rebound_reguide_mixed (include/vigo.h, "prologue and re-guide for
mixed control-point counts") — on the batches of tests/prologue_mixed_cases.py.  The invariant: every output of a
trajectory in a mixed call equals, bit for bit, its output in the UNIFORM call of its own count.  The reference of every
comparison is the uniform entry called per count on the same rows, never the mixed entry.  Output buffers are pre-filled
with a sentinel: nothing is written beyond a call's totals, nothing at all on a call-level error."""
import numpy as np
import pytest
import torch

import pathsearch_cases as pc
import prologue_mixed_cases as pm
import reguide_cases as rc
from gpu_util import to_dev
from trajectory_planner_amd.vigo import (GUIDE_DEFERRED, GUIDE_OK, PATHS_DEFERRED, PATHS_FAILED, PATHS_OK, Vigo, VigoError, default_params)

pytestmark = pytest.mark.gpu
FILL = -7
CAP = 512                                                         # search_path_cap
POINT_CAP = 1 << 17
INT32_MAX = 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _np(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def pair_cap(B, N):
    return B * (N + 4 * rc.MAX_SEGS) + 8


@pytest.fixture(scope="module")
def hlib():
    return pc.host_lib()


@pytest.fixture(scope="module")
def cases():
    """the crafted batches (both ratios) and the derived batch — built once, never changed"""
    return {"crafted 0.0": pm.crafted_case(0.0), "crafted 0.3": pm.crafted_case(0.3), "derived": pm.derived_case()[0]}


# ---- one call of every entry, mixed or uniform, as per-row records -------------------------------------------------------
def run_segs(v, case, ctrl, n_pts):
    """vigo_collision_segs[_mixed] -> per row (status, segments), raw buffers"""
    d = v.device
    cap = len(ctrl) * pc.MAX_SEGS
    if n_pts is None:
        out = v.collision_segs(to_dev(ctrl, d), case.ncr, seg_cap=cap, fill=FILL)
    else:
        out = v.collision_segs_mixed(to_dev(n_pts, d), to_dev(ctrl, d), case.ncr, seg_cap=cap, fill=FILL)
    torch.cuda.synchronize()
    seg_off, seg, st = _np(out)
    S = int(seg_off[-1])
    assert (seg[S:] == FILL).all()
    return [(int(st[b]), seg[seg_off[b]:seg_off[b + 1]].copy()) for b in range(len(ctrl))]


def run_search(v, case, ctrl, n_pts, seg_off=None, seg=None):
    """vigo_path_search[_mixed] -> per row (status, segments, [paths], counts), the device tensors of the outputs"""
    d = v.device
    B = len(ctrl)
    kw = dict(seg_off=to_dev(seg_off, d), seg=to_dev(seg, d), not_check_ratio=case.ncr, search_path_cap=CAP, seg_cap=B * pc.MAX_SEGS,
              point_cap=POINT_CAP, fill=FILL)
    step = case.res if case.step_ is None else case.step_
    if n_pts is None:
        out = v.path_search(to_dev(ctrl, d), step, case.pool, case.cfg[1], case.cfg[2], **kw)
    else:
        out = v.path_search_mixed(to_dev(n_pts, d), to_dev(ctrl, d), step, case.pool, case.cfg[1], case.cfg[2], **kw)
    torch.cuda.synchronize()
    st, so, sg, po, pa, counts = _np(out)
    S = int(so[B])
    P = int(po[S])
    assert (sg[S:] == FILL).all() and (po[S + 1:] == FILL).all() and (pa[P:] == float(FILL)).all()      # nothing beyond the totals
    r = pc.Result(0, st, so, sg[:S], po[:S + 1], pa[:P], counts)
    return [r.of(b) + (counts[b].copy(),) for b in range(B)], out


def same_search(a, e):
    return (a[0] == e[0] and np.array_equal(a[1], e[1]) and len(a[2]) == len(e[2]) and np.array_equal(a[3], e[3]) and
            all(x.shape == y.shape and np.array_equal(bits(x), bits(y)) for x, y in zip(a[2], e[2])))


def run_guides(v, ctrl, n_pts, search_out):
    """vigo_guide_assign[_mixed] on the device tensors of a path search -> per row (status, [per control point (pv bits, unk)]),
    the device tensors"""
    d = v.device
    B, N = ctrl.shape[0], ctrl.shape[1]
    cap = pair_cap(B, N)
    _, so, sg, po, pa, _ = search_out
    if n_pts is None:
        out = v.guide_assign(to_dev(ctrl, d), so, sg, po, pa, cap, fill=FILL)
    else:
        out = v.guide_assign_mixed(to_dev(n_pts, d), to_dev(ctrl, d), so, sg, po, pa, cap, fill=FILL)
    torch.cuda.synchronize()
    off, pv, unk, st = _np(out)
    G = int(off[-1])
    assert off[0] == 0 and (np.diff(off) >= 0).all() and (pv[G:] == float(FILL)).all() and (unk[G:] == (FILL & 0xFF)).all()
    rows = []
    for b in range(B):
        n = N if n_pts is None else int(n_pts[b])
        o = off[b * N:(b + 1) * N + 1]
        if not 7 <= n <= N:
            n = 0
        assert (o[n:] == o[N]).all()                      # the padded control points own empty ranges
        rows.append((int(st[b]), [(bits(pv[o[i]:o[i + 1]]), unk[o[i]:o[i + 1]].copy()) for i in range(n)]))
    return rows, out


def same_pairs(a, e):
    return a[0] == e[0] and len(a[1]) == len(e[1]) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a[1], e[1]))


def run_reguide(v, case, ctrl, n_pts, goff, gpv, weights, state):
    """vigo_rebound_reguide[_mixed] -> per row (status, state bytes, weights bits, [pairs per control point], [paths])"""
    d = v.device
    B, N = ctrl.shape[0], ctrl.shape[1]
    helper = rc.Case("", case.vox, case.origin, case.res, case.cfg, ctrl, goff, gpv, weights, state)
    t_goff, t_gpv = to_dev(goff, d), to_dev(np.concatenate([gpv.reshape(-1, 6), np.zeros((1, 6))]), d)
    t_gunk = to_dev(np.concatenate([helper.gunk(), np.zeros(1, dtype=np.uint8)]), d)
    t_w, t_st = to_dev(weights, d), to_dev(state, d)
    cap = len(gpv) + pair_cap(B, N)
    args = (to_dev(ctrl, d), t_goff, t_gpv, t_gunk, t_w, t_st, case.res if case.step_ is None else case.step_, case.pool, case.cfg[1], case.cfg[2], cap)
    kw = dict(not_check_ratio=case.ncr, search_path_cap=CAP, seg_cap=B * rc.MAX_SEGS, point_cap=POINT_CAP, fill=FILL)
    out = v.rebound_reguide(*args, **kw) if n_pts is None else v.rebound_reguide_mixed(to_dev(n_pts, d), *args, **kw)
    torch.cuda.synchronize()
    st, off, pv, unk, pso, po, pa = _np(out)
    G, S = int(off[-1]), int(pso[B])
    P = int(po[S])
    assert off[0] == 0 and (np.diff(off) >= 0).all()
    assert (pv[G:] == float(FILL)).all() and (unk[G:] == (FILL & 0xFF)).all() and (po[S + 1:] == FILL).all() and (pa[P:] == float(FILL)).all()
    w_out, s_out = t_w.cpu().numpy(), t_st.cpu().numpy()
    rows = []
    for b in range(B):
        o = off[b * N:(b + 1) * N + 1]
        n = N if n_pts is None else int(n_pts[b])
        keep = n if 7 <= n <= N else N                    # (a bad count: its old pairs are copied wherever they lie)
        if keep < N:
            assert (o[keep:] == o[N]).all() or (np.diff(goff[b * N + keep:(b + 1) * N + 1]) > 0).any()
        paths = [bits(pa[po[k]:po[k + 1]]) for k in range(pso[b], pso[b + 1])]
        rows.append((int(st[b]), s_out[b].tobytes(), bits(w_out[b]), [(bits(pv[o[i]:o[i + 1]]), unk[o[i]:o[i + 1]].copy()) for i in range(keep)], paths))
    return rows, (out, t_w, t_st)


def same_reguide(a, e):
    return (a[0] == e[0] and a[1] == e[1] and np.array_equal(a[2], e[2]) and same_pairs((0, a[3]), (0, e[3])) and len(a[4]) == len(e[4]) and
            all(np.array_equal(x, y) for x, y in zip(a[4], e[4])))


def uniform_reference(v, case, rows=None):
    """every entry, uniform, per count, on the rows cut to their counts -> per row dict(segs, search, guides[, reguide])"""
    ref = [dict() for _ in range(case.B)]
    for n in case.counts():
        idx = case.rows_of(n)
        ctrl = np.stack([case.rows[b] for b in idx])
        segs = run_segs(v, case, ctrl, None)
        search, dev = run_search(v, case, ctrl, None)
        guides, _ = run_guides(v, ctrl, None, dev)
        reguide = None
        if rows is not None:
            _, c = rows.uniform(case, n)
            reguide, _ = run_reguide(v, case, c.ctrl, None, c.goff, c.gpv, c.weights, c.state)
        for k, b in enumerate(idx):
            ref[b] = dict(segs=segs[k], search=search[k], guides=guides[k], reguide=None if reguide is None else reguide[k])
    return ref


def mixed_run(v, case, ctrl, n_pts, rows=None):
    segs = run_segs(v, case, ctrl, n_pts)
    search, dev = run_search(v, case, ctrl, n_pts)
    guides, gdev = run_guides(v, ctrl, n_pts, dev)
    reguide = None
    if rows is not None:
        goff, gpv = rows.csr(case)
        reguide, _ = run_reguide(v, case, ctrl, n_pts, goff, gpv, rows.weights, rows.state)
    return [dict(segs=segs[b], search=search[b], guides=guides[b], reguide=None if reguide is None else reguide[b]) for b in range(len(ctrl))], (dev, gdev)


def assert_row_equal(got, ref, what):
    assert got["segs"][0] == ref["segs"][0] and np.array_equal(got["segs"][1], ref["segs"][1]), (what, "segments", got["segs"], ref["segs"])
    assert same_search(got["search"], ref["search"]), (what, "path search", got["search"][0], ref["search"][0])
    assert same_pairs(got["guides"], ref["guides"]), (what, "guide pairs")
    if ref.get("reguide") is not None:
        assert same_reguide(got["reguide"], ref["reguide"]), (what, "re-guide", got["reguide"][0], ref["reguide"][0])


# ---- 1. per-count equality ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["crafted 0.0", "crafted 0.3", "derived"])
def test_every_entry_equals_the_uniform_entry_per_count_under_either_padding(vigo_handle, hlib, cases, which):
    v, case = vigo_handle, cases[which]
    v.set_grid(to_dev(case.vox, v.device), case.origin, case.res)
    rows = pm.reguide_rows(hlib, case)
    ref = uniform_reference(v, case, rows)
    got = {}
    for name, poison in (("zero padding", False), ("poisoned padding", True)):
        got[name], _ = mixed_run(v, case, case.padded(poison), case.n_pts, rows)
        for b in range(case.B):
            assert_row_equal(got[name][b], ref[b], (which, name, case.names[b]))
    st = np.array([r["search"][0] for r in ref])
    rg = np.array([r["reguide"][0] for r in ref])
    print(f"\n{case.name}: {case.B} rows of {case.Ns}, counts {case.counts()}; segments {sum(len(r['segs'][1]) for r in ref)}, path search ok / failed / "
          f"deferred {[int((st == k).sum()) for k in (0, 1, 2)]}, pairs {sum(sum(len(p[1]) for p in r['guides'][1]) for r in ref)}, re-guide statuses "
          f"{[int((rg == k).sum()) for k in range(5)]}: mixed == uniform per count, under zero and poisoned padding")
    if which.startswith("crafted"):
        # (under 0.3 the scan of the 120-point zigzag ends before its 49th segment: nothing is deferred there)
        deferred = which == "crafted 0.0"
        assert {PATHS_OK, PATHS_FAILED} | ({PATHS_DEFERRED} if deferred else set()) <= set(st)
        assert set(rg) == {0, 1, 2, 4} | ({3} if deferred else set())
        assert any(r["guides"][0] == GUIDE_OK and sum(len(p[1]) for p in r["guides"][1]) for r in ref)


def test_a_supplied_segment_list_is_held_against_the_own_count(vigo_handle, hlib, cases):
    """vigo_path_search_mixed on a caller's list: the scanned segments handed back in give the scan's result; an end that
    lies inside the row but beyond the trajectory's count is a call-level error and nothing is written"""
    v, case = vigo_handle, cases["crafted 0.0"]
    v.set_grid(to_dev(case.vox, v.device), case.origin, case.res)
    ctrl, n_pts = case.padded(True), case.n_pts
    segs = run_segs(v, case, ctrl, n_pts)
    seg_off = np.concatenate([[0], np.cumsum([len(s[1]) for s in segs])]).astype(np.int32)
    seg = np.concatenate([s[1].reshape(-1, 2) for s in segs] + [np.zeros((1, 2), dtype=np.int32)]).astype(np.int32)
    scanned, _ = run_search(v, case, ctrl, n_pts)
    listed, _ = run_search(v, case, ctrl, n_pts, seg_off, seg)
    for b in range(case.B):
        if segs[b][0] == PATHS_OK:
            assert same_search(listed[b], scanned[b]), case.names[b]
    b = next(b for b in range(case.B) if n_pts[b] == 12 and len(segs[b][1]))
    bad = seg.copy()
    bad[seg_off[b], 1] = 12                               # inside the row of 120, not a control point of this trajectory
    with pytest.raises(VigoError):
        run_search(v, case, ctrl, n_pts, seg_off, bad)
    d = v.device
    st = torch.full((case.B,), 77, dtype=torch.int32, device=d)
    outs = [torch.full(s, 77, dtype=torch.int32, device=d) for s in ((case.B + 1,), (64, 2), (65,))] + [torch.full((64, 3), 77.0, dtype=torch.float64, device=d)]
    import ctypes as C
    p = lambda t: C.c_void_p(t.data_ptr())
    rc_ = v._lib.vigo_path_search_mixed(v._h, case.B, case.Ns, p(to_dev(n_pts, d)), p(to_dev(ctrl, d)), p(to_dev(seg_off, d)), p(to_dev(bad, d)), 0.0,
                                        case.res, (C.c_int32 * 3)(*case.pool), float(case.cfg[1]), float(case.cfg[2]), 1 << 20, CAP, 64, 64, p(st),
                                        p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), None)
    torch.cuda.synchronize()
    assert rc_ == -1 and (st == 77).all() and all((t == 77).all() for t in outs)


# ---- 2. order independence and chaining --------------------------------------------------------------------------------
def test_a_trajectory_alone_and_the_reversed_batch(vigo_handle, hlib, cases):
    v, case = vigo_handle, cases["crafted 0.0"]
    v.set_grid(to_dev(case.vox, v.device), case.origin, case.res)
    rows = pm.reguide_rows(hlib, case)
    got, _ = mixed_run(v, case, case.padded(True), case.n_pts, rows)
    # alone, B = 1 and Ns = its count: of every count the row with the most segments
    for n in case.counts():
        b = max(case.rows_of(n), key=lambda b: len(got[b]["segs"][1]))
        one = case.subset([b])
        assert one.Ns == n
        r1 = pm.ReguideRows(rows.state[[b]], rows.weights[[b]], [rows.pairs[b]])
        alone, _ = mixed_run(v, one, one.padded(), one.n_pts, r1)
        assert_row_equal(alone[0], got[b], ("alone", case.names[b]))
    # reversed: the reversed results
    order = list(range(case.B))[::-1]
    rev = case.subset(order, Ns=case.Ns)
    r2 = pm.ReguideRows(rows.state[order], rows.weights[order], [rows.pairs[b] for b in order])
    back, _ = mixed_run(v, rev, rev.padded(True), rev.n_pts, r2)
    for k, b in enumerate(order):
        assert_row_equal(back[k], got[b], ("reversed", case.names[b]))


@pytest.mark.parametrize("cls", [32, 64])
def test_the_device_tensors_chain_into_optimize_mixed(cases, cls):
    """path_search_mixed -> guide_assign_mixed -> optimize_mixed on the tensors as they lie, against the uniform chain per count"""
    P = default_params()
    P.max_iterations = 30
    v = Vigo(0, P)
    d = v.device
    full = cases["crafted 0.0"]
    keep = [b for b in range(full.B) if (cls == 32 and len(full.rows[b]) <= 32) or (cls == 64 and 32 < len(full.rows[b]) <= 64)]
    case = full.subset(keep, Ns=cls)
    assert case.B >= 15 and len(case.counts()) >= 3
    v.set_grid(to_dev(case.vox, d), case.origin, case.res)
    ctrl, n_pts = case.padded(True), case.n_pts
    t_ctrl, t_n = to_dev(ctrl, d), to_dev(n_pts, d)
    _, dev = run_search(v, case, ctrl, n_pts)
    rows_m, (off, pv, unk, gst) = run_guides(v, ctrl, n_pts, dev)
    G = int(off[-1].item())
    assert G > 0
    r = v.optimize_mixed(t_n, t_ctrl, off, pv, unk)
    torch.cuda.synchronize()
    out, status = r.ctrl.cpu().numpy(), r.status.cpu().numpy()
    moved = 0
    for n in case.counts():
        idx = case.rows_of(n)
        c = np.stack([case.rows[b] for b in idx])
        _, dev_u = run_search(v, case, c, None)
        _, (off_u, pv_u, unk_u, _) = run_guides(v, c, None, dev_u)
        ru = v.optimize(to_dev(c, d), off_u, pv_u, unk_u)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out[idx][:, :n]), bits(ru.ctrl.cpu().numpy())), n
        assert np.array_equal(status[idx], ru.status.cpu().numpy()), n
        moved += int((bits(out[idx][:, :n]) != bits(c)).any())
    assert moved >= 2                                     # the guides pulled control points
    v.close()


# ---- 3. bad counts and the error contract -------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", pm.BAD_COUNTS)
def test_a_bad_count_in_the_middle_of_a_good_batch(vigo_handle, hlib, cases, bad):
    v, full = vigo_handle, cases["crafted 0.0"]
    case = full.subset(list(range(21)), Ns=full.Ns)
    v.set_grid(to_dev(case.vox, v.device), case.origin, case.res)
    rows = pm.reguide_rows(hlib, case)
    ctrl, n_pts = case.padded(True), case.n_pts.copy()
    good, _ = mixed_run(v, case, ctrl, n_pts, rows)
    m = next(b for b in range(8, 16) if len(good[b]["segs"][1]) and rows.state[b, rc.S_STATUS] == rc.RB_NEEDS_HOST and rows.pairs[b])
    n_pts[m] = case.Ns + 1 if bad is None else bad
    got, _ = mixed_run(v, case, ctrl, n_pts, rows)
    for b in range(case.B):
        if b != m:
            assert_row_equal(got[b], good[b], ("next to a bad count", case.names[b]))
    r = got[m]
    assert r["segs"][0] == PATHS_DEFERRED and len(r["segs"][1]) == 0
    assert r["search"][0] == PATHS_DEFERRED and len(r["search"][1]) == 0 and len(r["search"][2]) == 0 and list(r["search"][3]) == [0, 0]
    assert r["guides"][0] == GUIDE_DEFERRED and r["guides"][1] == []
    status, state, weights, pairs, paths = r["reguide"]
    assert status == rc.DEFERRED and state == rows.state[m].tobytes() and np.array_equal(weights, bits(rows.weights[m])) and paths == []
    # the merged CSR copies its old pairs, every one of them
    old = [np.array([np.concatenate([p, q]) for p, q in rows.pairs[m].get(i, [])]).reshape(-1, 6) for i in range(case.Ns)]
    assert sum(len(o) for o in old) > 0 and all(np.array_equal(pairs[i][0], bits(old[i])) for i in range(case.Ns))


def test_call_level_errors_write_nothing_and_an_empty_batch_is_a_no_op(vigo_handle, cases):
    import ctypes as C
    v, full = vigo_handle, cases["crafted 0.0"]
    case = full.subset(list(range(5)), Ns=full.Ns)
    d = v.device
    lib = v._lib
    B, Ns = case.B, case.Ns
    ctrl, n_pts = to_dev(case.padded(True), d), to_dev(case.n_pts, d)
    i32 = lambda *s: torch.full(s, 77, dtype=torch.int32, device=d)
    f64 = lambda *s: torch.full(s, 77.0, dtype=torch.float64, device=d)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    pool = (C.c_int32 * 3)(*case.pool)
    o_st, o_so, o_sg, o_po, o_pa, o_off, o_pv = i32(B), i32(B + 1), i32(64, 2), i32(65), f64(4096, 3), i32(B * Ns + 1), f64(4096, 6)
    state, weights = to_dev(rc.make_state(B), d), to_dev(np.ones((B, 4)), d)
    state0 = state.clone()
    seg_off, seg, path_off, path = to_dev(np.zeros(B + 1, dtype=np.int32), d), i32(1, 2), to_dev(np.zeros(1, dtype=np.int32), d), f64(1, 3)

    def calls(B_, Ns_, n_):
        search = (0.0, case.res, pool, float(case.cfg[1]), float(case.cfg[2]), 1 << 20, CAP)
        return [
            lib.vigo_collision_segs_mixed(v._h, B_, Ns_, p(n_), p(ctrl), 0.0, p(o_so), p(o_sg), 64, p(o_st)),
            lib.vigo_path_search_mixed(v._h, B_, Ns_, p(n_), p(ctrl), None, None, *search, 64, 4096, p(o_st), p(o_so), p(o_sg), p(o_po), p(o_pa), None),
            lib.vigo_guide_assign_mixed(v._h, B_, Ns_, p(n_), p(ctrl), p(seg_off), p(seg), p(path_off), p(path), 4096, p(o_off), p(o_pv), None, p(o_st)),
            lib.vigo_rebound_reguide_mixed(v._h, B_, Ns_, p(n_), p(ctrl), None, None, None, p(weights), *search, p(state), 4096, p(o_off), p(o_pv), None,
                                           64, 4096, None, None, None, p(o_st)),
        ]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 77).all()) for t in (o_st, o_so, o_sg, o_po, o_pa, o_off, o_pv)) and torch.equal(state, state0) and bool((weights == 1.0).all())

    assert calls(B, Ns, n_pts) == [-5] * 4 and untouched()                        # VIGO_ERR_NO_GRID
    v.set_grid(to_dev(case.vox, d), case.origin, case.res)
    assert calls(B, Ns, None) == [-1] * 4 and untouched()                         # n_pts == NULL: VIGO_ERR_INVALID_ARG
    for Ns_bad in (6, 257):
        assert calls(B, Ns_bad, n_pts) == [-4] * 4 and untouched()                # VIGO_ERR_UNSUPPORTED_N
    assert calls(-1, Ns, n_pts) == [-1] * 4 and untouched()
    assert calls(0, Ns, None) == [0] * 4 and untouched()                          # B = 0: a no-op, every array may be NULL
    # the capacities: the segments of the batch do not fit one slot, its pairs do not fit none
    assert lib.vigo_collision_segs_mixed(v._h, B, Ns, p(n_pts), p(ctrl), 0.0, p(o_so), p(o_sg), 1, p(o_st)) == -1 and untouched()
    st, so, sg, po, pa, _ = v.path_search_mixed(n_pts, ctrl, case.res, case.pool, case.cfg[1], case.cfg[2], search_path_cap=CAP, point_cap=POINT_CAP)
    assert int(so[-1].item()) >= 2
    assert lib.vigo_guide_assign_mixed(v._h, B, Ns, p(n_pts), p(ctrl), p(so), p(sg), p(po), p(pa), 1, p(o_off), p(o_pv), None, p(o_st)) == -1 and untouched()
    # for the re-guide, guide_off must not decrease over ALL B * Ns + 1 entries: a dip inside the padding of row 0
    goff = np.zeros(B * Ns + 1, dtype=np.int32)
    goff[int(case.n_pts[0]) + 2] = 1
    t_goff, t_gpv = to_dev(goff, d), f64(2, 6)
    search = (0.0, case.res, pool, float(case.cfg[1]), float(case.cfg[2]), 1 << 20, CAP)
    assert lib.vigo_rebound_reguide_mixed(v._h, B, Ns, p(n_pts), p(ctrl), p(t_goff), p(t_gpv), None, p(weights), *search, p(state), 4096, p(o_off), p(o_pv),
                                          None, 64, 4096, None, None, None, p(o_st)) == -1 and untouched()
