"""-m gpu: every handle entry point on a side stream BEHIND A PRODUCER THAT IS STILL RUNNING (the production path: the facades
chain the device stages on one non-blocking stream and the host does not wait in between).

One row of tests/stream_cases.py per entry point.  Reference phase: a fresh handle on the default stream, a device
synchronise before and after, the call on the real inputs and on the decoy.  Test phase: a second fresh handle bound to a
side stream s; on s, with no host wait in between: the buffers the call will read hold the DECOY; a delay kernel; device
copies overwrite the buffers with the real inputs; the event `produced`; the call; device clones of every output and of
the arrays updated in place; s.synchronize().  Asserted: (a) `produced` has not happened when the host reaches the call —
the inputs are still the decoy; (b) for the rows of stream_cases.NO_ROUND_TRIP, nor when the call returns; (c) every
output equals the reference's real-input result byte for byte; (d) the reference's decoy result differs from it.  A call
that read an input before its stream said so, a launch, memset or count read-back on another stream, gives the decoy's
answer and fails (c).  Two more tests: the prologue chain into optimize_mixed behind one delay, and a handle re-bound
between two streams under cached tables.

The outputs the wrappers allocate with torch.empty start as a sentinel during every call (sentinel_outputs), the others as
the zeros or the `fill` the wrappers document: an output the call did not write shows.

The delay is a measured number.  On an MI355X the slowest entry of the NO_ROUND_TRIP column returns to the host, on a cold
handle, after SLOWEST_COLD_CALL_MS = 0.12 ms (vigo_pack_grid, the first row: 0.10 - 0.12 ms over three runs; the others
take 0.02 - 0.10 ms; the test prints every row's time).  DELAY_MS = 40 ms is 330 times that: ten times would cover the call itself, the rest covers the host's
jitter on a shared machine, the copies queued in front of the call and the installs of the rebind test.  The delay kernel is
torch.cuda._sleep: 2.40e6 of its cycles take one millisecond there, measured once per session by two events around it
(cycles_per_ms), so the delay is about 9.6e7 cycles.  If (a) or (b) fails while (c) holds, the delay was too short."""
import time
from unittest import mock

import numpy as np
import pytest
import torch

import stream_cases as sc
from trajectory_planner_amd.vigo import Vigo, default_params

pytestmark = pytest.mark.gpu

SLOWEST_COLD_CALL_MS = 0.12       # measured: see the docstring
DELAY_MS = 40.0
assert DELAY_MS >= 10 * SLOWEST_COLD_CALL_MS
SENTINELS = {torch.float64: -7.25e33, torch.float32: -7.25e33, torch.int32: -7, torch.uint8: 0xA5}


@pytest.fixture(scope="module")
def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, by two events around a sleep of a few milliseconds"""
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    cycles = 2_000_000
    for _ in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 5.0:
            break
        cycles *= 4
    assert ms >= 5.0, f"torch.cuda._sleep({cycles}) took {ms} ms"
    rate = cycles / ms
    print(f"\ntorch.cuda._sleep: {cycles} cycles in {ms:.3f} ms = {rate:.0f} cycles per ms; the delay of {DELAY_MS} ms is {int(DELAY_MS * rate)} cycles")
    return rate


class sentinel_outputs:
    """while it is open, a tensor from torch.empty (the wrappers' output buffers) holds a sentinel, filled in stream order"""

    def __enter__(self):
        empty = torch.empty

        def filled(*size, **kw):
            t = empty(*size, **kw)
            return t.fill_(SENTINELS[t.dtype]) if t.is_cuda and t.dtype in SENTINELS else t
        self.patch = mock.patch.object(torch, "empty", filled)
        self.patch.start()

    def __exit__(self, *a):
        self.patch.stop()


def upload(arrays, dev):
    return {k: torch.from_numpy(a).to(dev) for k, a in arrays.items()}


def clones(t):
    return {k: x.clone() for k, x in t.items()}


def snapshot(outs):
    return [o.clone() if isinstance(o, torch.Tensor) else o for o in outs]


def host(outs):
    """after a synchronise: every output as (shape, bytes)"""
    got = []
    for o in outs:
        a = np.ascontiguousarray(o.cpu().numpy()) if isinstance(o, torch.Tensor) else np.asarray(o)
        got.append((a.shape, a.tobytes()))
    return got


def handle_for(row):
    P = default_params()
    if row.params is not None:
        row.params(P)
    return Vigo(0, P)


def reference(row, dev):
    """-> (the device inputs real and decoy, derived ones included; the results on the real inputs and on the decoy)"""
    torch.cuda.synchronize()
    t_real, t_decoy = upload(row.real, dev), upload(row.decoy, dev)
    if row.derive is not None:
        v = handle_for(row)
        try:
            for t in (t_real, t_decoy):
                t.update({k: x.clone().contiguous() for k, x in row.derive(v, t).items()})
                torch.cuda.synchronize()
        finally:
            v.close()
    v = handle_for(row)
    try:
        with sentinel_outputs():
            want = snapshot(row.call(v, clones(t_real)))
            torch.cuda.synchronize()
            want_decoy = snapshot(row.call(v, clones(t_decoy)))
            torch.cuda.synchronize()
    finally:
        v.close()
    return t_real, t_decoy, host(want), host(want_decoy)


def behind_a_producer(s, delay_cycles, t_real, t_decoy, work):
    """on s: buffers holding the decoy, the delay, the copies of the real inputs, `produced`, work(buffers); the outputs cloned
    on s; one synchronise at the end -> (produced had not happened before / after the work, host seconds of the work, outputs)"""
    with torch.cuda.stream(s):
        bufs = clones(t_decoy)
        torch.cuda._sleep(delay_cycles)
        for k, b in bufs.items():
            b.copy_(t_real[k])
        produced = torch.cuda.Event()
        produced.record(s)
        before = not produced.query()
        t0 = time.perf_counter()
        with sentinel_outputs():
            outs = work(bufs)
        took = time.perf_counter() - t0
        after = not produced.query()
        snap = snapshot(outs)
        s.synchronize()
    return before, after, took, host(snap)


def differing(a, b):
    return [k for k, (x, y) in enumerate(zip(a, b)) if x != y]


@pytest.mark.parametrize("name", sc.ROW_NAMES)
def test_entry_point_behind_a_pending_producer(name, cycles_per_ms):
    row = sc.by_name(name)
    dev = torch.device("cuda", 0)
    t_real, t_decoy, want, want_decoy = reference(row, dev)
    assert len(want) == len(want_decoy) > 0
    assert differing(want, want_decoy), f"(d) {name}: the decoy gives the real inputs' result: the row cannot discriminate"
    v = handle_for(row)
    try:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            v.use_current_stream()
        before, after, took, got = behind_a_producer(s, int(DELAY_MS * cycles_per_ms), t_real, t_decoy, lambda bufs: row.call(v, bufs))
        torch.cuda.synchronize()
    finally:
        v.close()
    print(f"\n{name}: the call returned to the host after {took * 1e3:.3f} ms; inputs still pending before / after it: {before} / {after}"
          f" ({'no round trip' if row.no_round_trip else 'round trip'})")
    bad = differing(got, want)
    assert [g[0] for g in got] == [w[0] for w in want] and not bad, f"(c) {name}: outputs {bad} differ from the default-stream reference" + (
        "; they are the DECOY's" if bad and all(got[k] == want_decoy[k] for k in bad) else "")
    assert before, f"(a) {name}: the inputs were complete before the call was made: the delay of {DELAY_MS} ms is too short"
    if row.no_round_trip:
        assert after, f"(b) {name}: the inputs were complete when the call returned ({took * 1e3:.3f} ms): a host wait, or the delay is too short"


# ---- the chain: segments -> search -> guides -> optimize_mixed behind one delay ---------------------------------------------
def _chain(v, t, case, between):
    """tests/test_gpu_prologue_mixed.py's composition on the device tensors as they lie; between(): what the host does between
    two stages -> every stage's outputs"""
    v.set_grid(t["vox"], tuple(float(x) for x in case.origin), float(case.res))
    B, Ns = t["ctrl"].shape[:2]
    kw = dict(not_check_ratio=case.ncr, search_path_cap=sc.PROLOGUE_CAP, seg_cap=B * 48, point_cap=sc.PROLOGUE_POINT_CAP, fill=-7)
    segs = v.collision_segs_mixed(t["n_pts"], t["ctrl"], case.ncr, seg_cap=B * 48, fill=-7)
    between()
    search = v.path_search_mixed(t["n_pts"], t["ctrl"], float(case.res), case.pool, case.cfg[1], case.cfg[2], **kw)
    between()
    _, so, sg, po, pa, _ = search
    guides = v.guide_assign_mixed(t["n_pts"], t["ctrl"], so, sg, po, pa, B * (Ns + 4 * 48) + 8, fill=-7)
    between()
    off, pv, unk, _ = guides
    r = v.optimize_mixed(t["n_pts"], t["ctrl"], off, pv, unk)
    between()
    return list(segs) + list(search) + list(guides) + [r.ctrl, r.x, r.status, r.fx, r.iters, r.evals]


def test_the_prologue_chain_into_optimize_mixed_behind_one_delay(cycles_per_ms):
    _, _, case = sc.prologue_cases()
    dev = torch.device("cuda", 0)
    P = default_params()
    P.max_iterations = 20
    rev = case.subset(range(case.B)[::-1], Ns=case.Ns)
    t_real = upload(dict(vox=case.vox, ctrl=case.padded(), n_pts=case.n_pts), dev)
    t_decoy = upload(dict(vox=sc.second_world(case.vox, 2), ctrl=rev.padded(), n_pts=rev.n_pts), dev)
    torch.cuda.synchronize()
    v = Vigo(0, P)
    try:
        with sentinel_outputs():
            want = host(snapshot(_chain(v, clones(t_real), case, torch.cuda.synchronize)))
            want_decoy = host(snapshot(_chain(v, clones(t_decoy), case, torch.cuda.synchronize)))
    finally:
        v.close()
    assert differing(want, want_decoy)
    moved = np.frombuffer(want[13][1], dtype=np.float64).reshape(want[13][0])
    assert int(np.frombuffer(want[9][1], dtype=np.int32)[-1]) > 0 and not np.array_equal(moved, case.padded())    # guide pairs, and they pulled
    v = Vigo(0, P)
    try:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            v.use_current_stream()
        before, _, took, got = behind_a_producer(s, int(DELAY_MS * cycles_per_ms), t_real, t_decoy, lambda bufs: _chain(v, bufs, case, lambda: None))
        torch.cuda.synchronize()
    finally:
        v.close()
    assert not differing(got, want), f"outputs {differing(got, want)} of the chain on the side stream differ from the synchronised chain"
    assert before, f"the inputs were complete before the chain started: the delay of {DELAY_MS} ms is too short"


# ---- the rebind: cached state installed on one stream, used on another, and back ----------------------------------------------
def test_a_handle_rebound_between_two_streams_under_cached_tables(cycles_per_ms):
    """grid, ESDF, parameters, fit operator, fit table, the gates' clock table and both finish clock tables are installed on s1
    behind a delay; the handle switches to s2 at once and uses them, then back to s1 and again: vigo_set_stream's wait on the
    old stream, and the hand-over of the clock tables' streams"""
    dev = torch.device("cuda", 0)
    fit, fitm, fin, opt = (sc.by_name(n) for n in ("bspline_fit", "bspline_fit_mixed", "traj_finish", "optimize"))
    esdf, gate = sc.by_name("esdf_query"), sc.by_name("traj_collision")
    P = default_params()
    fin.params(P)
    P.max_iterations = 15
    P.w_smoothness *= 2.0
    t = {n: upload(r.real, dev) for n, r in (("fit", fit), ("fitm", fitm), ("fin", fin), ("opt", opt), ("esdf", esdf), ("gate", gate))}
    torch.cuda.synchronize()

    def install(v):
        v.set_params(P)
        return esdf.call(v, clones(t["esdf"])) + gate.call(v, clones(t["gate"])) + fin.call(v, clones(t["fin"])) + fit.call(v, clones(t["fit"])) + \
            fitm.call(v, clones(t["fitm"]))

    def use(v):
        ctrl = t["gate"]["ctrl"]
        return list(v.traj_collision(ctrl, 0.05)) + fin.call(v, clones(t["fin"])) + fit.call(v, clones(t["fit"])) + fitm.call(v, clones(t["fitm"])) + \
            list(v.esdf_query(t["esdf"]["pts"])) + opt.call(v, clones(t["opt"]))

    v = Vigo(0)
    try:
        install(v)
        torch.cuda.synchronize()
        want = host(snapshot(use(v)))
    finally:
        v.close()
    v = Vigo(0)
    try:
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        with torch.cuda.stream(s1):
            v.use_current_stream()
            torch.cuda._sleep(int(DELAY_MS * cycles_per_ms))
            install(v)
            installed = torch.cuda.Event()
            installed.record(s1)
            pending = not installed.query()
        with torch.cuda.stream(s2):
            v.use_current_stream()
            on_s2 = snapshot(use(v))
        with torch.cuda.stream(s1):
            v.use_current_stream()
            on_s1 = snapshot(use(v))
        s2.synchronize()
        s1.synchronize()
        got2, got1 = host(on_s2), host(on_s1)
        torch.cuda.synchronize()
    finally:
        v.close()
    assert not differing(got2, want), f"outputs {differing(got2, want)} on the second stream differ from the default-stream reference"
    assert not differing(got1, want), f"outputs {differing(got1, want)} back on the first stream differ from the default-stream reference"
    assert pending, f"the installs had completed before the handle was re-bound: the delay of {DELAY_MS} ms is too short"
