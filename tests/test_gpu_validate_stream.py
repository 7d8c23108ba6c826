"""-m gpu: vigo_traj_validate on a side stream behind a producer that is still running — the row tests/stream_cases.py would
hold for it (the entry is declared in include/vigo_validate.h, so the table of include/vigo.h's entries does not list it),
run through the functions of tests/test_gpu_stream_order.py with its four assertions: (a) the inputs are still the decoy when
the host reaches the call, (b) and when the call returns — the entry makes no host round trip, (c) every output equals the
default-stream reference byte for byte, (d) the decoy gives another answer.  The inputs are validate_cases.stream_inputs():
three counts in one stride; the decoy has the batch reversed, the counts permuted, the obstacle CSR rebuilt and the second
small world.  (d) also holds by the host twin, on the CPU, in tests/test_validate_core.py."""
import numpy as np
import pytest
import torch

import stream_cases as sc
import validate_cases as vc
from test_gpu_stream_order import DELAY_MS, behind_a_producer, cycles_per_ms, differing, handle_for, reference  # noqa: F401 (cycles_per_ms: a fixture)

pytestmark = pytest.mark.gpu


def row():
    real, decoy, world = vc.stream_inputs()
    origin, res = tuple(float(x) for x in world.origin), float(world.res)

    def call(v, t):
        v.set_grid(t["vox"], origin, res)
        r = v.traj_validate(t["ctrl"], vc.STREAM_DT, n_pts=t["n_pts"], not_check_ratio=vc.STREAM_RATIO, rule=vc.STREAM_RULE, obs_off=t["obs_off"],
                            obs=t["obs"])
        return [r[k] for k in vc.KEYS]

    c = lambda d: {k: np.ascontiguousarray(a) for k, a in d.items()}
    return sc.Row("traj_validate", "vigo_traj_validate", c(real), c(decoy), call, no_round_trip=True, twin=vc.stream_twin,
                  notes="the per-count table is copied in stream order from the handle's pinned stage; the clock is filled by a kernel")


def test_traj_validate_behind_a_pending_producer(cycles_per_ms):  # noqa: F811
    r = row()
    name = r.name
    dev = torch.device("cuda", 0)
    t_real, t_decoy, want, want_decoy = reference(r, dev)
    assert len(want) == len(want_decoy) == len(vc.KEYS)
    assert differing(want, want_decoy), f"(d) {name}: the decoy gives the real inputs' result: the row cannot discriminate"
    twin = r.twin(r.real)
    assert [w[1] for w in want] == [np.ascontiguousarray(a).tobytes() for a in twin], "the default-stream reference is not the host twin's answer"
    v = handle_for(r)
    try:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):
            v.use_current_stream()
        before, after, took, got = behind_a_producer(s, int(DELAY_MS * cycles_per_ms), t_real, t_decoy, lambda bufs: r.call(v, bufs))
        torch.cuda.synchronize()
    finally:
        v.close()
    print(f"\n{name}: the call returned to the host after {took * 1e3:.3f} ms; inputs still pending before / after it: {before} / {after}")
    bad = differing(got, want)
    assert [g[0] for g in got] == [w[0] for w in want] and not bad, f"(c) {name}: outputs {bad} differ from the default-stream reference" + (
        "; they are the DECOY's" if bad and all(got[k] == want_decoy[k] for k in bad) else "")
    assert before, f"(a) {name}: the inputs were complete before the call was made: the delay of {DELAY_MS} ms is too short"
    assert after, f"(b) {name}: the inputs were complete when the call returned ({took * 1e3:.3f} ms): a host wait, or the delay is too short"
