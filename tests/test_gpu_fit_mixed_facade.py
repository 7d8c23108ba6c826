"""-m gpu: bsplineTraj::setMixedFit through vigo_host_seed_batch (host/src/cabi_host.cpp) — the fit stage of seedPathBatch as
ONE vigo_bspline_fit_mixed call per knot span against the per-count vigo_bspline_fit launches, on the 64-pair workloads
of seed_cases.py and on the 24-planner mixed batch of test_gpu_seed_facade.py, with the device seed off and on.  The mixed
entry gives a path the bits of the uniform one (test_gpu_fit_mixed.py), so everything the harness returns is IDENTICAL
between the two settings: seeds, counts, statuses, control points, and who decided each planner."""
import ctypes as C

import numpy as np
import pytest

import seed_cases as sc
from test_gpu_seed_facade import seed_batch

pytestmark = pytest.mark.gpu


def both_settings(*args, **kw):
    """seed_batch with the mixed fit on, then off; the process-wide switch is put back whatever happens"""
    L = C.CDLL(sc.HOST_LIB)
    L.vigo_host_set_mixed_fit.argtypes = [C.c_int]
    L.vigo_host_set_mixed_fit.restype = C.c_int
    was = L.vigo_host_set_mixed_fit(1)
    try:
        assert L.vigo_host_set_mixed_fit(1) == 1                  # the setter returns what it replaces
        on = seed_batch(*args, **kw)
        assert L.vigo_host_set_mixed_fit(0) == 1
        off = seed_batch(*args, **kw)
    finally:
        L.vigo_host_set_mixed_fit(was)
    return on, off


def assert_identical(on, off, who=None):
    who = list(range(len(on["seed_n"]))) if who is None else who
    for k in ("seed_n", "tries", "dt", "status", "ctrl_n", "seed", "ctrl"):
        assert np.array_equal(on[k][who], off[k][who]), (k, np.argwhere(on[k][who] != off[k][who])[:5])
    assert np.array_equal(on["totals"], off["totals"])           # device-decided / host-run planners: the switch moves none


@pytest.mark.parametrize("device", [0, 1])
@pytest.mark.parametrize("which", ["open", "pillar"])
def test_mixed_fit_installs_the_control_points_of_the_per_count_route(which, device, capfd):
    world, pairs = sc.workload_world(which), sc.workload_pairs(which)
    on, off = both_settings(world, pairs, 1000.0, device=device)
    out = capfd.readouterr().out
    assert "vigo_bspline_fit_mixed failed" not in out and "vigo_bspline_fit failed" not in out
    assert_identical(on, off)
    fitted = on["ctrl_n"][on["ctrl_n"] > 0]
    assert len(fitted) >= 48 and len(set(fitted.tolist())) >= 4 and fitted.max() <= 64      # many counts, all the mixed route's
    assert (on["totals"][0] >= 60) if device else (on["totals"][0] == 0 and on["totals"][1] == 64)


@pytest.mark.parametrize("device", [0, 1])
def test_mixed_fit_on_the_batch_with_redone_and_host_run_planners(device, capfd):
    world = sc.open_world()
    world.vox[30, 30, 0] |= 1
    pairs = sc.workload_pairs("open")[:24]
    kind = np.zeros(24, np.int32)
    kind[5] = 1                                                  # a bsplineTraj without a device
    kind[9] = 2                                                  # a polyTrajOccMap flying its PWL fallback
    max_len = np.full(24, 1000.0)
    max_len[[3, 4, 12, 17]] = 1.5                                # the length handed down exceeds these: redone on the host
    on, off = both_settings(world, pairs, max_len, kind, prev0=2.5, device=device)
    assert_identical(on, off)
    assert on["status"][5] == 0 and on["status"][9] == 0         # as test_gpu_seed_facade.py finds them
    assert (on["ctrl_n"] > 0).sum() >= 18
    if device:
        assert 1 <= on["totals"][0] <= 18 and on["totals"][1] >= 6
    else:
        assert on["totals"][0] == 0
