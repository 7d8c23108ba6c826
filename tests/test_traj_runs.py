"""-m "not gpu": vigo_traj_sample_runs — where the samples of one whole trajectory fall (rules 1-3 of
vigo_traj_corridor_check, include/vigo.h) — against the literal loop of polyTrajSolver::getTrajectory
(`for (t = 0; t < k[K]; t += delT)`, PS.cpp:1125-1137) with getPose's first-match segment (PS.cpp:1026-1056)."""
import ctypes as C

import numpy as np
import pytest

from trajectory_planner_amd import _lib

OK, BAD_KNOTS, BAD_DELT, STALL, TOO_LONG = 0, 1, 2, 3, 4


def runs(knots, delT):
    k = np.ascontiguousarray(knots, dtype=np.float64)
    K = len(k) - 1
    first = np.full(max(K, 1), -7, dtype=np.int32)
    length = np.full(max(K, 1), -7, dtype=np.int32)
    n_total = C.c_int32(-7)
    st = _lib.load().vigo_traj_sample_runs(K, k.ctypes.data_as(C.c_void_p), float(delT), first.ctypes.data_as(C.c_void_p),
                                           length.ctypes.data_as(C.c_void_p), C.byref(n_total))
    return st, first[:K], length[:K], n_total.value


def literal(knots, delT):
    """the reference's loop and attribution: per sample its segment (-1: none), and n"""
    end = knots[-1]
    seg = []
    t = 0.0
    while t < end:
        s = -1
        for i in range(len(knots) - 1):
            if knots[i] <= t <= knots[i + 1]:
                s = i
                break
        seg.append(s)
        t += delT
    return np.array(seg, dtype=np.int64), t


def check(knots, delT):
    knots = [float(x) for x in knots]
    st, first, length, n_total = runs(knots, delT)
    assert st == OK, st
    seg, t_end = literal(knots, delT)
    n = len(seg)
    assert n_total == n + 1
    K = len(knots) - 1
    lead = int(first[0]) if K else n
    assert np.all(seg[:lead] == -1)
    covered = lead
    for i in range(K):
        if length[i]:
            assert np.all(seg[first[i]:first[i] + length[i]] == i), (i, first[i], length[i])
            assert first[i] == covered
        covered += int(length[i])
    assert covered == n
    # the endpoint's clock is the loop's value after the last step
    assert t_end >= knots[-1]
    return seg, t_end


def test_samples_on_knots_and_endpoint_exactly_on_the_last_knot():
    # delT = 0.25 with quarter-second knots: every knot is hit exactly, an inner one belongs to the earlier segment
    seg, t_end = check([0.0, 0.5, 1.25, 2.0], 0.25)
    assert list(seg) == [0, 0, 0, 1, 1, 1, 2, 2]
    assert t_end == 2.0


def test_endpoint_clock_beyond_the_last_knot():
    seg, t_end = check([0.0, 0.6, 1.3], 0.25)
    assert t_end > 1.3


def test_zero_length_segments_first_inner_last():
    check([0.0, 0.0, 0.5, 1.0], 0.25)            # first: takes the sample at 0 exactly
    check([0.0, 0.5, 0.5, 1.0], 0.25)            # inner: takes nothing
    check([0.0, 0.5, 1.0, 1.0], 0.25)            # last
    check([0.0, 0.5, 1.0, 1.0], 0.3)
    check([0.3, 0.3, 0.3, 0.9], 0.1)
    st, first, length, n_total = runs([0.0, 0.0], 0.1)   # k[K] = 0: no sample, only the endpoint
    assert st == OK and n_total == 1 and list(length) == [0]


def test_first_knot_after_zero():
    seg, _ = check([0.35, 1.0, 2.2], 0.1)
    assert seg[0] == -1 and (seg == -1).sum() == 4
    check([5.0, 6.0], 0.5)
    check([-1.0, 0.5, 2.0], 0.1)                 # k[0] < 0: sample 0 in segment 0 at local time 1
    st, first, length, n_total = runs([0.5], 0.1)        # no segment at all: every sample is the default pose
    assert st == OK and n_total == len(literal([0.5], 0.1)[0]) + 1


def test_long_trajectory_where_the_clock_drifts_from_j_delT():
    knots = [0.0, 700.0, 1500.1, 2222.2, 3000.0]
    seg, t_end = check(knots, 0.1)
    n = len(seg)
    t = 0.0                                      # the accumulated clock really is not j * delT here
    drift = 0.0
    for j in range(n):
        drift = max(drift, abs(t - j * 0.1))
        t += 0.1
    assert drift > 1e-9


@pytest.mark.parametrize("seed", range(12))
def test_seeded_random_knot_vectors(seed):
    rng = np.random.default_rng(seed)
    K = int(rng.integers(1, 9))
    d = float(rng.choice([0.1, 0.05, 0.25, rng.uniform(0.01, 0.3)]))
    steps = rng.uniform(0.0, 2.0, size=K)
    steps[rng.random(K) < 0.2] = 0.0
    if rng.random() < 0.5:                       # knots on the sample grid of d
        steps = np.round(steps / d) * d
    k0 = float(rng.choice([0.0, rng.uniform(0.0, 1.0), -rng.uniform(0.0, 1.0)]))
    knots = np.concatenate([[k0], k0 + np.cumsum(steps)])
    check(knots, d)


def test_rejections():
    assert runs([0.0, float("nan"), 1.0], 0.1)[0] == BAD_KNOTS
    assert runs([0.0, float("inf")], 0.1)[0] == BAD_KNOTS
    assert runs([0.0, 1.0, 0.5], 0.1)[0] == BAD_KNOTS
    for d in (0.0, -0.1, float("nan"), float("inf")):
        assert runs([0.0, 1.0], d)[0] == BAD_DELT, d
    assert runs([0.0, 1.0], 1e-300)[0] == STALL                  # the reference's loop never ends
    assert runs([0.0, 2.0 ** 40], 2.0 ** -14)[0] == STALL         # stalls at 2^39: delT is half an ulp there
    assert runs([0.0, 2.0 ** 20], 2.0 ** -11)[0] == TOO_LONG      # 2^31 samples
    st, first, length, n_total = runs([0.0, 2.0 ** 20], 2.0 ** -10)   # 2^30: fine
    assert st == OK and n_total == 2 ** 30 + 1 and first[0] == 0 and length[0] == 2 ** 30
    # not a stall: the clock's last step below k[K] still advances
    st, _, _, n_total = runs([0.0, 1.0], 2.0 ** -30)
    assert st == OK and n_total == 2 ** 30 + 1
