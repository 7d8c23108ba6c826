"""-m gpu: bsplineTraj::seedPathBatch through vigo_host_seed_batch (host/src/cabi_host.cpp) — polyTrajOccMap::makePlanBatch,
the seed-path stage, bsplineTraj::makePlanBatch for 64 start/goal pairs of each workload — with setDeviceSeed on and off,
and a mixed batch against the planners run one after another in the reference's order.

Tolerances.  The launch takes the correctly rounded power where the host steps take libm's, which is the same value or
its neighbour: a seed pose, the sample at one t_j of the last try's clock, moves by at most 16 * 2^-52 * sum_d |c_d| t_j^d
per coordinate (tests/test_seed_core.py) — evaluated per pose at its own t_j, on the polynomial the harness returns for
that planner (the one both runs sampled; the host run's poses are its samples bit for bit, which is how each pose finds
its t_j).  The control points are a linear least-squares fit of the seed's points; tests/test_gpu_fit.py holds the fit
to 1e-10 relative to the largest control point, four orders above the seeds' bound, so the same figure holds here."""
import ctypes as C

import numpy as np
import pytest

import seed_cases as sc

pytestmark = pytest.mark.gpu
_dp, _ip = sc._dp, sc._ip
SEED_CAP, CTRL_CAP, SEG_CAP = 256, 260, 4
FIT_TOL = 1e-10


def seed_batch(world, pairs, max_len, kind=None, prev0=0.0, device=1, serial=0, max_tries=16):
    L = C.CDLL(sc.HOST_LIB)
    L.vigo_host_seed_batch.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _dp, _dp, _dp, _dp, _ip, C.c_double,
                                       C.c_int, C.c_int, C.c_int, C.c_int, _dp, _ip, _dp, _ip, _ip, C.c_int, _dp, _ip, C.POINTER(C.c_longlong), C.c_int, _ip, _dp, _dp, _dp]
    Pn = len(pairs)
    vox = np.ascontiguousarray(world.vox)
    se = np.ascontiguousarray(pairs, dtype=np.float64)
    ml = np.ascontiguousarray(np.broadcast_to(np.asarray(max_len, float), (Pn,)))
    kd = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    r = dict(seed=np.zeros((Pn, SEED_CAP, 3)), seed_n=np.zeros(Pn, np.int32), dt=np.zeros(Pn), tries=np.zeros(Pn, np.int32),
             status=np.zeros(Pn, np.int32), ctrl=np.zeros((Pn, CTRL_CAP, 3)), ctrl_n=np.zeros(Pn, np.int32), totals=np.zeros(2, np.int64),
             K=np.zeros(Pn, np.int32), knots=np.zeros((Pn, SEG_CAP + 1)), coeffs=np.zeros((Pn, SEG_CAP, 3, 8)), duration=np.zeros(Pn))
    D = lambda a: a.ctypes.data_as(_dp)
    I = lambda a: a.ctypes.data_as(_ip)
    rc = L.vigo_host_seed_batch(*vox.shape, D(np.ascontiguousarray(world.origin)), float(world.res), vox.ctypes.data_as(C.c_void_p), Pn, D(se),
                                D(sc.poly_cfg()), D(sc.BSP_CFG), D(ml), None if kd is None else I(kd), float(prev0), device, serial, max_tries,
                                SEED_CAP, D(r["seed"]), I(r["seed_n"]), D(r["dt"]), I(r["tries"]), I(r["status"]), CTRL_CAP, D(r["ctrl"]),
                                I(r["ctrl_n"]), r["totals"].ctypes.data_as(C.POINTER(C.c_longlong)), SEG_CAP, I(r["K"]), D(r["knots"]),
                                D(r["coeffs"]), D(r["duration"]))
    assert rc == 0
    r["polys"] = [sc.Traj(f"planner_{i}", r["knots"][i, :r["K"][i] + 1].copy(), r["coeffs"][i, :r["K"][i]].copy(), float(r["duration"][i]))
                  for i in range(Pn)]
    assert (r["seed_n"] <= SEED_CAP).all() and (r["ctrl_n"] <= CTRL_CAP).all()
    return r


def assert_same_seeds(a, b, i):
    """planner i's search in run a against run b, the host's (libm): counts, tries and dt equal, every pose within its own bound"""
    assert a["seed_n"][i] == b["seed_n"][i] and a["tries"][i] == b["tries"][i] and a["dt"][i] == b["dt"][i], i
    c, n = b["polys"][i], b["seed_n"][i]
    assert np.array_equal(c.knots, a["polys"][i].knots) and np.array_equal(c.coeffs, a["polys"][i].coeffs), i   # one polynomial
    bound = sc.point_bounds(c, float(b["dt"][i]), b["seed"][i, :n])
    assert (np.abs(a["seed"][i, :n] - b["seed"][i, :n]) <= bound).all(), i


def assert_same_plans(a, b, who=None):
    who = range(len(a["seed_n"])) if who is None else who
    for i in who:
        assert_same_seeds(a, b, i)
        assert a["status"][i] == b["status"][i] and a["ctrl_n"][i] == b["ctrl_n"][i], (i, a["status"][i], b["status"][i])
        m = a["ctrl_n"][i]
        assert np.abs(a["ctrl"][i, :m] - b["ctrl"][i, :m]).max(initial=0.0) <= FIT_TOL * max(1.0, np.abs(b["ctrl"][i, :m]).max(initial=0.0)), i


@pytest.mark.parametrize("which", ["open", "pillar"])
def test_device_seed_equals_host_seed(which, capfd):
    world, pairs = sc.workload_world(which), sc.workload_pairs(which)
    on = seed_batch(world, pairs, 1000.0, device=1)
    off = seed_batch(world, pairs, 1000.0, device=0)
    assert "vigo_seed_paths failed" not in capfd.readouterr().out
    assert on["totals"][0] >= 60 and off["totals"][0] == 0 and off["totals"][1] == 64
    assert_same_plans(on, off)
    assert (on["status"] >= 1).sum() >= 48 and (on["tries"] > 1).any()
    if which == "open":
        assert (on["status"] >= 1).all()


def test_mixed_batch_equals_the_planners_one_after_another(capfd):
    world = sc.open_world()
    world.vox[30, 30, 0] |= 1                                   # the default pose (0, 0, 0), the PWL planner's goal: refused
    pairs = sc.workload_pairs("open")[:24]
    kind = np.zeros(24, np.int32)
    kind[5] = 1                                                  # a bsplineTraj without a device: no snapshot
    kind[9] = 2                                                  # a polyTrajOccMap flying its PWL fallback
    max_len = np.full(24, 1000.0)
    max_len[[3, 4, 12, 17]] = 1.5                                # the length handed down (4 m and more) exceeds these
    serial = seed_batch(world, pairs, max_len, kind, prev0=2.5, serial=1)
    others = [i for i in range(24) if i != 5]
    for device in (1, 0):
        batch = seed_batch(world, pairs, max_len, kind, prev0=2.5, device=device)
        assert_same_plans(batch, serial, others)
        # the planner without a device gets its seed from the host steps; a batch cannot fit it (the fit is the device's,
        # on a handle of its own target), where alone it is fitted on the host and then fails to plan
        assert_same_seeds(batch, serial, 5)
        assert batch["status"][5] == 0 and serial["status"][5] == 1
        assert batch["status"][9] == 0 and batch["seed_n"][9] == 2
        if device:
            assert 1 <= batch["totals"][0] <= 18 and batch["totals"][1] >= 6     # redone, without device, PWL: the host's
        else:
            assert batch["totals"][0] == 0
    # the handed-down length did enter: alone, from a previous length of 0, pair 3 is cut at its own 1.5 m
    alone = seed_batch(world, pairs[3:4], 1.5, prev0=0.0, device=1)
    assert alone["seed_n"][0] < serial["seed_n"][3]
