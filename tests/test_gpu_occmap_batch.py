"""-m gpu: polyTrajOccMap::makePlanBatch (device QP, whole trajectories checked by vigo_traj_point_check) against each
planner's twin planned alone with makePlan (host QP, host sampling, the map's own lookups), through
vigo_host_occ_plan_batch: seeded pillar worlds with inflated-and-unknown regions and waypoints on the map's edge, both
corridorConstraint modes, soft constraints, path shapes the device QP refuses, non-zero end conditions.  Verdicts and
iteration counts exactly, trajectories to 1e-9; every sample of a valid corridor plan re-checked with numpy.  Then
bspline_node's seed chain (vigo_host_occ_seed_chain) for 64 start/goal pairs against its solo twin."""
import ctypes as C
import os

import numpy as np
import pytest

from test_occmap_planner import CAP, cfg_vec, lookup_collides

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
ORIGIN = np.array([-3.0, -3.0, 0.0])
RES = 0.1


def pillar_world(seed):
    """60 x 60 x 20 voxels of 0.1 m from (-3, -3, 0) (the origin test_occmap_planner's lookup uses): pillars that are
    inflated-occupied, some of them unknown as well, unknown blocks"""
    rng = np.random.default_rng(seed)
    vox = np.zeros((60, 60, 20), np.uint8)
    for _ in range(25):
        c = rng.integers(3, 57, size=2)
        s = rng.integers(1, 4, size=2)
        vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], :] |= int(rng.choice([1, 3, 3]))
    for _ in range(6):
        c = rng.integers(5, 55, size=3)
        vox[c[0] - 4:c[0] + 4, c[1] - 4:c[1] + 4, max(c[2] % 20 - 4, 0):c[2] % 20 + 4] |= 2
    return vox


def plan_batch(vox, paths, cfgs, conds=None, corridor=1):
    L = C.CDLL(LIB)
    L.vigo_host_occ_plan_batch.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _ip, _dp, _dp, _dp,
                                           C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp]
    Pn = len(paths)
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
    wp = np.ascontiguousarray(np.concatenate(paths), dtype=np.float64)
    cf = np.ascontiguousarray(cfgs, dtype=np.float64)
    cd = None if conds is None else np.ascontiguousarray(conds, dtype=np.float64)
    v = np.ascontiguousarray(vox)
    tr, info, str_, sinfo, secs = np.zeros((Pn, CAP, 3)), np.zeros((Pn, 5)), np.zeros((Pn, CAP, 3)), np.zeros((Pn, 5)), np.zeros(2)
    D = lambda a: a.ctypes.data_as(_dp)
    rc = L.vigo_host_occ_plan_batch(*v.shape, D(ORIGIN), RES, v.ctypes.data_as(C.c_void_p), Pn, off.ctypes.data_as(_ip), D(wp),
                                    D(cf), None if cd is None else D(cd), corridor, CAP, D(tr), D(info), D(str_), D(sinfo), D(secs))
    assert rc == 0
    return tr, info, str_, sinfo


def assert_batch_equals_solo(vox, paths, tr, info, str_, sinfo, corridor):
    for i in range(len(paths)):
        assert np.array_equal(info[i, :3], sinfo[i, :3]), (i, info[i], sinfo[i])     # verdict, iterations, samples
        n = int(info[i, 2])
        np.testing.assert_allclose(tr[i, :n], str_[i, :n], rtol=0, atol=1e-9, err_msg=str(i))
        assert info[i, 3] == sinfo[i, 3]
        if corridor and info[i, 0]:
            assert not any(lookup_collides(vox, p) for p in tr[i, :n]), i   # the numpy re-check of a valid plan


def random_paths(rng, P, wmin=2, wmax=6):
    paths = []
    for i in range(P):
        W = int(rng.integers(wmin, wmax + 1))
        p = np.column_stack([np.linspace(-2.6, 2.6, W) * rng.choice([-1, 1]), rng.uniform(-2.6, 2.6, W), rng.uniform(0.4, 1.6, W)])
        if i % 5 == 0:
            p[-1, 0] = 2.98 * np.sign(p[-1, 0])                   # on the map's edge
        paths.append(p)
    return paths


@pytest.mark.parametrize("corridor", [1, 0])
def test_batch_equals_solo_on_pillar_worlds(corridor, capfd):
    rng = np.random.default_rng(40 + corridor)
    seen = set()
    for seed in (1, 2):
        vox = pillar_world(seed)
        paths = random_paths(rng, 24)
        cfgs = [cfg_vec(maximum_iteration_num=int(rng.integers(2, 10)), shrinking_factor=0.75) for _ in paths]
        conds = rng.uniform(-0.4, 0.4, size=(len(paths), 4, 3))
        conds[::3] = 0.0
        tr, info, str_, sinfo = plan_batch(vox, paths, cfgs, conds, corridor)
        assert_batch_equals_solo(vox, paths, tr, info, str_, sinfo, corridor)
        seen |= {(bool(a), int(b) > 1) for a, b in info[:, :2]}
    assert "no device for the batch" not in capfd.readouterr().out   # the device path ran
    if corridor:
        assert (True, False) in seen and (True, True) in seen and any(not v for v, _ in seen)
    else:
        assert seen == {(True, False)}


def test_soft_constraints_refused_shapes_and_mixed_degrees(capfd):
    rng = np.random.default_rng(77)
    vox = pillar_world(3)
    paths = random_paths(rng, 16)
    paths[3] = np.column_stack([np.linspace(-2.6, 2.6, 12), np.sin(np.linspace(0, 3, 12)), np.full(12, 1.0)])   # 12 waypoints
    paths[7] = np.column_stack([np.linspace(-2.6, 2.6, 11), np.cos(np.linspace(0, 3, 11)), np.full(11, 1.2)])
    cfgs = [cfg_vec(maximum_iteration_num=6) for _ in paths]
    for i in (1, 5, 9):
        cfgs[i] = cfg_vec(maximum_iteration_num=6, soft_constraint=1)           # host QP inside the batch
    cfgs[7] = cfg_vec(maximum_iteration_num=6, continuity_degree=2)              # refused by vigo_minsnap_supported
    cfgs[10] = cfg_vec(maximum_iteration_num=6, differential_degree=3, continuity_degree=3)   # a group of its own
    cfgs[11] = cfg_vec(maximum_iteration_num=6, use_pwl_failsafe=1)
    conds = rng.uniform(-0.3, 0.3, size=(len(paths), 4, 3))
    for corridor in (1, 0):
        tr, info, str_, sinfo = plan_batch(vox, paths, cfgs, conds, corridor)
        assert_batch_equals_solo(vox, paths, tr, info, str_, sinfo, corridor)
    assert "no device for the batch" not in capfd.readouterr().out


def test_seed_chain_batch_equals_solo(capfd):
    L = C.CDLL(LIB)
    L.vigo_host_occ_seed_chain.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_double, C.c_void_p, C.c_int, _dp, _dp, _dp, C.c_int,
                                           C.c_int, _dp, _ip, _dp, _ip]
    rng = np.random.default_rng(8)
    Pn, cap = 64, 512
    vox = np.zeros((60, 60, 20), np.uint8)                       # open world
    se = np.concatenate([rng.uniform([-2.5, -2.5, 0.8], [-1.0, 2.5, 1.4], size=(Pn, 1, 3)),
                         rng.uniform([1.0, -2.5, 0.8], [2.5, 2.5, 1.4], size=(Pn, 1, 3))], 1)
    pc = cfg_vec(desired_velocity=1.0, desired_acceleration=1.0)
    bc = np.array([0.5, 0.0, 2.0, 2.0, 2.0, 2.0])
    D = lambda a: a.ctypes.data_as(_dp)
    out = []
    for solo in (0, 1):
        seeds, n, dt, st = np.zeros((Pn, cap, 3)), np.zeros(Pn, np.int32), np.zeros(Pn), np.zeros(Pn, np.int32)
        rc = L.vigo_host_occ_seed_chain(*vox.shape, D(ORIGIN), RES, vox.ctypes.data_as(C.c_void_p), Pn, D(np.ascontiguousarray(se)),
                                        D(pc), D(bc), solo, cap, D(seeds), n.ctypes.data_as(_ip), D(dt), st.ctypes.data_as(_ip))
        assert rc == 0
        out.append((seeds, n, dt, st))
    assert "no device for the batch" not in capfd.readouterr().out
    (sb, nb, db, stb), (ss, ns, ds, sts) = out
    assert np.array_equal(nb, ns) and np.array_equal(db, ds)
    assert (nb > 1).all() and (nb <= cap).all()
    for i in range(Pn):
        np.testing.assert_allclose(sb[i, :nb[i]], ss[i, :ns[i]], rtol=0, atol=1e-9, err_msg=str(i))
    assert (stb >= 1).all() and (sts >= 1).all()                 # every seed accepted by updatePath: every plan made
    assert np.array_equal(stb, sts)
