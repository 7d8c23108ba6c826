"""-m gpu: vigo_traj_point_check (whole trajectories, polyTrajOccMap's point test) against a Python restatement of its
rules 1-3, 4' and 5 (include/vigo.h) over the oracle's own sampler (vgo_poly_pos, correctly rounded pow) and lookups
(vgo_is_inflated_occupied && vgo_is_unknown), integer for integer; status and n against vigo_traj_corridor_check on the
same inputs; on vigo_minsnap output straight from device memory; on more trajectories than one chunk; and on hostile
arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as ol
import test_gpu_traj_corridor as tc
from gpu_util import to_dev
from trajectory_planner_amd import synth
from trajectory_planner_amd._lib import load

pytestmark = pytest.mark.gpu
KEYS = ("status", "n", "flag", "first", "count", "seg")


def bits_world(seed=7, n=96, res=0.1):
    """96 x 96 x 40 voxels from (-4.8, -4.8, -0.5): pillars with bit 0 only, bit 1 only or both, unknown blocks (bit 1)
    and a few occupied-only columns (bit 2, which the point test ignores)"""
    rng = np.random.default_rng(seed)
    vox = np.zeros((n, n, 40), dtype=np.uint8)
    for _ in range(90):
        c = rng.integers(4, n - 4, size=2)
        s = rng.integers(1, 5, size=2)
        vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], 0:rng.integers(10, 40)] |= int(rng.choice([1, 2, 3, 4]))
    unk = rng.random((n // 8, n // 8, 5)) < 0.1
    vox[np.repeat(np.repeat(np.repeat(unk, 8, 0), 8, 1), 8, 2)] |= 2
    return synth.World(vox, np.array([-4.8, -4.8, -0.5]), res, np.zeros((0, 6)))


def restate(g, seg_off, coeffs, knots, delT, endpoint):
    """rules 1-3 and 5 as tc.restate, rule 4': isInflatedOccupied(p) && isUnknown(p) on the fp64 pose"""
    O = ol.oracle()
    T = len(seg_off) - 1
    S, _, d1 = coeffs.shape
    deg = d1 - 1
    out = dict(status=np.zeros(T, np.int32), n=np.zeros(T, np.int32), flag=np.zeros(T, np.uint8),
               first=np.full(T, -1, np.int32), count=np.zeros(T, np.int32), seg=np.zeros(S, np.uint8))
    p = np.zeros(3)
    q = np.zeros(3)
    with ol.pow_mode(True):
        for t in range(T):
            a, b = int(seg_off[t]), int(seg_off[t + 1])
            K = b - a
            k = [float(x) for x in knots[a + t:a + t + K + 1]]
            d = float(delT[t])
            st = tc.runs_status(k, d)
            out["status"][t] = st
            if st:
                continue
            poses, segs = [], []
            tt = 0.0
            while tt < k[-1]:                                  # rule 1
                s = next((i for i in range(K) if k[i] <= tt <= k[i + 1]), -1)   # rule 2
                if s < 0:
                    poses.append((0.0, 0.0, 0.0))
                else:
                    c = np.ascontiguousarray(coeffs[a + s])
                    O.vgo_poly_pos(deg, ol._d(c[0]), ol._d(c[1]), ol._d(c[2]), tt - k[s], ol._d(p))
                    poses.append(tuple(p))
                segs.append(s)
                tt += d
            poses.append(tuple(float(x) for x in endpoint[t]))   # rule 3
            segs.append(next((i for i in range(K) if k[i] <= tt <= k[i + 1]), -1))
            first, count = -1, 0
            for j, (pose, s) in enumerate(zip(poses, segs)):
                q[:] = pose
                if O.vgo_is_inflated_occupied(C.byref(g), ol._d(q)) and O.vgo_is_unknown(C.byref(g), ol._d(q)):   # rule 4'
                    count += 1
                    first = j if first < 0 else first
                    if s >= 0:
                        out["seg"][a + s] = 1                  # rule 5
            out["n"][t] = len(poses)
            out["flag"][t] = count > 0
            out["first"][t] = first
            out["count"][t] = count
    return out


def device(v, seg_off, coeffs, knots, delT, endpoint):
    r = v.traj_point_check(to_dev(seg_off, v.device), to_dev(coeffs, v.device), to_dev(knots, v.device),
                           to_dev(delT, v.device), to_dev(endpoint, v.device))
    return dict(zip(KEYS, (x.cpu().numpy() for x in r)))


def assert_same(got, ref, ctx=""):
    for key in KEYS:
        assert np.array_equal(got[key], ref[key]), (ctx, key, np.nonzero(got[key] != ref[key])[0][:10], got[key][:16], ref[key][:16])


def set_world(v, w):
    v.set_grid(to_dev(w.voxels, v.device), w.origin, w.res)
    return ol.make_grid(w)


@pytest.mark.parametrize("deg", [3, 5, 7])
def test_seeded_worlds_match_the_restatement(vigo_handle, deg):
    v = vigo_handle
    w = bits_world(20 + deg)
    g, keep = set_world(v, w)
    args = tc.pack(tc.random_trajs(200 + deg, 32, deg, 60))
    got = device(v, *args)
    assert_same(got, restate(g, *args), deg)
    assert 0 < got["flag"].mean() < 1                           # colliding and clean trajectories both occur
    assert got["seg"].sum() > 0                                  # ... and blamed segments
    # the pillars of one bit alone are there, and the trajectories cross them without colliding
    seg_off, coeffs, knots, delT, endpoint = args
    crossed = False
    for t in range(len(delT)):
        a, b = seg_off[t], seg_off[t + 1]
        for s in range(a, b):
            k0, k1 = knots[s + t], knots[s + t + 1]
            pts = np.zeros((8, 3))
            with ol.pow_mode(True):
                for i, tt in enumerate(np.linspace(0, k1 - k0, 8)):
                    c = np.ascontiguousarray(coeffs[s])
                    r = np.zeros(3)
                    ol.oracle().vgo_poly_pos(deg, ol._d(c[0]), ol._d(c[1]), ol._d(c[2]), float(tt), ol._d(r))
                    pts[i] = r
            idx = np.floor((pts - w.origin) / w.res).astype(np.int64)
            inside = ((idx >= 0) & (idx < w.voxels.shape)).all(1)
            bits = w.voxels[tuple(idx[inside].T)] & 3
            crossed |= bool(((bits == 1) | (bits == 2)).any())
    assert crossed


def test_edge_cases_match_the_restatement(vigo_handle):
    v = vigo_handle
    w = bits_world(11)
    g, keep = set_world(v, w)
    args = tc.pack(tc.edge_trajs())
    got = device(v, *args)
    assert_same(got, restate(g, *args))
    assert list(got["status"][17:23]) == [1, 1, 2, 2, 2, 3]
    # NaN / infinite poses and endpoints lie outside the grid: they collide
    assert got["flag"][10] == 1 and got["flag"][14] == 1 and got["flag"][15] == 1
    # the default pose collides in another world: the leading run is counted whole, blames nothing
    vox = w.voxels.copy()
    vox[46:50, 46:50, 3:7] |= 3                                   # around (0, 0, 0)
    w2 = synth.World(vox, w.origin, w.res, w.boxes)
    g2, keep2 = set_world(v, w2)
    got2 = device(v, *args)
    assert_same(got2, restate(g2, *args), "default pose")
    assert got2["first"][5] == 0 and got2["flag"][5] == 1


def test_status_and_n_equal_the_corridor_check(vigo_handle):
    v = vigo_handle
    w = tc.small_world(11)
    set_world(v, w)
    args = tc.pack(tc.edge_trajs() + tc.random_trajs(9, 16, 7, 40))
    got = device(v, *args)
    ref = tc.device(v, *args, False)
    for key in ("status", "n"):
        assert np.array_equal(got[key], ref[key]), key


def test_minsnap_output_straight_from_device_memory(vigo_handle):
    v = vigo_handle
    w, wp0 = tc.maze()
    g, keep = set_world(v, w)
    rng = np.random.default_rng(9)
    T, W = 12, 8
    wp = np.repeat(wp0[None], T, 0) + np.concatenate([np.zeros((1, W, 3)), rng.normal(0, 0.3, size=(T - 1, W, 3))])
    coeffs, knots, status = v.minsnap(to_dev(wp, v.device), to_dev(np.full((T, W - 1), 0.5), v.device))
    seg_off = to_dev((np.arange(T + 1) * (W - 1)).astype(np.int32), v.device)
    delT = to_dev(np.full(T, 0.1), v.device)
    endpoint = to_dev(wp[:, -1], v.device)
    r = v.traj_point_check(seg_off, coeffs.reshape(-1, 3, 8), knots.reshape(-1), delT, endpoint)
    got = dict(zip(KEYS, (x.cpu().numpy() for x in r)))
    args = (seg_off.cpu().numpy(), coeffs.reshape(-1, 3, 8).cpu().numpy(), knots.reshape(-1).cpu().numpy(),
            delT.cpu().numpy(), wp[:, -1])
    assert_same(got, restate(g, *args))
    assert (got["status"] == 0).all()


def test_more_trajectories_than_one_chunk(vigo_handle):
    v = vigo_handle
    w = bits_world(13)
    g, keep = set_world(v, w)
    rng = np.random.default_rng(17)
    trajs = []
    for t in range(4100):
        K = int(rng.integers(1, 3))
        c = rng.uniform(-0.3, 0.3, size=(K, 3, 8)) * 0.1
        c[:, :, 0] = rng.uniform([-3, -3, 0.7], [3, 3, 1.5], size=(K, 3))
        c[:, :, 1] = rng.uniform(-1, 1, size=(K, 3))
        knots = np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.4, size=K))])
        trajs.append((knots, c, 0.05, rng.uniform([-3, -3, 0.7], [3, 3, 1.5])))
    args = tc.pack(trajs)
    got = device(v, *args)
    assert (got["status"] == 0).all() and 0 < got["flag"].mean() < 1
    pick = sorted(set(rng.choice(4100, 40, replace=False).tolist()) | {4094, 4095, 4096, 4097, 4099})
    seg_off, coeffs, knots, delT, endpoint = args
    for t in pick:
        a, b = seg_off[t], seg_off[t + 1]
        sub = (np.array([0, b - a], np.int32), coeffs[a:b], knots[a + t:b + t + 1], delT[t:t + 1], endpoint[t:t + 1])
        ref = restate(g, *sub)
        for key in ("status", "n", "flag", "first", "count"):
            assert got[key][t] == ref[key][0], (t, key)
        assert np.array_equal(got["seg"][a:b], ref["seg"]), t
    cut = 2050
    r1, r2 = device(v, *tc.pack(trajs[:cut])), device(v, *tc.pack(trajs[cut:]))
    for key in KEYS:
        assert np.array_equal(got[key], np.concatenate([r1[key], r2[key]])), key


def test_hostile_arguments(vigo_handle):
    v = vigo_handle
    lib = load()
    h = v._h
    d = v.device
    seg_off, coeffs, knots, delT, endpoint = (to_dev(a, d) for a in tc.pack(tc.edge_trajs()[:3]))
    T, S = 3, coeffs.shape[0]
    outs = [torch.zeros(T, dtype=torch.int32, device=d), torch.zeros(T, dtype=torch.int32, device=d),
            torch.zeros(T, dtype=torch.uint8, device=d), torch.zeros(T, dtype=torch.int32, device=d),
            torch.zeros(T, dtype=torch.int32, device=d), torch.zeros(S, dtype=torch.uint8, device=d)]
    P = lambda x: C.c_void_p(x.data_ptr())

    def call(h=h, T=T, S=S, deg=7, so=seg_off, outp=None, co=coeffs):
        o = [P(x) for x in outs] if outp is None else outp
        return lib.vigo_traj_point_check(h, T, S, deg, P(so) if so is not None else None, P(co) if co is not None else None,
                                         P(knots), P(delT), P(endpoint), *o)
    assert call() == -5                                          # before a grid
    w = bits_world()
    v.set_grid(to_dev(w.voxels, d), w.origin + 0.037, w.res)    # an origin off the key lattice is fine here
    assert call() == 0
    assert call(h=None) == -1
    assert call(T=-1) == -1 and call(S=-1) == -1
    assert call(deg=16) == -1 and call(deg=-1) == -1
    assert call(so=None) == -1 and call(co=None) == -1
    for i in range(6):
        o = [P(x) for x in outs]
        o[i] = None
        assert call(outp=o) == (0 if i == 4 else -1), i            # only out_count may be NULL
    for bad in ([0, 3, 2, 9], [-1, 3, 6, 9], [0, 3, 6, 10 ** 6], [0, 6, 3, 9]):
        so = to_dev(np.array(bad, np.int32), d)
        assert call(so=so) == 0
        torch.cuda.synchronize()
        assert outs[0].cpu().tolist() == [5, 5, 5] and outs[2].sum() == 0 and outs[5].sum() == 0
    with pytest.raises(ValueError):
        v.traj_point_check(seg_off, coeffs, knots[:-1], delT, endpoint)
    with pytest.raises(ValueError):
        v.traj_point_check(seg_off, coeffs, knots, delT, endpoint[:-1])
    st, n, flag, first, count, seg = v.traj_point_check(seg_off[:1], coeffs, knots[:S], delT[:0], endpoint[:0])
    assert seg.sum() == 0
    assert call(T=0, S=0, so=seg_off, outp=[None] * 6, co=None) == 0
