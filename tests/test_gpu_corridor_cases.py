"""-m gpu: the adversarial case set of tests/corridor_cases.py on the device, integer for integer against the oracle —
vigo_corridor_check (flag, first, count of every segment of every case against vgo_corridor_check_batch with the exact
power), vigo_box_collision_points (random poses and poses on voxel faces, metric bounds and the grid's rim +- one float
ulp, for every box / map_resolution of the case set) and vigo_traj_corridor_check (all six outputs against the Python
restatement of its rules, nonfinite_collides off and on).  Which route of k_corridor each segment takes is predicted on
the CPU (tests/test_corridor_cases.py holds the census and its minima); a mismatch names the case, the segment, its
family and that route."""
import ctypes as C

import numpy as np
import pytest

import corridor_cases as cc
import oracle_lib as ol
from gpu_util import to_dev
from test_corridor_cases import oracle_grid, trajectory_runs
from corridor_restatement import segment_route
from traj_corridor_util import pack, restate

pytestmark = pytest.mark.gpu

_cases = {c.name: c for c in cc.segment_cases()}
_groups = sorted({c.group for c in _cases.values()})
_traj_cases = {t.name: t for t in cc.traj_cases()}
_oracle = {}


def set_world(v, world, bounds):
    v.set_grid(to_dev(world.voxels, v.device), world.origin, world.res)
    if bounds is not None:
        v.set_metric_bounds(*bounds)
    return oracle_grid(world, bounds)


def oracle_results(c, g):
    """flag, first, count of the oracle's per-sample walk (exact power), once per case"""
    if c.name not in _oracle:
        with ol.pow_mode(True):
            _oracle[c.name] = ol.corridor_check_batch(g, c.coeffs, c.n_samp, c.delT, np.array(c.box), c.map_res)
    return _oracle[c.name]


@pytest.mark.parametrize("group", _groups)
def test_segment_mode_matches_the_oracle(vigo_handle, group):
    v = vigo_handle
    flags = []
    for c in (c for c in _cases.values() if c.group == group):
        g, keep = set_world(v, c.world, c.bounds)
        args = (to_dev(c.coeffs, v.device), to_dev(c.n_samp, v.device), to_dev(c.delT, v.device), c.box, c.map_res)
        got = [x.cpu().numpy() for x in v.corridor_check(*args)]
        again = [x.cpu().numpy() for x in v.corridor_check(*args)]
        ref = oracle_results(c, g)
        bad = [s for s in range(len(c.n_samp)) if any(int(a[s]) != int(b[s]) for a, b in zip(got, ref))]
        msg = [dict(case=c.name, segment=s, family=c.tags[s], n=int(c.n_samp[s]),
                    route=segment_route(c.coeffs[s], int(c.n_samp[s]), float(c.delT[s]), c.box, c.map_res, c.world.grid)["route"],
                    device=[int(a[s]) for a in got], oracle=[int(b[s]) for b in ref]) for s in bad[:8]]
        assert not bad, msg
        for a, b in zip(got, again):
            assert np.array_equal(a, b), (c.name, "second call differs")
        flags.append(got[0])
    mean = np.concatenate(flags).mean()
    assert 0 < mean < 1, (group, mean)


def test_box_collision_points_on_faces_bounds_and_rim(vigo_handle):
    v = vigo_handle
    O = ol.oracle()
    W = cc.worlds()
    rng = np.random.default_rng(11)
    hits = []
    for bi, (bname, box, mres) in enumerate(cc.BOXES):
        for w in (W["ABCD"[bi % 4]], W["ABCD"[(bi + 2) % 4]]):
            g, keep = set_world(v, w, w.bounds)
            dims, origin, res = w.grid
            half = dims[0] * res / 2
            height = dims[2] * res
            # the fuzz tool's random poses (some outside the map) and the poses on faces, bounds and the rim
            pts = np.concatenate([rng.uniform(-half * 1.1, half * 1.1, size=(300, 3)) * [1, 1, 0.0] + origin * [0, 0, 1] +
                                  rng.uniform(-0.1, 1.1, size=(300, 1)) * [0, 0, height], cc.face_poses(w, box, mres, rng)])
            got = v.box_collision_points(to_dev(pts, v.device), box, mres).cpu().numpy()
            bx = np.ascontiguousarray(box, dtype=np.float64)
            ref = np.array([O.vgo_box_collision(C.byref(g), C.c_float(p[0]), C.c_float(p[1]), C.c_float(p[2]), ol._d(bx), C.c_double(mres))
                            for p in pts], dtype=np.uint8)
            bad = np.nonzero(got != ref)[0]
            assert len(bad) == 0, (bname, w.name, [(pts[i].tolist(), int(got[i]), int(ref[i])) for i in bad[:5]])
            hits.append(got)
    assert 0 < np.concatenate(hits).mean() < 1


def device_traj(v, args, box, map_res, nonfinite):
    seg_off, coeffs, knots, delT, endpoint = args
    r = v.traj_corridor_check(to_dev(seg_off, v.device), to_dev(coeffs, v.device), to_dev(knots, v.device), to_dev(delT, v.device),
                              to_dev(endpoint, v.device), box, map_res, nonfinite_collides=nonfinite)
    return dict(zip(("status", "n", "flag", "first", "count", "seg"), (x.cpu().numpy() for x in r)))


@pytest.mark.parametrize("name", sorted(_traj_cases))
def test_trajectory_mode_matches_the_restatement(vigo_handle, name):
    v = vigo_handle
    tc = _traj_cases[name]
    g, keep = set_world(v, tc.world, tc.bounds)
    args = pack(tc.trajs)
    refs = {}
    for nf in (False, True):
        got = device_traj(v, args, tc.box, tc.map_res, nf)
        ref = restate(g, *args, nf, box=np.array(tc.box), map_res=tc.map_res)
        for key in ("status", "n", "flag", "first", "count", "seg"):
            bad = np.nonzero(got[key] != ref[key])[0]
            if len(bad) and key != "seg":
                t = int(bad[0])
                knots, coeffs, delT, endpoint = tc.trajs[t]
                clock, runs = trajectory_runs(knots, delT)
                routes = [segment_route(coeffs[i], n, delT, tc.box, tc.map_res, tc.world.grid, traj=(knots[i], knots[i + 1]),
                                        table=len(clock) > 0)["route"] for i, (first, n) in enumerate(runs)]
                assert False, dict(case=name, nonfinite=nf, output=key, trajectory=t, runs=runs, routes=routes,
                                   device=int(got[key][t]), restatement=int(ref[key][t]))
            assert len(bad) == 0, dict(case=name, nonfinite=nf, output=key, segments=bad[:10].tolist())
        assert (got["status"] == 0).all()
        refs[nf] = ref
        again = device_traj(v, args, tc.box, tc.map_res, nf)
        for key in got:
            assert np.array_equal(got[key], again[key]), (name, key, "second call differs")
    if name.startswith("non-finite"):
        # nonfinite_collides is exercised: poses at NaN / infinity in fp64 collide with it and do not without it
        assert (refs[True]["count"] > refs[False]["count"]).sum() >= 4 and (refs[True]["seg"] != refs[False]["seg"]).any()
    if name.startswith("large knots"):
        # the default pose before k[0] is free, so the verdicts are those of the real samples; in world A the first
        # trajectory creeps across a wall's face by a few float spacings: a partial count, the hugger does flicker
        pre = np.array([int((trajectory_runs(k, d)[0] < k[0]).sum()) for k, c, d, e in tc.trajs])
        assert (refs[True]["first"][refs[True]["flag"] > 0] >= pre[refs[True]["flag"] > 0]).all()
        if " A " in name:
            real = refs[True]["n"][0] - pre[0]
            assert 0.05 * real < refs[True]["count"][0] < 0.95 * real, (int(refs[True]["count"][0]), int(real))

