"""The table of tests/test_gpu_stream_order.py (GPU) and tests/test_stream_cases.py (CPU): one row per handle entry point of
include/vigo.h that enqueues device work.

A row names the entry, holds the device arrays the call reads twice — `real`, and a `decoy` of the same shapes and dtypes that
is a VALID input giving another answer (the batch in reverse order with its CSR lists rebuilt, another permutation of the
counts, a second world of the same dimensions) — and a `call(v, t)` that makes the call on the handle v with the device
tensors t[name] and returns every output tensor, the arrays the call updates in place included.  Host scalars and small host
arrays (origin, box, pool, parameters) live in the closure.  Entries that read installed state install it inside `call`,
from a voxel / lattice tensor that is one of the row's delayed inputs.  `derive(v, t)` (optional) runs the producing stage of
an entry whose integer inputs are another stage's outputs: the GPU test runs it on the default stream on the real and on the
decoy inputs and adds what it returns to both.  `no_round_trip` is the column of the entries that reach neither read_back nor
a stream or event wait on a cold handle (csrc/vigo_api.cpp): the host returns from them while their inputs are still being
produced.  `twin(inputs)` (optional) is the same call by a host twin or the oracle on numpy arrays: the CPU test shows with it
that the decoy gives another answer before anything runs on a GPU."""
import functools
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from trajectory_planner_amd import synth

# handle entry points without a row, each with its reason
EXEMPT = {
    "vigo_destroy": "frees the handle; enqueues nothing",
    "vigo_set_stream": "binds the stream (waits for the old one); the rebind test of test_gpu_stream_order.py pins it",
    "vigo_set_params": "host checks and one stream-ordered copy of the constants; every row with params runs behind it",
    "vigo_get_params": "host state only",
    "vigo_set_precision": "host state only",
    "vigo_last_error": "host state only",
    "vigo_set_metric_bounds": "host state only (the grid view's bounds); the corridor rows call it",
}


@dataclass
class Row:
    name: str                                # the test id: the entry without its vigo_ prefix (+ a variant)
    entry: str                               # the vigo_* entry of include/vigo.h the row is for
    real: dict
    decoy: dict
    call: Callable                           # call(v, t) -> list of output tensors (or host integers)
    no_round_trip: bool                      # assertion (b): the host returns while the producer still runs
    params: Optional[Callable] = None        # params(P): the handle's parameters, set at creation
    derive: Optional[Callable] = None        # derive(v, t) -> dict of further device inputs
    twin: Optional[Callable] = None          # twin(inputs) -> list of numpy arrays
    notes: str = ""


def _c(a, dtype=None):
    return np.ascontiguousarray(a, dtype=dtype)


def second_world(vox, shift=7):
    """another occupancy on the same dimensions: the voxels moved `shift` cells along x and y (wrapping)"""
    return _c(np.roll(np.roll(vox, shift, axis=0), -shift, axis=1))


@functools.lru_cache(maxsize=None)
def small_worlds():
    """conftest's small_world, and a second world of its dimensions with other boxes"""
    return tuple(synth.make_box_world(synth.SEED_BASE + 2 + k, n=128, n_boxes=60, centre_range=5.5, z_range=2.0) for k in (0, 1))


# ---- solve batches --------------------------------------------------------------------------------------------------------
def batch_arrays(b, order=None, weights=None, n_pts=None, state=None):
    """the device arrays of a synth.Batch / PaddedBatch with its trajectories in `order`, every CSR list rebuilt"""
    B, Ns = b.ctrl.shape[:2]
    order = list(range(B)) if order is None else list(order)
    counts = np.diff(b.guide_off.astype(np.int64)).reshape(B, Ns)
    pv = [b.guide_pv[b.guide_off[r * Ns]:b.guide_off[(r + 1) * Ns]] for r in order]
    unk = [b.guide_unk[b.guide_off[r * Ns]:b.guide_off[(r + 1) * Ns]] for r in order]
    a = dict(ctrl=_c(b.ctrl[order]), guide_off=np.concatenate([[0], np.cumsum(counts[order].reshape(-1))]).astype(np.int32),
             guide_pv=_c(np.concatenate(pv).reshape(-1, 6)), guide_unk=_c(np.concatenate(unk), np.uint8))
    if b.obs is not None:
        obs = [b.obs[b.obs_off[r]:b.obs_off[r + 1]] for r in order]
        a["obs_off"] = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int32)
        a["obs"] = _c(np.concatenate(obs).reshape(-1, 9))
    if weights is not None:
        a["weights"] = _c(weights[order])
    if n_pts is not None:
        a["n_pts"] = _c(np.asarray(n_pts)[order], np.int32)
    if state is not None:
        a["state"] = _c(state[order], np.int32)
    return a


def _as_batch(a):
    return synth.Batch(a["ctrl"], a["guide_off"], a["guide_pv"], a["guide_unk"], a.get("obs_off"), a.get("obs"), a.get("weights"))


def _solve_params(P):
    P.max_iterations = 20


def _solve_out(r):
    return [r.ctrl, r.x, r.status, r.fx, r.iters, r.evals]


def _obs_kw(t):
    return dict(obs_off=t.get("obs_off"), obs=t.get("obs"), weights=t.get("weights"))


# ---- the rows ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows():
    """every row, built once and shared read-only"""
    import astar_cases as ac
    import corridor_cases as cc
    import esdf_update_cases as uc
    import finish_cases as fc
    import gate_cases as gates
    import grid_update_cases as gu
    import mixed_cases as mc
    import oracle_lib as ol
    import pathsearch_cases as pc
    import prologue_mixed_cases as pm
    import reguide_cases as rc
    import seed_cases as sc
    from traj_corridor_util import pack as pack_trajs

    out = []

    def add(name, real, decoy, call, no_round_trip, entry=None, **kw):
        assert set(real) == set(decoy), name
        for k in real:
            real[k], decoy[k] = _c(real[k]), _c(decoy[k])
            assert real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype, (name, k, real[k].shape, decoy[k].shape)
        out.append(Row(name, entry or "vigo_" + name, real, decoy, call, no_round_trip, **kw))

    rev = lambda a: _c(a[::-1])
    world, world2 = small_worlds()
    origin, res = tuple(float(x) for x in world.origin), float(world.res)
    P0 = ol.default_params()
    rng = np.random.default_rng(0x57AE)

    def lookups(vox, pts, bit):
        return synth.lookup(synth.World(vox, world.origin, world.res, None), pts, bit)

    # -- the map: pack, inflate, the setters, the region update, the lookups
    vox_pair = (dict(vox=world.voxels), dict(vox=world2.voxels))
    pts = rng.uniform(-6.6, 6.6, size=(257, 3))
    add("pack_grid", *vox_pair, lambda v, t: [v.pack_grid(t["vox"])], True)
    small = [(np.random.default_rng(s).random((8, 9, 40)) < 0.05).astype(np.uint8) * 4 for s in (8, 9)]
    add("inflate_grid", dict(vox=small[0]), dict(vox=small[1]), lambda v, t: [v.inflate_grid(t["vox"], 1, 2, 1)], True,
        twin=lambda a: [gu.inflated(a["vox"], (1, 2, 1))])

    def set_grid_call(v, t):
        v.set_grid(t["vox"], origin, res)
        return [v.query_points(t["pts"], 0), v.get_grid_packed()]
    add("set_grid", dict(vox=world.voxels, pts=pts), dict(vox=world2.voxels, pts=pts), set_grid_call, True,
        twin=lambda a: [lookups(a["vox"], a["pts"], 0)])

    def set_grid_packed_call(v, t):
        v.set_grid_packed(t["packed"], world.voxels.shape, origin, res)
        return [v.query_points(t["pts"], 0), v.query_points(t["pts"], 1)]
    add("set_grid_packed", dict(vox=world.voxels, pts=pts), dict(vox=world2.voxels, pts=pts), set_grid_packed_call, True,
        derive=lambda v, t: dict(packed=v.pack_grid(t["vox"])), notes="vox is read by derive only: the delayed input is `packed`")

    def set_grid_host_call(v, t):
        v.set_grid_host(world.voxels, origin, res)
        return [v.query_points(t["pts"], 0)]
    add("set_grid_host", dict(pts=pts), dict(pts=rev(pts)), set_grid_host_call, False,
        twin=lambda a: [lookups(world.voxels, a["pts"], 0)], notes="the voxels are host memory: staged, packed and waited for")

    lo, box_r = (20, 30, 40), (1, 1, 1)
    boxes = [(np.random.default_rng(s).random((24, 17, 37)) < 0.2).astype(np.uint8) * 4 for s in (3, 4)]

    def region_call(v, t):
        v.set_grid(t["vox"], origin, res)
        v.update_grid_region(lo, t["box"], box_r)
        return [v.get_grid_packed(), v.query_points(t["pts"], 0)]

    def region_twin(a, box=None):
        rc_, g = synth.host_grid_region_apply(a["vox"], lo, a["box"] if box is None else box, box_r)
        assert rc_ == 0
        return [g]
    add("update_grid_region", dict(vox=world.voxels, box=boxes[0], pts=pts), dict(vox=world2.voxels, box=boxes[1], pts=pts), region_call, True,
        twin=region_twin)

    def region_host_call(v, t):
        v.set_grid(t["vox"], origin, res)
        v.update_grid_region_host(lo, boxes[0], box_r)
        return [v.get_grid_packed()]
    add("update_grid_region_host", *vox_pair, region_host_call, False, twin=lambda a: region_twin(a, boxes[0]),
        notes="the box is host memory: staged and waited for")

    def get_packed_call(v, t):
        v.set_grid(t["vox"], origin, res)
        return [v.get_grid_packed()]
    add("get_grid_packed", *vox_pair, get_packed_call, True)

    def query_call(v, t):
        v.set_grid(t["vox"], origin, res)
        return [v.query_points(t["pts"], 0), v.query_points(t["pts"], 1)]
    add("query_points", dict(vox=world.voxels, pts=pts), dict(vox=world2.voxels, pts=rev(pts)), query_call, True,
        twin=lambda a: [lookups(a["vox"], a["pts"], 0), lookups(a["vox"], a["pts"], 1)])

    # -- the solve family on a batch of 5 trajectories of 16 control points; the decoy is the reversed batch
    b = mc.rich_guides(world, synth.make_bspline_batch(world, 5, 16, 4242, start_range=3.0, n_obs=2), 77)
    b.obs[0, :3], b.obs[0, 3:6] = b.ctrl[0, 8], 0.0                  # an obstacle parked on trajectory 0 ...
    b.obs[b.obs_off[4]:b.obs_off[5], :2] += 100.0                     # ... and trajectory 4's far away: the dynamic gate tells them apart
    w5 = mc.random_weights(P0)(np.random.default_rng(5), 5)
    order = [4, 3, 2, 1, 0]
    sb, sb_rev = batch_arrays(b, weights=w5), batch_arrays(b, order, weights=w5)

    def guides_unknown_call(v, t):
        v.set_grid(t["vox"], origin, res)
        return [v.guides_unknown(t["guide_pv"])]
    add("guides_unknown", dict(vox=world.voxels, guide_pv=sb["guide_pv"]), dict(vox=world2.voxels, guide_pv=sb_rev["guide_pv"]), guides_unknown_call, True,
        twin=lambda a: [lookups(a["vox"], a["guide_pv"][:, :3], 1)])

    total = int(sb["guide_off"][-1])
    short = sb["guide_off"].copy()
    short[-1] = total - 3                                             # monotone, three pairs fewer: fits the count passed below
    short = np.minimum.accumulate(short[::-1])[::-1].astype(np.int32)

    def check_lists_call(v, t):
        return [v.check_lists(5, 16, t["guide_off"], total - 3, t["obs_off"], int(sb["obs_off"][-1]))]
    add("check_lists", dict(guide_off=sb["guide_off"], obs_off=sb["obs_off"]), dict(guide_off=short, obs_off=sb_rev["obs_off"]), check_lists_call, False,
        notes="the real list names more pairs than the count passed (a violation, counted); the decoy fits it")

    def cost_grad_call(v, t):
        return list(v.cost_grad(t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], **_obs_kw(t)))
    add("cost_grad", dict(sb), dict(sb_rev), cost_grad_call, True,
        twin=lambda a: list(ol.cost_grad_batch(P0, _as_batch(a))))

    def optimize_call(v, t):
        return _solve_out(v.optimize(t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], inplace=True, **_obs_kw(t)))

    def optimize_twin(a):
        P = ol.default_params()
        _solve_params(P)
        r = ol.optimize_batch(P, _as_batch(a))
        return [r["ctrl"], r["status"]]
    add("optimize", dict(sb), dict(sb_rev), optimize_call, True, params=_solve_params, twin=optimize_twin)

    # mixed counts: 7, 12 and 16 control points in rows of 16
    parts = mc.make_parts(world, 32, 990, n_obs=1, counts=((7, 1), (16, 2), (12, 2)), weights=mc.random_weights(P0))
    pb, _ = synth.pad_batches(parts, interleave=True, Ns=16)
    assert len(set(pb.n_pts.tolist())) == 3 and pb.n_pts.tolist() != pb.n_pts.tolist()[::-1]
    mb, mb_rev = batch_arrays(pb, weights=pb.weights, n_pts=pb.n_pts), batch_arrays(pb, order, weights=pb.weights, n_pts=pb.n_pts)

    def cost_grad_mixed_call(v, t):
        return list(v.cost_grad_mixed(t["n_pts"], t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], **_obs_kw(t)))
    add("cost_grad_mixed", dict(mb), dict(mb_rev), cost_grad_mixed_call, True)

    def optimize_mixed_call(v, t):
        return _solve_out(v.optimize_mixed(t["n_pts"], t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], inplace=True, **_obs_kw(t)))
    add("optimize_mixed", dict(mb), dict(mb_rev), optimize_mixed_call, True, params=_solve_params)

    # the rebound rounds: the same batches with the state makePlan's first step leaves
    st_u = mc.initial_state(world, synth.PaddedBatch(b.ctrl, b.guide_off, b.guide_pv, b.guide_unk, b.obs_off, b.obs, None, {}, np.full(5, 16, np.int32)),
                            np.random.default_rng(11))
    st_m = mc.initial_state(world, pb, np.random.default_rng(12))
    ru, ru_rev = batch_arrays(b, weights=w5, state=st_u), batch_arrays(b, order, weights=w5, state=st_u)
    rm, rm_rev = (batch_arrays(pb, o, weights=pb.weights, n_pts=pb.n_pts, state=st_m) for o in (None, order))

    def rebound_call(v, t):
        v.set_grid(t["vox"], origin, res)
        v.rebound_rounds(t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], t["obs_off"], t["obs"], t["weights"], 0.1, t["state"], max_rounds=2)
        return [t["ctrl"], t["weights"], t["state"]]
    add("rebound_rounds", dict(ru, vox=world.voxels), dict(ru_rev, vox=world2.voxels), rebound_call, True, params=_solve_params)

    def rebound_mixed_call(v, t):
        v.set_grid(t["vox"], origin, res)
        v.rebound_rounds_mixed(t["n_pts"], t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], t["obs_off"], t["obs"], t["weights"], 0.1,
                               t["state"], max_rounds=2)
        return [t["ctrl"], t["weights"], t["state"]]
    add("rebound_rounds_mixed", dict(rm, vox=world.voxels), dict(rm_rev, vox=world2.voxels), rebound_mixed_call, False, params=_solve_params,
        notes="the table of sample counts per count is uploaded from the stack and waited for")

    # -- fit, evaluation, gates, finish
    fit_pts = rng.uniform(-2.0, 2.0, size=(5, 10, 3))
    fit_cd = rng.uniform(-0.5, 0.5, size=(5, 4, 3))
    add("bspline_fit", dict(points=fit_pts, conds=fit_cd), dict(points=rev(fit_pts), conds=rev(fit_cd)),
        lambda v, t: [v.bspline_fit(t["points"], t["conds"])], True,
        twin=lambda a: [ol.bspline_fit_batch(a["points"], P0.ts_ctrl, a["conds"])])
    n_fit = np.array([5, 14, 9, 14, 6], dtype=np.int32)
    fm_pts = rng.uniform(-2.0, 2.0, size=(5, 15, 3))
    zeros5 = np.zeros(5, dtype=np.int32)

    def fit_mixed_call(v, t):
        return list(v.bspline_fit_mixed(t["points"], t["n_fit"], 16, t["conds"], t["status"]))

    def fit_mixed_twin(a):
        return [ol.bspline_fit_batch(a["points"][i:i + 1, :n], P0.ts_ctrl, a["conds"][i:i + 1]) for i, n in enumerate(a["n_fit"])]
    add("bspline_fit_mixed", dict(points=fm_pts, n_fit=n_fit, conds=fit_cd, status=zeros5),
        dict(points=rev(fm_pts), n_fit=np.array([9, 6, 14, 5, 14], dtype=np.int32), conds=rev(fit_cd), status=zeros5), fit_mixed_call, True, twin=fit_mixed_twin)

    times = np.linspace(0.0, (16 - 3) * P0.ts_ctrl, 33)
    add("bspline_eval", dict(ctrl=sb["ctrl"], times=times), dict(ctrl=sb_rev["ctrl"], times=rev(times)),
        lambda v, t: [v.bspline_eval(t["ctrl"], t["times"], 0), v.bspline_eval(t["ctrl"], t["times"], 1)], True)

    def traj_collision_call(v, t):
        v.set_grid(t["vox"], origin, res)
        return list(v.traj_collision(t["ctrl"], 0.05))
    def gate_case(a):
        return gates.GateCase("", gates.World(a.get("vox"), world.origin, world.res), P0.ts_ctrl, 16, 0.05, a["ctrl"], obs_off=a.get("obs_off"), obs=a.get("obs"))
    add("traj_collision", dict(vox=world.voxels, ctrl=sb["ctrl"]), dict(vox=world2.voxels, ctrl=sb_rev["ctrl"]), traj_collision_call, True,
        twin=lambda a: list(gates.oracle_static(gate_case(a))))
    dyn = lambda a: {k: a[k] for k in ("ctrl", "obs_off", "obs")}
    add("traj_dynamic_collision", dyn(sb), dyn(sb_rev), lambda v, t: [v.traj_dynamic_collision(t["ctrl"], 0.05, t["obs_off"], t["obs"])], True,
        twin=lambda a: [gates.oracle_dynamic(gate_case(a))])

    def occupancy_call(v, t):
        v.set_grid(t["vox"], origin, res)
        return list(v.ctrl_occupancy(t["ctrl"]))
    add("ctrl_occupancy", dict(vox=world.voxels, ctrl=sb["ctrl"]), dict(vox=world2.voxels, ctrl=sb_rev["ctrl"]), occupancy_call, True,
        twin=lambda a: [lookups(a["vox"], a["ctrl"], 0)])

    f3 = fc.by_name("batch:3")                                        # counts 9, 16, 12 in rows of 16
    f_ctrl = np.nan_to_num(f3.ctrl, nan=0.0)
    S_cap = fc.plain_count(f3.dt, (f3.Ns - 3) * f3.ts_ctrl, False) + 2

    def finish_params(P):
        P.ts_ctrl, P.ts = f3.ts_ctrl, f3.ts
        P.pred_horizon = max(P.pred_horizon, f3.ts)

    def finish_call(v, t):
        d = t["ctrl"].device
        import torch
        outs = (torch.full((3, S_cap, 3), fc.SENTINEL, dtype=torch.float64, device=d), torch.full((3, S_cap, 3), fc.SENTINEL, dtype=torch.float64, device=d))
        r = v.traj_finish(t["ctrl"], t["limits"], f3.dt, S_cap, n_pts=t["n_pts"], out=outs)
        return [r[k] for k in ("factor", "max", "n", "pos", "vel", "status")]

    def finish_twin(a):
        r = synth.host_traj_finish(f3.ts_ctrl, f3.ts, a["ctrl"], a["limits"], f3.dt, S_cap, a["n_pts"])
        return [r[k] for k in ("factor", "max", "n", "pos", "vel", "status")]
    add("traj_finish", dict(ctrl=f_ctrl, limits=f3.limits, n_pts=f3.n_pts), dict(ctrl=rev(f_ctrl), limits=rev(f3.limits), n_pts=rev(f3.n_pts)),
        finish_call, True, params=finish_params, twin=finish_twin)

    # -- min-snap, the corridor checkers, the samplers
    wp = np.cumsum(rng.uniform(0.4, 1.2, size=(3, 4, 3)) * np.array([1.0, 0.5, 0.1]), axis=1) + np.array([0.0, 0.0, 1.0])
    cor = rng.uniform(0.4, 0.8, size=(3, 3))
    add("minsnap", dict(waypoints=wp, corridor=cor), dict(waypoints=rev(wp), corridor=rev(cor)),
        lambda v, t: list(v.minsnap(t["waypoints"], t["corridor"])), True)

    seg = next(c for c in cc.segment_cases() if len(c.n_samp) >= 5 and 0 < c.n_samp[:5].min())
    cw = seg.world
    c_origin, c_res = tuple(float(x) for x in cw.origin), float(cw.res)
    cvox2 = second_world(cw.voxels)
    cs = dict(coeffs=seg.coeffs[:5], n_samp=seg.n_samp[:5], delT=seg.delT[:5])
    cs_rev = {k: rev(a) for k, a in cs.items()}

    def install_corridor_world(v, t, c=seg):
        v.set_grid(t["vox"], c_origin, c_res)
        if c.bounds is not None:
            v.set_metric_bounds(*c.bounds)

    def corridor_call(v, t):
        install_corridor_world(v, t)
        return list(v.corridor_check(t["coeffs"], t["n_samp"], t["delT"], seg.box, seg.map_res))

    def corridor_twin(a):
        w = synth.World(a["vox"], cw.origin, cw.res, None)
        g, keep = ol.make_grid(w)
        if seg.bounds is not None:
            return None
        with ol.pow_mode(True):
            return list(ol.corridor_check_batch(g, a["coeffs"], a["n_samp"], a["delT"], np.array(seg.box), seg.map_res))
    add("corridor_check", dict(cs, vox=cw.voxels), dict(cs_rev, vox=cvox2), corridor_call, True, twin=corridor_twin)

    stride = int(cs["n_samp"].max())
    add("poly_sample", dict(cs), dict(cs_rev), lambda v, t: list(v.poly_sample(t["coeffs"], t["n_samp"], t["delT"], stride, want_f64=True, want_f32=True)), True,
        twin=lambda a: [ol.poly_sample(a["coeffs"], a["n_samp"], a["delT"], stride)])

    bpts = np.concatenate([rng.uniform(-4.0, 4.0, size=(120, 2)), rng.uniform(0.0, 2.0, size=(120, 1))], axis=1)

    def box_points_call(v, t):
        install_corridor_world(v, t)
        return [v.box_collision_points(t["pts"], seg.box, seg.map_res)]
    add("box_collision_points", dict(vox=cw.voxels, pts=bpts), dict(vox=cvox2, pts=rev(bpts)), box_points_call, True)

    tcase = next(t for t in cc.traj_cases() if len(t.trajs) >= 3 and t.world.name == cw.name and not t.name.startswith("non-finite"))
    keys = ("seg_off", "coeffs", "knots", "delT", "endpoint")
    tr, tr_rev = dict(zip(keys, pack_trajs(tcase.trajs[:3]))), dict(zip(keys, pack_trajs(tcase.trajs[:3][::-1])))

    def traj_corridor_call(v, t):
        install_corridor_world(v, t, tcase)
        return list(v.traj_corridor_check(t["seg_off"], t["coeffs"], t["knots"], t["delT"], t["endpoint"], tcase.box, tcase.map_res))
    add("traj_corridor_check", dict(tr, vox=cw.voxels), dict(tr_rev, vox=cvox2), traj_corridor_call, True)

    point_vox = lambda vox: _c(np.where(vox & 4, 3, 0), np.uint8)     # the point lookup reads bits 0 and 1

    def traj_point_call(v, t):
        v.set_grid(t["vox"], c_origin, c_res)
        return list(v.traj_point_check(t["seg_off"], t["coeffs"], t["knots"], t["delT"], t["endpoint"]))
    add("traj_point_check", dict(tr, vox=point_vox(cw.voxels)), dict(tr_rev, vox=point_vox(cvox2)), traj_point_call, True)

    # -- seed paths
    sw = sc.craft_world()
    crafted = sc.crafted()
    strajs = [crafted[n] for n in ("samples_3", "two_tries", "on_inner_knot", "past_max_length_wall", "goal_occupied")]
    skeys = ("seg_off", "coeffs", "knots", "duration", "dt0", "cpd", "max_len", "prev_seed", "prev_fit")
    sp, sp_rev = sc.pack(strajs), sc.pack(strajs[::-1])

    def seed_call(v, t):
        v.set_grid(t["vox"], tuple(sw.origin), sw.res)
        o = v.seed_paths(t["seg_off"], t["coeffs"], t["knots"], t["duration"], t["dt0"], t["cpd"], t["max_len"], t["prev_seed"], t["prev_fit"],
                         max_tries=sc.MAX_TRIES, point_cap=sc.POINT_CAP)
        return [o[k] for k in sc.OUT_KEYS]

    def seed_twin(a):
        full = dict(a, T=5, S=int(a["seg_off"][-1]))
        rc_, o = sc.twin(sc.World(a["vox"]), full, 0)
        assert rc_ == 0
        return [o[k] for k in sc.OUT_KEYS]
    add("seed_paths", dict({k: sp[k] for k in skeys}, vox=sw.vox), dict({k: sp_rev[k] for k in skeys}, vox=second_world(sw.vox, 3)), seed_call, True, twin=seed_twin)

    # -- A*: five searches on the wall world of tests/astar_cases.py, one pool and band
    acs = [c for c in ac.crafted_cases() if c.name in ("wall: detour", "start inside the wall (pushed out)", "end inside the wall (pushed out)",
                                                       "both ends inside obstacles", "ties: diagonal, empty world")]
    assert len(acs) == 5
    a_vox = next(c.vox for c in acs if c.name == "wall: detour")
    a_vox2 = next(c.vox for c in ac.crafted_cases() if c.name.startswith("enclosed goal"))
    a_start, a_end = np.stack([c.start for c in acs]), np.stack([c.end for c in acs])
    a_origin = tuple(float(x) for x in acs[0].origin)

    def astar_call(v, t):
        v.set_grid(t["vox"], a_origin, 0.1)
        return list(v.astar_search(t["start"], t["end"], 0.1, (40, 40, 40), 0.7, 1.3, path_cap=256))

    def astar_twin(a):
        lib = ac.host_lib()
        got = []
        for s, e in zip(a["start"], a["end"]):
            st, path, _, _ = ac.core_astar(lib, ac.Case("", a["vox"], np.array(a_origin), 0.1, (40, 40, 40), 0.7, 1.3, 0.1, s, e), **pc.shipped())
            got += [np.array([st]), np.zeros((0, 3)) if path is None else path]
        return got
    add("astar_search", dict(vox=a_vox, start=a_start, end=a_end), dict(vox=a_vox2, start=rev(a_start), end=rev(a_end)), astar_call, True, twin=astar_twin)

    # -- the prologue and the re-guide: five rows of the crafted batch (a block, the cage whose searches merge, the wall, a free
    # lane, the last point), uniform (32 control points) and mixed (12, 31 and 32 in rows of 32)
    hlib = pc.host_lib()
    CAP, POINT_CAP = PROLOGUE_CAP, PROLOGUE_POINT_CAP
    full, uni, mix = prologue_cases()
    p_origin, p_res = tuple(float(x) for x in full.origin), float(full.res)
    p_vox2 = second_world(full.vox, 2)
    pair_cap = 5 * (32 + 4 * rc.MAX_SEGS) + 8

    def prologue_rows(case, mixed):
        n_real, n_decoy = case.n_pts, case.n_pts[::-1]
        rows_ = pm.reguide_rows(hlib, case)
        goff, gpv = rows_.csr(case)
        helper = rc.Case("", case.vox, case.origin, case.res, case.cfg, case.padded(), goff, gpv, rows_.weights, rows_.state)
        gunk = helper.gunk()
        rcase = case.subset(range(case.B)[::-1], Ns=32)
        rrows = pm.ReguideRows(rows_.state[::-1], rows_.weights[::-1], rows_.pairs[::-1])
        goff_r, gpv_r = rrows.csr(rcase)
        gunk_r = rc.Case("", p_vox2, case.origin, case.res, case.cfg, rcase.padded(), goff_r, gpv_r, rrows.weights, rrows.state).gunk()
        assert len(gpv) == len(gpv_r) > 0
        pad6 = lambda a: np.concatenate([a.reshape(-1, 6), np.zeros((1, 6))])
        pad1 = lambda a: np.concatenate([a, np.zeros(1, dtype=np.uint8)])
        base = (dict(vox=case.vox, ctrl=case.padded()), dict(vox=p_vox2, ctrl=rcase.padded()))
        if mixed:
            base[0]["n_pts"], base[1]["n_pts"] = _c(n_real), _c(n_decoy)
        n_of = lambda t: (t["n_pts"],) if mixed else ()
        sfx = "_mixed" if mixed else ""
        search_kw = dict(not_check_ratio=case.ncr, search_path_cap=CAP, seg_cap=5 * pc.MAX_SEGS, point_cap=POINT_CAP, fill=-7)

        def grid(v, t):
            v.set_grid(t["vox"], p_origin, p_res)

        def segs_call(v, t):
            grid(v, t)
            return list(getattr(v, "collision_segs" + sfx)(*n_of(t), t["ctrl"], case.ncr, seg_cap=5 * pc.MAX_SEGS, fill=-7))

        def search(v, t):
            return getattr(v, "path_search" + sfx)(*n_of(t), t["ctrl"], p_res, case.pool, case.cfg[1], case.cfg[2], **search_kw)

        def search_call(v, t):
            grid(v, t)
            return list(search(v, t))

        def derive_paths(v, t):
            grid(v, t)
            _, so, sg, po, pa, _ = search(v, t)
            return dict(seg_off=so, seg=sg, path_off=po, path=pa)

        def guides_call(v, t):
            grid(v, t)
            return list(getattr(v, "guide_assign" + sfx)(*n_of(t), t["ctrl"], t["seg_off"], t["seg"], t["path_off"], t["path"], pair_cap, fill=-7))

        def reguide_call(v, t):
            grid(v, t)
            o = getattr(v, "rebound_reguide" + sfx)(*n_of(t), t["ctrl"], t["guide_off"], t["guide_pv"], t["guide_unk"], t["weights"], t["state"], p_res,
                                                      case.pool, case.cfg[1], case.cfg[2], len(gpv) + pair_cap, **search_kw)
            return list(o) + [t["weights"], t["state"]]

        def segs_twin(a):
            w = pc.Workload("", a["vox"], case.origin, case.res, a["ctrl"], case.cfg, ncr=case.ncr)
            r_, so, sg, st = pc.twin_segments(hlib, w)
            assert r_ == 0
            return [so, sg, st]

        def search_twin(a):
            w = pc.Workload("", a["vox"], case.origin, case.res, a["ctrl"], case.cfg, ncr=case.ncr)
            r_ = pc.twin(hlib, w, cap=pc.shipped(), search_path_cap=CAP)
            assert r_.rc == 0
            return [r_.status, r_.seg_off, r_.seg, r_.path_off, r_.path]
        tw = {} if mixed else dict(twin=segs_twin)                  # (the host twins take one count per call)
        add("collision_segs" + sfx, dict(base[0]), dict(base[1]), segs_call, False, **tw)
        tw = {} if mixed else dict(twin=search_twin)
        add("path_search" + sfx, dict(base[0]), dict(base[1]), search_call, False, **tw)
        add("guide_assign" + sfx, dict(base[0]), dict(base[1]), guides_call, False, derive=derive_paths)
        rg = (dict(base[0], guide_off=goff, guide_pv=pad6(gpv), guide_unk=pad1(gunk), weights=rows_.weights, state=rows_.state),
              dict(base[1], guide_off=goff_r, guide_pv=pad6(gpv_r), guide_unk=pad1(gunk_r), weights=rrows.weights, state=rrows.state))
        add("rebound_reguide" + sfx, *rg, reguide_call, False)

    prologue_rows(uni, False)
    prologue_rows(mix, True)

    # -- the ESDF: a lattice installed, and the field built from the snapshot and refreshed after a region update
    lat, e_origin = synth.sphere_esdf(32, 0.2, (0.3, -0.2, 0.1), 1.5)
    lat2, _ = synth.sphere_esdf(32, 0.2, (-0.9, 0.4, 0.0), 1.0)
    q = rng.uniform(-3.0, 3.0, size=(129, 3))
    q32 = q.astype(np.float32)

    def esdf_rows(name, pts_real, call, twin):
        def run(v, t):
            v.set_esdf(t["dist"], tuple(e_origin), 0.2)
            return call(v, t)
        add(name, dict(dist=lat, pts=pts_real), dict(dist=lat2, pts=rev(pts_real)), run, True,
            twin=lambda a: twin(a["dist"], e_origin, 0.2, a["pts"]))
    esdf_rows("set_esdf", q, lambda v, t: list(v.esdf_query(t["pts"])), lambda *a: list(ol.esdf_query_batch(*a)))
    esdf_rows("esdf_query", q[::2], lambda v, t: list(v.esdf_query(t["pts"])), lambda *a: list(ol.esdf_query_batch(*a)))
    esdf_rows("esdf_query_f32", q32, lambda v, t: [v.esdf_query_f32(t["pts"])], lambda *a: [ol.esdf_query_f32_batch(*a)])

    ucase = uc.by_name("9x70x31_three_updates_one_refresh")
    g0 = uc.start_grid(ucase)
    g1 = _c(g0[::-1, ::-1])
    u_res = uc.res_of(ucase)
    u_origin = (0.0, 0.0, 0.0)
    step = ucase.steps[1]
    box2 = _c(step.box[::-1])
    eq = rng.uniform(0.0, 1.0, size=(65, 3)) * np.array(g0.shape) * u_res

    def build_call(tracked):
        def run(v, t):
            v.set_grid(t["vox"], u_origin, u_res)
            lattice = v.build_esdf(plane=2, return_lattice=True, tracked=tracked)
            return [lattice] + list(v.esdf_query(t["pts"]))
        return run

    def build_twin(a):
        return [synth.host_esdf(synth.World(a["vox"], np.zeros(3), u_res, None), 2, False)[0]]
    add("build_esdf", dict(vox=g0, pts=eq), dict(vox=g1, pts=rev(eq)), build_call(False), True, twin=build_twin)
    add("build_esdf_tracked", dict(vox=g0, pts=eq), dict(vox=g1, pts=rev(eq)), build_call(True), True, twin=build_twin)

    def update_call(stats):
        def run(v, t):
            v.set_grid(t["vox"], u_origin, u_res)
            v.build_esdf(plane=2, tracked=True)
            v.update_grid_region(step.lo, t["box"])
            r = v.update_esdf(return_lattice=True, stats=stats)
            extra = [int(r[1]["y_lines"]), int(r[1]["x_lines"])] if stats else []
            return [r[0] if stats else r] + list(v.esdf_query(t["pts"])) + extra
        return run

    def update_twin(a):
        rc_, ta, tb, tl = synth.host_esdf_tracked(a["vox"], 2, False, u_res)
        assert rc_ == 0
        rc_, new = synth.host_grid_region_apply(a["vox"], step.lo, a["box"])
        assert rc_ == 0
        rc_, st = synth.host_esdf_update(new, step.lo, step.box.shape, ta, tb, tl, 2, False, u_res)
        assert rc_ == 0
        return [tl]
    up = (dict(vox=g0, box=step.box, pts=eq), dict(vox=g1, box=box2, pts=rev(eq)))
    add("update_esdf", dict(up[0]), dict(up[1]), update_call(False), True, twin=update_twin)
    add("update_esdf_stats", dict(up[0]), dict(up[1]), update_call(True), False, entry="vigo_update_esdf", twin=update_twin,
        notes="the line counters are read back")
    names = [r.name for r in out]
    assert len(set(names)) == len(names)
    return tuple(out)


PROLOGUE_CAP, PROLOGUE_POINT_CAP = 512, 1 << 15                    # search_path_cap and point_cap of the prologue rows


@functools.lru_cache(maxsize=None)
def prologue_cases():
    """(the crafted batch of counts 12, 31 and 32; five of its rows with 32 control points; five with 12, 31 and 32 in rows of
    32): a block, the cage whose searches merge, the wall whose search fails, a free lane, the last point"""
    import prologue_mixed_cases as pm
    full = pm.crafted_case(0.0, counts=(12, 31, 32))
    pick = lambda wanted: [next(i for i, n in enumerate(full.names) if n == w) for w in wanted]
    uni = full.subset(pick(["32 points, block lane", "32 points, cage lane", "32 points, wall lane", "32 points, free lane", "32 points, last point"]), Ns=32)
    mix = full.subset(pick(["12 points, block lane", "32 points, cage lane", "31 points, wall lane", "12 points, free lane", "32 points, last point"]), Ns=32)
    return full, uni, mix


def by_name(name):
    return next(r for r in rows() if r.name == name)


# the ids of the GPU test, known without building the table (tests/test_stream_cases.py holds them against rows())
ROW_NAMES = (
    "pack_grid", "inflate_grid", "set_grid", "set_grid_packed", "set_grid_host", "update_grid_region", "update_grid_region_host", "get_grid_packed",
    "query_points", "guides_unknown", "check_lists", "cost_grad", "optimize", "cost_grad_mixed", "optimize_mixed", "rebound_rounds", "rebound_rounds_mixed",
    "bspline_fit", "bspline_fit_mixed", "bspline_eval", "traj_collision", "traj_dynamic_collision", "ctrl_occupancy", "traj_finish", "minsnap",
    "corridor_check", "poly_sample", "box_collision_points", "traj_corridor_check", "traj_point_check", "seed_paths", "astar_search",
    "collision_segs", "path_search", "guide_assign", "rebound_reguide", "collision_segs_mixed", "path_search_mixed", "guide_assign_mixed",
    "rebound_reguide_mixed", "set_esdf", "esdf_query", "esdf_query_f32", "build_esdf", "build_esdf_tracked", "update_esdf", "update_esdf_stats")

# assertion (b): the entries that reach neither read_back nor a stream or event wait on a cold handle (csrc/vigo_api.cpp).
# Not in it: set_grid_host and update_grid_region_host (a staged host copy, waited for), check_lists, guide_assign, collision_segs,
# path_search, rebound_reguide and their _mixed forms (read_back), rebound_rounds_mixed (the count table's upload), update_esdf
# with stats (read_back).
NO_ROUND_TRIP = (
    "pack_grid", "inflate_grid", "set_grid", "set_grid_packed", "update_grid_region", "get_grid_packed", "query_points", "guides_unknown", "cost_grad",
    "optimize", "cost_grad_mixed", "optimize_mixed", "rebound_rounds", "bspline_fit", "bspline_fit_mixed", "bspline_eval", "traj_collision",
    "traj_dynamic_collision", "ctrl_occupancy", "traj_finish", "minsnap", "corridor_check", "poly_sample", "box_collision_points", "traj_corridor_check",
    "traj_point_check", "seed_paths", "astar_search", "set_esdf", "esdf_query", "esdf_query_f32", "build_esdf", "build_esdf_tracked", "update_esdf")
