"""-m gpu: the entry points that share and regrow a handle's device buffers (csrc/vigo_handle.hpp, vigo_ws_layout.hpp).
One handle runs a sequence in which every buffer is used at a small size, grown, used at the small size again, and
handed from one entry point to the next; after every call the outputs are compared bit for bit with the same call on a
handle created only for it.  The odd batch sizes (1, 3, 33) are the smallest at which a workspace array that lost its
alignment or its last element would show."""
import numpy as np
import pytest
import torch

import corridor_cases as cc
import pathsearch_cases as pc
import reguide_cases as rc
from gpu_util import to_dev
from trajectory_planner_amd.vigo import Vigo

pytestmark = pytest.mark.gpu
CAP = 512                                                         # search_path_cap, as in the path-search and re-guide tests


def _host(tensors):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in tensors]


def _path_search(w):
    def run(v):
        v.set_grid(to_dev(w.vox, v.device), w.origin, w.res)
        sc, pcap = pc.caps(w, CAP)
        return _host(v.path_search(to_dev(w.ctrl, v.device), w.res, w.pool, w.cfg[1], w.cfg[2], not_check_ratio=w.ncr, search_path_cap=CAP,
                                   seg_cap=sc, point_cap=pcap))
    return run


def _corridor(c, S):
    def run(v):
        v.set_grid(to_dev(c.world.voxels, v.device), c.world.origin, c.world.res)
        if c.bounds is not None:
            v.set_metric_bounds(*c.bounds)
        return _host(v.corridor_check(to_dev(c.coeffs[:S], v.device), to_dev(c.n_samp[:S], v.device), to_dev(c.delT[:S], v.device), c.box, c.map_res))
    return run


def _reguide(c):
    def run(v):
        d = v.device
        v.set_grid(to_dev(c.vox, d), c.origin, c.res)
        weights, state = to_dev(c.weights, d), to_dev(c.state, d)             # updated in place: outputs too
        gpv = to_dev(np.concatenate([c.gpv.reshape(-1, 6), np.zeros((1, 6))]), d)
        gunk = to_dev(np.concatenate([c.gunk(), np.zeros(1, dtype=np.uint8)]), d)
        scap = c.B * rc.MAX_SEGS
        out = v.rebound_reguide(to_dev(c.ctrl, d), to_dev(c.goff, d), gpv, gunk, weights, state, c.res if c.step is None else c.step, c.pool,
                                c.cfg[1], c.cfg[2], rc.pair_room(c), not_check_ratio=c.ncr, search_path_cap=CAP, seg_cap=scap,
                                point_cap=min(scap * (CAP + 1), 1 << 21), want_paths=True, fill=-7)
        return _host(list(out) + [weights, state])
    return run


def _traj_collision(w):
    def run(v):
        v.set_grid(to_dev(w.vox, v.device), w.origin, w.res)
        return _host(v.traj_collision(to_dev(w.ctrl, v.device), 0.1))
    return run


def _fit(K):
    pts = np.random.default_rng(K).uniform(-2.0, 2.0, size=(5, K, 3))
    return lambda v: _host([v.bspline_fit(to_dev(pts, v.device))])


def _inflate(v):
    vox = (np.random.default_rng(8).random((8, 8, 40)) < 0.05).astype(np.uint8) * 4
    return _host([v.inflate_grid(to_dev(vox, v.device), 1, 1, 1)])


def test_entry_points_sharing_one_handle_equal_fresh_handles():
    crafted = dict(pc.crafted_workloads())
    one = crafted["a merge taken while another segment stays unmerged"]   # B = 1: four searches, second choices among them
    pipe = pc.pipeline_workload()
    many = pipe.subset(range(33))
    derived = rc.derived_batch(128)
    done = [int(b) for b in np.nonzero(derived.state[:, rc.S_NSEG] > 0)[0]]
    few, more = derived.subset(done[:3]), derived.subset(range(33))
    corridor = next(c for c in cc.segment_cases() if len(c.n_samp) >= 5)
    steps = [("path search, B = 1", _path_search(one)), ("path search, B = 33", _path_search(many)), ("path search, B = 1 again", _path_search(one)),
             ("corridor check, S = 5", _corridor(corridor, 5)),
             ("re-guide, B = 3", _reguide(few)), ("re-guide, B = 33", _reguide(more)), ("re-guide, B = 3 again", _reguide(few)),
             ("trajectory gate", _traj_collision(many)), ("fit, K = 8", _fit(8)), ("fit, K = 40", _fit(40)),
             ("trajectory gate after the fits", _traj_collision(many)), ("inflate 8 x 8 x 40", _inflate),
             ("path search, B = 1 at the end", _path_search(one))]
    shared = Vigo(0)
    seen = {}
    try:
        for label, run in steps:
            got = run(shared)
            fresh = Vigo(0)
            try:
                want = run(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want), label
            for k, (a, b) in enumerate(zip(got, want)):
                assert (a is None) == (b is None) and (a is None or (a.shape == b.shape and a.tobytes() == b.tobytes())), (label, k)
            seen[label] = got
    finally:
        shared.close()
    # the sequence does what it is for: searches of both choices, paths and appended pairs, a grown operator, set bits
    assert seen["path search, B = 1"][5][0, 0] >= 2 and int(seen["path search, B = 33"][1][-1]) > 0
    status, off = seen["re-guide, B = 33"][0], seen["re-guide, B = 33"][1]
    assert (status == rc.DONE).any() and int(off[-1]) > len(more.gpv) and int(seen["re-guide, B = 33"][4][-1]) > 0
    assert (seen["re-guide, B = 3"][0] == rc.DONE).any()
    assert seen["fit, K = 40"][0].shape == (5, 42, 3) and seen["inflate 8 x 8 x 40"][0].sum() > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(seen["trajectory gate"], seen["trajectory gate after the fits"]))
