"""-m gpu: vigo_seed_paths (csrc/vigo_seed.hip, a wavefront per trajectory) against its host twin with the kernels' exact
power (vigo_seed_paths_host, pinned on the CPU by test_seed_core.py against the facade's steps and a Python
restatement) bit for bit on every output array: the two 64-pair workloads with coefficients from vigo_minsnap, every
crafted case alone and all of them in one launch; the hostile arguments; two calls on one handle."""
import ctypes as C

import numpy as np
import pytest
import torch

import seed_cases as sc
from gpu_util import to_dev

pytestmark = pytest.mark.gpu
IN_KEYS = ("seg_off", "coeffs", "knots", "duration", "dt0", "cpd", "max_len", "prev_seed", "prev_fit")


def device_run(v, a, max_tries=sc.MAX_TRIES, point_cap=sc.POINT_CAP):
    """vigo_seed_paths on the arrays of seed_cases.pack(), the outputs pre-filled with the twin's sentinels"""
    d = v.device
    dev_in = [to_dev(a[k], d) for k in IN_KEYS]
    o = {k: to_dev(x, d) for k, x in sc.blank_outputs(a["T"], point_cap).items()}
    P = lambda x: C.c_void_p(x.data_ptr())
    rc = v._lib.vigo_seed_paths(v._h, a["T"], a["S"], 7, *[P(x) for x in dev_in], max_tries, point_cap, *[P(o[k]) for k in sc.OUT_KEYS])
    torch.cuda.synchronize()
    return rc, {k: x.cpu().numpy() for k, x in o.items()}


@pytest.fixture()
def craft(vigo_handle):
    w = sc.craft_world()
    vigo_handle.set_grid(to_dev(w.vox, vigo_handle.device), w.origin, w.res)
    return vigo_handle, w


@pytest.mark.parametrize("which", ["open", "pillar"])
def test_workloads_equal_the_twin(vigo_handle, which):
    v = vigo_handle
    w = sc.workload_world(which)
    v.set_grid(to_dev(w.vox, v.device), w.origin, w.res)
    pairs = sc.workload_pairs(which)
    coeffs, knots, status = v.minsnap(to_dev(pairs, v.device), conds=to_dev(np.zeros((64, 4, 3)), v.device), vel=1.0)
    assert (status.cpu().numpy() == 0).all()
    kn = knots.cpu().numpy()
    trajs = [sc.Traj(f"pair_{t}", kn[t].copy(), coeffs[t].cpu().numpy().copy(), float(kn[t, -1]), dt0=sc.CPD / 1.0) for t in range(64)]
    a = sc.pack(trajs)
    rc, got = device_run(v, a, max_tries=16)
    assert rc == 0
    rc, want = sc.twin(w, a, 0, max_tries=16)
    assert rc == 0
    sc.assert_same_outputs(got, want, which)
    assert (got["status"] != sc.DEFERRED).all() and (got["status"] == sc.OK).sum() >= 48
    assert (got["tries"] > 1).any()                             # the search did retry
    # the Python wrapper returns the same arrays (zeros where nothing is written)
    r = v.seed_paths(to_dev(a["seg_off"], v.device), to_dev(a["coeffs"], v.device), to_dev(a["knots"], v.device),
                     *[to_dev(a[k], v.device) for k in ("duration", "dt0", "cpd", "max_len")], max_tries=16, point_cap=sc.POINT_CAP)
    for k in ("status", "tries", "seed_n", "fit_n", "dt", "final_time", "prev_seed", "prev_fit"):
        assert np.array_equal(r[k].cpu().numpy(), want[k]), k
    for t in range(64):
        assert np.array_equal(r["seed"][t, :want["seed_n"][t]].cpu().numpy(), want["seed"][t, :want["seed_n"][t]])
        assert np.array_equal(r["fit"][t, :want["fit_n"][t]].cpu().numpy(), want["fit"][t, :want["fit_n"][t]])


def test_crafted_cases_equal_the_twin(craft):
    v, w = craft
    cases = sc.crafted()
    for name, c in cases.items():
        a = sc.pack([c])
        rc, got = device_run(v, a)
        assert rc == 0, name
        rc, want = sc.twin(w, a, 0)
        assert rc == 0, name
        sc.assert_same_outputs(got, want, name)
        if "status" in c.expect:
            assert got["status"][0] == c.expect["status"], name
        if "tries" in c.expect and got["status"][0] != sc.DEFERRED:
            assert got["tries"][0] == c.expect["tries"], name
    # T = 65, every case in one launch
    names = list(cases)
    a = sc.pack([cases[names[i % len(names)]] for i in range(65)])
    rc, got = device_run(v, a)
    rc2, want = sc.twin(w, a, 0)
    assert rc == 0 and rc2 == 0
    sc.assert_same_outputs(got, want, "mixed")
    assert set(got["status"]) == {sc.OK, sc.NO_SPACING, sc.GOAL_OCCUPIED, sc.TOO_SHORT, sc.DEFERRED, sc.BAD_INPUT}
    # a list longer than point_cap is deferred, nothing written
    a = sc.pack([cases["past_max_length"]])
    rc, got = device_run(v, a, point_cap=10)
    rc2, want = sc.twin(w, a, 0, point_cap=10)
    assert rc == 0 and got["status"][0] == sc.DEFERRED
    sc.assert_same_outputs(got, want, "point_cap")


def test_two_calls_on_one_handle_give_identical_results(craft):
    v, w = craft
    cases = sc.crafted()
    a = sc.pack([cases[n] for n in ("two_tries", "past_max_length_wall", "samples_65", "goal_occupied", "prev_above_max_both")])
    (rc1, r1), (rc2, r2) = device_run(v, a), device_run(v, a)
    assert rc1 == 0 and rc2 == 0
    sc.assert_same_outputs(r1, r2, "repeat")


def test_hostile_arguments_return_their_error_and_write_nothing(vigo_handle):
    v = vigo_handle
    d = v.device
    a = sc.pack([sc.crafted()["one_try"]])
    dev_in = [to_dev(a[k], d) for k in IN_KEYS]
    blank = sc.blank_outputs(1)
    outs = [to_dev(blank[k], d) for k in sc.OUT_KEYS]
    P = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def call(h=v._h, T=1, S=1, deg=7, ins=dev_in, max_tries=4, point_cap=sc.POINT_CAP, outp=outs):
        return v._lib.vigo_seed_paths(h, T, S, deg, *[P(x) for x in ins], max_tries, point_cap, *[P(x) for x in outp])

    def untouched():
        torch.cuda.synchronize()
        return all(np.array_equal(x.cpu().numpy(), blank[k]) for k, x in zip(sc.OUT_KEYS, outs))
    assert call() == -5 and untouched()                          # VIGO_ERR_NO_GRID before a grid
    w = sc.craft_world()
    v.set_grid(to_dev(w.vox, d), w.origin, w.res)
    assert call(h=None) == -1
    assert call(T=-1) == -1 and call(S=-1) == -1 and call(deg=16) == -1 and call(deg=-1) == -1
    assert call(max_tries=0) == -1 and call(point_cap=-1) == -1
    for i in range(len(dev_in)):
        ins = list(dev_in)
        ins[i] = None
        assert call(ins=ins) == -1, IN_KEYS[i]
    for i in range(len(outs)):
        o = list(outs)
        o[i] = None
        assert call(outp=o) == -1, sc.OUT_KEYS[i]
    assert untouched()
    assert call(T=0, S=0, ins=[None] * 9, outp=[None] * 10) == 0
    # offsets outside [0, S] are that trajectory's status, not a fault
    for bad in ([0, 5], [-1, 1], [1, 0]):
        ins = list(dev_in)
        ins[0] = to_dev(np.array(bad, np.int32), d)
        assert call(ins=ins) == 0
        torch.cuda.synchronize()
        assert outs[0].cpu().tolist() == [sc.BAD_INPUT] and outs[4].cpu().tolist() == [0]
    assert call() == 0
    torch.cuda.synchronize()
    assert outs[0].cpu().tolist() == [sc.OK]
    with pytest.raises(ValueError):
        v.seed_paths(dev_in[0], dev_in[1], dev_in[2][:-1], *dev_in[3:7])
    cap = C.c_int32(0)
    assert v._lib.vigo_seed_capacity(C.byref(cap)) == 0 and cap.value == sc.capacity()
    assert v._lib.vigo_seed_capacity(None) == -1
