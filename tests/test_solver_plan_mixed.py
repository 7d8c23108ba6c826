"""-m "not gpu": the launch plan of the mixed-count entries (plan_optimize_mixed, csrc/vigo_solver_plan.hpp), the workspace of
vigo_rebound_rounds_mixed (csrc/vigo_ws_layout.hpp) and the padded batch layout (synth.pad_batches).
tests/solver_plan_mixed_check.cpp is a program of its own: built here with the address and undefined-behaviour
sanitizers, it answers queries from stdin with the headers' functions."""
import os
import subprocess

import numpy as np
import pytest

import solver_dispatch_rule as rule
from trajectory_planner_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")
MODES = ("f64", "fast", "f32")
STRIDES = (7, 8, 31, 32, 33, 63, 64)
SIMDS = (0, 4, 1024)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("solver_plan_mixed") / "solver_plan_mixed_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "solver_plan_mixed_check.cpp"), "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        answers = r.stdout.split("\n")[:-1]
        assert len(answers) == len(queries)
        return answers
    return ask


def keys_of(answer):
    return [tuple(int(x) for x in k.split()) for k in answer.split(";")]


def batch_sizes(S, group):
    """either side of the SIMD count, in trajectories and in waves (of 64 / group trajectories)"""
    if S == 0:
        return (1, 40, 5000)
    tpb = 64 // group
    return sorted({b for b in (1, 2, S - 1, S, S + 1, tpb * S - 1, tpb * S, tpb * S + 1, tpb * S + 2, 16 * S) if b > 0})


def test_one_general_launch_sized_by_the_stride(ask):
    cases = [(mode, Ns, B, m, obs, S) for mode in MODES for Ns in STRIDES for m in range(1, 17) for S in SIMDS
             for B in batch_sizes(S, rule.shape_for(Ns)[0]) for obs in (0, 1)]
    answers = ask([f"M {Ns} {B} {rule.PREC[mode]} {obs} {m} {S}" for mode, Ns, B, m, obs, S in cases])
    mixed_keys = keys_of(ask(["MK"])[0])
    assert len(mixed_keys) == 12 and len(set(mixed_keys)) == 12
    # {f32, f64_fast, f64} x {32 x 1, 64 x 1} x {WPS 1, 2}: the general kernel (OBS, D = 3, RH = 1)
    assert set(mixed_keys) == {(rule.PREC[mode], g, 1, wps, 1, 3, 1) for mode in MODES for g in (32, 64) for wps in (1, 2)}
    selected = set()
    for (mode, Ns, B, m, obs, S), a in zip(cases, answers):
        assert a != "error" and ";" not in a, (mode, Ns, B, m, obs, S)              # ONE launch
        prec, group, ppl, wps, kobs, d, rh, grid, lds, lwe = (int(x) for x in a.split())
        tpb = 64 // group
        assert (prec, group, ppl) == (rule.PREC[mode],) + rule.shape_for(Ns)
        assert (kobs, d, rh, lwe) == (1, 3, 1, 0)
        assert grid == (B + tpb - 1) // tpb
        assert lds == rule.lds_bytes(mode, Ns, m) and lds <= 64 * 1024               # at Ns, with the table; no limit to raise
        assert wps == (2 if S > 0 and grid > S and lds <= rule.LDS // 8 else 1)
        selected.add((prec, group, ppl, wps, kobs, d, rh))
    assert selected == set(mixed_keys), f"never selected: {set(mixed_keys) - selected}"
    # ... the same bytes as the header's own requirement for a uniform call of Ns points
    lds_cases = [(mode, Ns, m) for mode in MODES for Ns in STRIDES for m in (1, 8, 16)]
    assert [int(a) for a in ask([f"R {Ns} {m} {rule.PREC[mode]}" for mode, Ns, m in lds_cases])] == \
        [rule.lds_bytes(mode, Ns, m) for mode, Ns, m in lds_cases]


def test_strides_outside_7_to_64_are_refused(ask):
    qs = [f"M {Ns} {B} {rule.PREC[mode]} {obs} 16 {S}" for Ns in (6, 65, 256) for mode in MODES for B in (1, 40, 5000) for obs in (0, 1) for S in SIMDS]
    assert ask(qs) == ["error"] * len(qs)


def test_counts_of_a_mixed_call_share_the_shape_class_of_the_stride(ask):
    cases = [(n, Ns) for Ns in (6, 7, 8, 31, 32, 33, 40, 63, 64, 65) for n in range(-1, 70)]
    got = [int(a) for a in ask([f"C {n} {Ns}" for n, Ns in cases])]
    assert got == [int(7 <= n <= Ns <= 64 and (n <= 32) == (Ns <= 32)) for n, Ns in cases]


def test_the_uniform_key_list_is_unchanged(ask):
    keys = keys_of(ask(["K"])[0])
    assert len(keys) == 53 and len(set(keys)) == 53
    f32, fast, f64 = rule.PREC["f32"], rule.PREC["fast"], rule.PREC["f64"]
    assert keys[:4] == [(f32, 32, 1, 2, 0, 2, 1), (f32, 32, 1, 1, 0, 2, 1), (f32, 32, 1, 2, 0, 3, 1), (f32, 32, 1, 1, 0, 3, 1)]
    assert keys[10] == (fast, 32, 1, 2, 0, 2, 4) and keys[22] == (f64, 32, 1, 1, 0, 1, 1) and keys[35] == (f32, 32, 1, 2, 1, 3, 1)
    assert keys[-6:] == [(f64, 32, 1, 2, 1, 3, 1), (f64, 32, 1, 1, 1, 3, 1), (f64, 64, 1, 2, 1, 3, 1), (f64, 64, 1, 1, 1, 3, 1),
                         (f64, 64, 2, 1, 1, 3, 0), (f64, 64, 4, 1, 1, 3, 0)]
    assert sum(k[4] for k in keys) == 18 and sum(1 for k in keys if k[5] == 1) == 1


def test_rebound_workspace_fits_its_own_size(ask):
    cases = [(B, Ns) for B in (1, 2, 3, 40, 1025) for Ns in (7, 8, 32, 33, 64)]
    got = [int(a) for a in ask([f"W {B} {Ns}" for B, Ns in cases])]
    for (B, Ns), bytes_ in zip(cases, got):
        # 16 flags, B + 16 indices, a pair per count, each array on an 8-byte boundary
        assert bytes_ == 64 + ((4 * (B + 16) + 7) & ~7) + 8 * (Ns - 6), (B, Ns)


def test_pad_batches_layout():
    world = synth.make_box_world(synth.SEED_BASE + 2, n=64, n_boxes=30, centre_range=2.5, z_range=2.0)
    parts = [synth.make_bspline_batch(world, B, N, 40 + N, start_range=2.0, n_obs=n_obs, guide2_prob=0.6)
             for B, N, n_obs in ((3, 9, 0), (2, 16, 2), (4, 12, 0))]
    assert sum(len(p.guide_pv) for p in parts) > 0
    for interleave in (False, True):
        pb, rows = synth.pad_batches(parts, interleave=interleave)
        B, Ns = 9, 16
        assert pb.ctrl.shape == (B, Ns, 3) and pb.guide_off.shape == (B * Ns + 1,) and pb.n_pts.dtype == np.int32
        assert sorted(np.concatenate(rows).tolist()) == list(range(B))
        if interleave:
            assert [r.tolist() for r in rows] == [[0, 3, 6], [1, 4], [2, 5, 7, 8]]
        else:
            assert [r.tolist() for r in rows] == [[0, 1, 2], [3, 4], [5, 6, 7, 8]]
        assert pb.guide_off[0] == 0 and np.all(np.diff(pb.guide_off) >= 0) and pb.guide_off[-1] == len(pb.guide_pv) == len(pb.guide_unk)
        assert pb.obs_off[0] == 0 and pb.obs_off[-1] == len(pb.obs) == 4
        for p, r in zip(parts, rows):
            for k, i in enumerate(r):
                n = p.N
                assert pb.n_pts[i] == n
                assert np.array_equal(pb.ctrl[i, :n], p.ctrl[k]) and not pb.ctrl[i, n:].any()
                off = pb.guide_off[i * Ns:(i + 1) * Ns + 1]
                src = p.guide_off[k * n:(k + 1) * n + 1]
                assert np.array_equal(np.diff(off[:n + 1]), np.diff(src)) and np.all(off[n:] == off[n])      # padding: empty lists
                assert np.array_equal(pb.guide_pv[off[0]:off[n]], p.guide_pv[src[0]:src[n]])
                assert np.array_equal(pb.guide_unk[off[0]:off[n]], p.guide_unk[src[0]:src[n]])
                want_obs = p.obs[p.obs_off[k]:p.obs_off[k + 1]] if p.obs is not None else np.zeros((0, 9))
                assert np.array_equal(pb.obs[pb.obs_off[i]:pb.obs_off[i + 1]], want_obs)


def test_host_batch_packs_planners_as_pad_batches_does(tmp_path):
    """the facade's HostBatch (host/src/batchLayout.h) with a stride against synth.pad_batches on a three-count example:
    padded control-point rows, re-based guide offsets with empty lists on the padding, n_pts, obstacles, weights"""
    host = os.path.join(HERE, "..", "trajectory_planner_amd", "host")
    exe = str(tmp_path / "host_batch_layout_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(host, "include"), "-I", os.path.join(rocm, "include"),
                    os.path.join(HERE, "host_batch_layout_check.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(3)
    spec = [(9, 2, 0), (16, 1, 2), (12, 2, 1)]        # (control points, planners, obstacles per planner) per source batch
    parts, lines, t = [], [], 0
    for N, B, n_obs in spec:
        counts = np.zeros((B, N), dtype=np.int64)
        counts[:, 3:N - 3] = rng.choice([0, 1, 3], size=(B, N - 6))
        ctrl = np.array([[[tt * 100 + i + k * 0.25 for k in range(3)] for i in range(N)] for tt in range(t, t + B)])
        pv = [[tt * 1000 + i * 10 + j + q * 0.125 for q in range(6)] for tt in range(t, t + B) for i in range(N) for j in range(counts[tt - t, i])]
        obs = [[tt * 7 + j + q * 0.5 for q in range(9)] for tt in range(t, t + B) for j in range(n_obs)]
        goff = np.concatenate([[0], np.cumsum(counts.reshape(-1))]).astype(np.int32)
        parts.append(synth.Batch(ctrl, goff, np.array(pv).reshape(-1, 6), np.zeros(len(pv), dtype=np.uint8),
                                 (np.arange(B + 1) * n_obs).astype(np.int32), np.array(obs).reshape(-1, 9),
                                 np.array([[1.0 + tt, 2.0 + tt, 3.0 + tt, 4.0 + tt] for tt in range(t, t + B)])))
        lines += [f"{N} {n_obs} " + " ".join(str(int(c)) for c in counts[b]) for b in range(B)]
        t += B
    pb, rows = synth.pad_batches(parts)
    r = subprocess.run([exe], input="16\n" + "\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    nums = lambda line, dtype: np.array(line.split(), dtype=dtype)
    assert out[0] == "5 16" and pb.ctrl.shape == (5, 16, 3)
    assert np.array_equal(nums(out[1], np.int32), pb.n_pts)
    assert np.array_equal(nums(out[2], np.float64), pb.ctrl.reshape(-1))
    assert np.array_equal(nums(out[3], np.int32), pb.guide_off)
    assert np.array_equal(nums(out[4], np.float64), pb.guide_pv.reshape(-1))
    assert np.array_equal(nums(out[5], np.int32), pb.obs_off)
    assert np.array_equal(nums(out[6], np.float64), pb.obs.reshape(-1))
    assert np.array_equal(nums(out[7], np.float64), pb.weights.reshape(-1))
    assert out[8] == "0"
