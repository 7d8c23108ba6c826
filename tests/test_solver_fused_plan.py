"""-m "not gpu": the fusing rule of vigo_optimize (fuse_optimize, csrc/vigo_solver_plan.hpp) — which plans of two launches
run as ONE launch of k_optimize_fused, with what grid and how much LDS — against a restatement written from its comment,
over the sweep of test_solver_plan.py.  tests/solver_fused_plan_check.cpp is a program of its own: built here with the
address and undefined-behaviour sanitizers, it answers queries from stdin with the header's rule.  plan_optimize's own
answers are test_solver_plan.py's business."""
import os
import subprocess

import pytest

import solver_dispatch_rule as rule
from test_solver_plan import FLAGS, MEMS, MODES, NS, batch_sizes, plan_query

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")


def solo_lds(N, m):
    """the general body on ONE trajectory (fp64 reference order, N <= 32, no obstacle table): per history slot that is
    not in registers (m - 2) a 48-byte record {s[3], y[3]} per free control point, the zero column and 16 bytes of
    {ys, 1/ys}; then m alphas"""
    return max(m - 2, 0) * ((N - 6 + 1) * 48 + 16) + m * 8


def fused(mode, N, B, m, has_obs, pz, sz, S, allow_axis=True):
    """(grid, lds) of the one launch, None where the plan runs as planned.  The calls whose plan is [axis-per-lane,
    general]: fp64 reference order, N <= 32, no obstacle list, no z planning, 0 < B <= SIMD count (known), and the
    axis kernel not switched off."""
    if not (mode == "f64" and N <= 32 and not has_obs and not pz and not sz and 0 < B <= S and allow_axis):
        return None
    return B, max(rule.lds_bytes("f64", N, m, D=1, obs=False), solo_lds(N, m))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("solver_fused_plan") / "solver_fused_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "solver_fused_plan_check.cpp"), "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        answers = r.stdout.split("\n")[:-1]
        assert len(answers) == len(queries)
        return answers
    return ask


def parse(answer):
    """(launches, D of the first, fuse, grid, lds), None for a refused shape"""
    return None if answer == "error" else tuple(int(x) for x in answer.split())


@pytest.fixture(scope="module")
def sweep(ask):
    cases = [(mode, N, B, m, obs, pz, sz, S) for mode in MODES for N in NS for m in MEMS for S in (0, 4, 1024)
             for B in batch_sizes(S) for obs in (0, 1) for pz, sz in FLAGS]
    return cases, [parse(a) for a in ask([plan_query(*c) for c in cases])]


def test_rule_equals_the_restatement(sweep):
    cases, got = sweep
    assert len(cases) == 3 * len(NS) * len(MEMS) * (3 + 10 + 10) * 2 * 3
    n_fused = 0
    for c, g in zip(cases, got):
        want = fused(*c)
        if g is None:
            assert want is None and rule.plan(*c) is None, c
            continue
        count, d_first, fuse, grid, lds = g
        assert bool(fuse) == (want is not None), c
        assert bool(fuse) == (d_first == 1), c            # fuses exactly when the plan's first launch is D = 1
        if fuse:
            n_fused += 1
            assert count == 2 and (grid, lds) == want and grid == c[2], c
            assert lds <= rule.LDS // 8, c                # two waves per SIMD: eight workgroups per CU
        else:
            assert (grid, lds) == (0, 0), c
    assert n_fused > 0


def test_the_dev_switch_and_an_unknown_simd_count_do_not_fuse(ask):
    cases = [(mode, N, B, 16, 0, 0, 0, S, axis) for mode in MODES for N in (8, 32, 33) for S in (0, 1024) for B in (1, 40, 1024, 1025)
             for axis in (0, 1)]
    for c, a in zip(cases, ask([plan_query(*c) for c in cases])):
        count, d_first, fuse, grid, lds = parse(a)
        assert bool(fuse) == (fused(*c) is not None) == (d_first == 1), c


def test_lds_of_the_fused_launch(ask):
    cases = [(N, m) for N in range(7, 33) for m in range(1, 17)]
    got = [int(a) for a in ask([f"S {N} {m}" for N, m in cases])]
    assert got == [solo_lds(N, m) for N, m in cases]
    assert dict(zip(cases, got))[(32, 16)] == 14 * (27 * 48 + 16) + 128 == 18496
    # every N <= 32 and mem_size <= 16: the fused launch's LDS is the larger layout's and leaves room for eight per CU
    plans = ask([plan_query("f64", N, 40, m, 0, 0, 0, 1024) for N, m in cases])
    for (N, m), a, solo in zip(cases, plans, got):
        count, d_first, fuse, grid, lds = parse(a)
        assert fuse == 1 and grid == 40, (N, m)
        assert lds == max(rule.lds_bytes("f64", N, m, D=1, obs=False), solo) <= rule.LDS // 8, (N, m)
    assert parse(ask([plan_query("f64", 32, 1024, 16, 0, 0, 0, 1024)])[0]) == (2, 1, 1, 1024, 18496)
