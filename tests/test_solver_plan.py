"""-m "not gpu": the launch plan of vigo_optimize (csrc/vigo_solver_plan.hpp) against its independent restatement
(tests/solver_dispatch_rule.py) and against the dispatch matrix that test_gpu_solver_dispatch.py runs on the device.
tests/solver_plan_check.cpp is a program of its own: built here with the address and undefined-behaviour sanitizers, it
answers queries from stdin with the header's plan."""
import itertools
import os
import subprocess

import pytest

import solver_dispatch_rule as rule

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")
MODES = ("f64", "fast", "f32")
NS = (7, 8, 31, 32, 33, 63, 64, 65, 128, 129, 200, 216, 217, 256)
MEMS = (1, 2, 3, 5, 6, 7, 8, 16)
FLAGS = ((0, 0), (1, 0), (0, 1))          # (plan_in_z, strict_z)


def batch_sizes(S):
    """every threshold of the rule on both sides: trajectories and waves (of one or two) against the SIMD count"""
    if S == 0:
        return (1, 40, 5000)
    return sorted({b for b in (1, 2, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, 2 * S + 2, 16 * S) if b > 0})


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("solver_plan") / "solver_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "solver_plan_check.cpp"), "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        answers = r.stdout.split("\n")[:-1]
        assert len(answers) == len(queries)
        return answers
    return ask


def plan_query(mode, N, B, m, has_obs, pz, sz, S, allow_axis=True):
    return f"P {N} {B} {rule.PREC[mode]} {int(has_obs)} {pz} {sz} {m} {S} {int(allow_axis)}"


def parse_plan(answer):
    """[(precision, GROUP, PPL, WPS, OBS, D, RH, grid, lds, level_waves_elsewhere)], None for a refused shape"""
    return None if answer == "error" else [tuple(int(x) for x in l.split()) for l in answer.split(";")]


def expected(mode, N, launches):
    """the restatement's launches in the form of parse_plan"""
    if launches is None:
        return None
    return [(rule.PREC[mode],) + rule.shape_for(N) + (l.wps, int(l.obs), l.D, l.rh, l.grid, l.lds, l.level_waves_elsewhere) for l in launches]


@pytest.fixture(scope="module")
def sweep(ask):
    cases = [(mode, N, B, m, obs, pz, sz, S) for mode in MODES for N in NS for m in MEMS for S in (0, 4, 1024)
             for B in batch_sizes(S) for obs in (0, 1) for pz, sz in FLAGS]
    return cases, [parse_plan(a) for a in ask([plan_query(*c) for c in cases])]


def test_plan_equals_the_restatement(sweep):
    cases, plans = sweep
    assert len(cases) == 3 * len(NS) * len(MEMS) * (3 + 10 + 10) * 2 * 3
    for c, got in zip(cases, plans):
        assert got == expected(c[0], c[1], rule.plan(*c)), f"(mode, N, B, mem_size, obstacles, plan_in_z, strict_z, SIMDs) = {c}"
    assert any(p is None for p in plans) and any(p is not None and len(p) == 2 for p in plans)


def test_unknown_simd_count_and_the_dev_switch_keep_the_axis_kernel_out(ask):
    cases = [(mode, N, B, 16, 0, 0, 0, S, axis) for mode in MODES for N in (8, 32, 33) for S in (0, 1024) for B in (1, 40, 1024, 1025)
             for axis in (0, 1)]
    for c, a in zip(cases, ask([plan_query(*c) for c in cases])):
        got = parse_plan(a)
        assert got == expected(c[0], c[1], rule.plan(*c)), c
        mode, N, B, _, _, _, _, S, axis = c
        assert (got[0][5] == 1) == (mode == "f64" and N <= 32 and S > 0 and B <= S and axis == 1), c
        assert all(l[3] == 1 for l in got) or S > 0, c


def test_lds_requirement_equals_the_restatement(ask):
    cases = [(N, m, mode) for mode in MODES for m in range(1, 17) for N in range(7, 257)]
    got = [int(a) for a in ask([f"R {N} {m} {rule.PREC[mode]}" for N, m, mode in cases])]
    assert got == [rule.lds_bytes(mode, N, m) for N, m, mode in cases]
    fits = {c: g <= rule.LDS for c, g in zip(cases, got)}
    for mode in ("f64", "fast"):          # include/vigo.h
        assert max(N for N in range(7, 257) if fits[(N, 16, mode)]) == 216


def test_every_key_is_selected_and_every_selected_key_is_listed(ask, sweep):
    keys = [tuple(int(x) for x in k.split()) for k in ask(["K"])[0].split(";")]
    assert len(keys) == 53 and len(set(keys)) == 53
    cases, plans = sweep
    selected = {l[:7] for p in plans if p is not None for l in p}
    assert selected == set(keys), f"never selected: {set(keys) - selected}; not in the list: {selected - set(keys)}"
    restated = {e[:7] for c in cases for e in expected(c[0], c[1], rule.plan(*c)) or []}
    assert restated <= set(keys)


@pytest.mark.parametrize("mode,cell", [pytest.param(m, c, id=f"{m}-{c[0]}") for c in rule.CELLS for m in c[1].split()])
def test_plan_of_each_dispatch_cell_on_the_mi355x(ask, mode, cell):
    _, _, N, _, mem, n_obs, flags, want = cell
    B = rule.cell_batch_size(cell, rule.MI355X_SIMDS)
    got = parse_plan(ask([plan_query(mode, N, B, mem, n_obs > 0, int("plan_in_z" in flags), int("strict_z" in flags), rule.MI355X_SIMDS)])[0])
    assert [(l[3], bool(l[4]), l[5], l[6]) for l in got] == want
    assert all(l[:3] == (rule.PREC[mode],) + rule.shape_for(N) for l in got)
