"""-m "not gpu": the work plan of vigo_bspline_fit_mixed (csrc/vigo_fit_plan.hpp) — which paths are fitted, their regrouping
by point count into wave-groups of up to 5 paths of one K, the launch bound, the operator table's offsets — against a
restatement in Python.  tests/fit_plan_check.cpp is a program of its own: built here with the address and
undefined-behaviour sanitizers, it answers queries from stdin with the header's functions."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")
KMIN, KMAX, BINS, GROUP = 4, 62, 59, 5


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_plan") / "fit_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "fit_plan_check.cpp"), "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        answers = r.stdout.split("\n")[:-1]
        assert len(answers) == len(queries)
        return answers
    return ask


def fitted(K, status, Ns, stride):
    return status == 0 and KMIN <= K <= min(Ns - 2, stride)


def check_plan(ask, Ns, stride, counts, status=None):
    """the plan of one batch, held against the rule: returns (groups, bound)"""
    counts = [int(k) for k in counts]
    T = len(counts)
    status = [0] * T if status is None else [int(s) for s in status]
    a = ask([f"P {Ns} {stride} {T} " + " ".join(f"{k} {s}" for k, s in zip(counts, status))])[0]
    head, bins, groups = a.split("|")
    bound, total = (int(x) for x in head.split())
    bins = [int(x) for x in bins.split()]
    want = [k - KMIN if fitted(k, s, Ns, stride) else -1 for k, s in zip(counts, status)]
    assert bins == want
    groups = [[int(x) for x in g.split()] for g in groups.split(";")] if groups.strip() else []
    assert len(groups) == total
    assert bound == -(-T // GROUP) + BINS and total <= bound
    seen, first_want, last_K = [], 0, 0
    for K, first, members, *who in groups:
        assert 1 <= members <= GROUP and len(who) == members
        assert first == first_want and K >= last_K               # the groups tile the sorted order, bins ascending
        assert all(counts[t] == K and want[t] == K - KMIN for t in who)          # of its own K, fitted
        assert who == sorted(who)
        if seen and counts[seen[-1]] == K:
            assert who[0] > seen[-1]                             # ascending across the groups of a bin as well
        seen += who
        first_want += members
        last_K = K
    assert sorted(seen) == [t for t in range(T) if want[t] >= 0] and len(set(seen)) == len(seen)   # each exactly once
    for K in set(counts[t] for t in seen):                       # ceil(cnt / 5) groups per bin: only the last partly filled
        sizes = [g[2] for g in groups if g[0] == K]
        n = sum(sizes)
        assert len(sizes) == -(-n // GROUP) and all(s == GROUP for s in sizes[:-1])
    return groups, bound


def test_table_offsets_are_disjoint_and_sum_to_the_table(ask):
    nums = [int(x) for x in ask(["O"])[0].split()]
    off, woff, (table, work) = nums[:BINS + 1], nums[BINS + 1:2 * BINS + 2], nums[2 * BINS + 2:]
    sizes = [(K + 4) * (K + 2) for K in range(KMIN, KMAX + 1)]
    assert off[0] == 0 and np.array_equal(np.diff(off), sizes)   # back to back: disjoint, no gap
    assert off[-1] == table == sum(sizes) and table * 8 < 1 << 20
    # the work matrices [A | I], (K + 4) x (2K + 6), laid out alike
    wsizes = [(K + 4) * (2 * K + 6) for K in range(KMIN, KMAX + 1)]
    assert woff[0] == 0 and np.array_equal(np.diff(woff), wsizes) and woff[-1] == work == sum(wsizes)


@pytest.mark.parametrize("Ns,stride", [(64, 70), (64, 40), (32, 128), (7, 1), (7, 9)])
def test_bins_of_1_4_5_6_10_11_paths_with_empty_bins(ask, Ns, stride):
    top = min(Ns - 2, stride)
    ks = [k for k in (4, 5, 12, 30, 31, 47, 62) if k <= top] or [4]
    sizes = [1, 4, 5, 6, 10, 11, 1]
    counts = np.concatenate([np.full(n, k) for k, n in zip(ks, sizes)])
    rng = np.random.default_rng(Ns + stride)
    for order in (counts, counts[::-1], rng.permutation(counts)):
        groups, _ = check_plan(ask, Ns, stride, order)
        if top >= 4:
            per_bin = {k: sorted(g[2] for g in groups if g[0] == k) for k in ks}
            assert per_bin == {k: sorted([GROUP] * (n // GROUP) + ([n % GROUP] if n % GROUP else [])) for k, n in zip(ks, sizes)}
        else:
            assert groups == []


def test_everything_in_one_bin_and_no_path_at_all(ask):
    for T in (1, 5, 6, 1024, 1025):
        groups, bound = check_plan(ask, 64, 256, [30] * T)
        assert len(groups) == -(-T // GROUP) and bound - len(groups) == BINS
    groups, bound = check_plan(ask, 64, 256, [])
    assert groups == [] and bound == BINS
    # every bin with one path over a multiple of five: each ends in a partly filled group
    groups, bound = check_plan(ask, 64, 256, [k for k in range(KMIN, KMAX + 1) for _ in range(6)])
    assert len(groups) == 2 * BINS and len(groups) <= bound


def test_unfitted_paths_get_no_group(ask):
    for Ns, stride in ((64, 70), (32, 128), (64, 20)):
        top = min(Ns - 2, stride)
        bad = [3, Ns - 1, -1, 2 ** 30, -2 ** 31, top + 1, 0]
        rng = np.random.default_rng(Ns)
        good = rng.integers(KMIN, top + 1, size=40).tolist()
        counts = good[:13] + bad + good[13:]
        status = [0] * len(counts)
        for t in (2, 30, 45):
            status[t] = (1, -3, 5)[t % 3]
        groups, _ = check_plan(ask, Ns, stride, counts, status)
        in_groups = {t for g in groups for t in g[3:]}
        assert in_groups == {t for t in range(len(counts)) if status[t] == 0 and KMIN <= counts[t] <= top}
        # the others' groups are those of the batch without the unfitted paths, up to the renumbering
        keep = sorted(in_groups)
        alone, _ = check_plan(ask, Ns, stride, [counts[t] for t in keep])
        assert [[g[0], g[1], g[2]] + [keep[i] for i in g[3:]] for g in alone] == groups
    check_plan(ask, 64, 70, [30, 31], [7, 7])                    # nothing fitted


def test_group_lookup_on_sparse_counts(ask):
    cnt = [0] * BINS
    cnt[0], cnt[26], cnt[27], cnt[58] = 5, 7, 1, 11              # K = 4, 30, 31, 62
    line = " ".join(str(c) for c in cnt)
    got = [tuple(int(x) for x in a.split()) for a in ask([f"G {g} {line}" for g in range(-1, 8)])]
    assert got == [(0, 0, 0), (4, 0, 5), (30, 5, 5), (30, 10, 2), (31, 12, 1), (62, 13, 5), (62, 18, 5), (62, 23, 1), (0, 0, 0)]
