"""-m "not gpu": the workloads of tests/prologue_mixed_cases.py are about what they claim to be about — judged by the host
twins alone (vigo_host_collision_segs_core, vigo_host_path_search_core, vigo_host_guide_core,
vigo_host_rebound_reguide_core, called per count) — and the index arithmetic of the mixed rows
(csrc/vigo_rows_core.hpp) walks the crafted rows between guard bytes under ASan and UBSan, as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import guide_cases as gc
import pathsearch_cases as pc
import prologue_mixed_cases as pm
import reguide_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return pc.host_lib()


@pytest.fixture(scope="module")
def crafted():
    return [pm.crafted_case(ncr) for ncr in pm.NCRS]


def test_the_crafted_batches_are_interleaved_odd_and_cover_the_counts(crafted):
    for case in crafted:
        assert case.counts() == sorted(pm.COUNTS) and len(case.counts()) >= 8 and case.Ns == 120
        assert case.B % 2 == 1
        n = case.n_pts
        assert (n[1:len(pm.COUNTS)] != n[:len(pm.COUNTS) - 1]).all()          # neighbouring rows differ in count
        zero, poison = case.padded(False), case.padded(True)
        for b in range(case.B):
            assert np.array_equal(zero[b, :n[b]], poison[b, :n[b]]) and (zero[b, n[b]:] == 0).all()
            tail = poison[b, n[b]:]
            assert np.isnan(tail).all() if b % 2 == 0 else (np.isfinite(tail).all() and (tail == case.poison_point()).all())


def test_the_crafted_workload_is_about_what_it_claims(lib, crafted):
    with_segments, statuses, merges, last_point, poisoned = set(), set(), 0, set(), 0
    for case in crafted:
        segs = pm.twin_segments_per_count(lib, case)
        paths = pm.twin_paths_per_count(lib, case)
        n = case.n_pts
        for b in range(case.B):
            st, sg = segs[b]
            if len(sg):
                with_segments.add(int(n[b]))
            statuses.add(paths[b][0])
            if st == pc.OK:
                statuses.add(("scan", st))
                # a merge: the walk left fewer segments than the scan found, and they are the merged pairs
                if paths[b][0] == pc.OK and 0 < len(paths[b][1]) < len(sg):
                    merges += 1
            else:
                assert len(sg) == 0 and paths[b][0] == pc.DEFERRED and "zigzag" in case.names[b]
            if "last point" in case.names[b] and pm.end_idx(int(n[b]), case.ncr) - 1 >= 3:
                e = pm.end_idx(int(n[b]), case.ncr)
                # the (start, N - 1) segment and its duplicate, closed at endIdx
                assert [tuple(s) for s in sg] == [(e - 2, int(n[b]) - 1), (e - 2, e)], (case.name, case.names[b], sg)
                last_point.add((int(n[b]), case.ncr))
        # the padding would add segments if it were scanned: the twin on the poisoned row with N = Ns
        ctrl = case.padded(True)
        w = pc.Workload("poisoned rows scanned to Ns", case.vox, case.origin, case.res, ctrl, case.cfg, ncr=case.ncr)
        r, seg_off, seg, st = pc.twin_segments(lib, w)
        assert r == 0
        for b in range(case.B):
            if n[b] < case.Ns and (st[b] != segs[b][0] or not np.array_equal(seg[seg_off[b]:seg_off[b + 1]], segs[b][1])):
                poisoned += 1
        # ... and read at their own count the poisoned rows are the clean ones
        again = pm.twin_segments_per_count(lib, case, ctrl)
        assert all(a[0] == e[0] and np.array_equal(a[1], e[1]) for a, e in zip(again, segs))
    # a trajectory of 7 control points owns no segment under any ratio (endIdx = 3: prologue_mixed_cases' docstring)
    assert with_segments == set(pm.COUNTS) - {7}, with_segments
    assert {pc.OK, pc.FAILED, pc.DEFERRED} <= statuses and merges >= 1
    assert {c for c, _ in last_point} == set(pm.COUNTS) - {7} and len(last_point) >= 2 * len(pm.COUNTS) - 3
    assert poisoned >= 1
    print(f"\ncrafted: counts with segments {sorted(with_segments)}, {merges} merges, {len(last_point)} last-point rows, "
          f"{poisoned} rows whose poisoned padding would add segments")


def test_the_derived_batch_and_the_reguide_rows(lib):
    case, base = pm.derived_case()
    assert 60 <= case.B <= 64 and case.counts() == sorted(pm.DERIVED_COUNTS) and case.Ns == 32
    paths = pm.twin_paths_per_count(lib, case)
    ok = [b for b in range(case.B) if paths[b][0] == pc.OK and len(paths[b][1])]
    assert len(ok) >= 8 and {len(case.rows[b]) for b in ok} == set(pm.DERIVED_COUNTS)
    # the re-guide rows of the crafted batch: every status but DEFERRED comes from the states alone
    glib = rc.host_lib()
    crafted = pm.crafted_case(0.0)
    rows = pm.reguide_rows(lib, crafted)
    seen = set()
    for n in crafted.counts():
        idx, c = rows.uniform(crafted, n)
        t = rc.twin(glib, c, 1, rc.shipped())
        assert t.rc == 0
        seen |= set(int(s) for s in t.status)
    assert seen == {rc.DONE, rc.SEARCH_FAILED, rc.NOT_REQUIRED, rc.DEFERRED, rc.SKIPPED}, seen


def test_index_arithmetic_under_sanitizers(tmp_path):
    """tests/prologue_mixed_check.cpp: row_count, row_offsets and row_slot_owner of csrc/vigo_rows_core.hpp over rows like
    the crafted ones, every array between guard bytes, built with ASan and UBSan and run as a program of its own"""
    exe = tmp_path / "prologue_mixed_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "trajectory_planner_amd", "csrc"), os.path.join(ROOT, "tests", "prologue_mixed_check.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows ok" in r.stdout
