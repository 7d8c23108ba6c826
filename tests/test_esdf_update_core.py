"""-m "not gpu": the rule of the ESDF region update (csrc/vigo_esdf_core.hpp, "Region update") before any GPU run.  The host
twin vigo_esdf_update_host on every case of tests/esdf_update_cases.py: its A, B and lattice against the tracked host build
of the final grid, that lattice against the existing vigo_esdf_from_voxels_host and the all-pairs definition, its line
counts against a numpy count made from the tracked arrays of the old and the new grid; the twins' error codes; and
tests/esdf_update_check.cpp, a program of its own built here with the address and undefined-behaviour sanitizers, which
walks the kernels' per-thread functions over the launches' own grids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import esdf_build_cases as ec
import esdf_update_cases as uc
from trajectory_planner_amd import _lib, synth

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")
BRUTE_MAX_VOXELS = 20000          # every shape of uc.SHAPES; not the 64^3 world


def tracked(vox, case):
    rc, a, b, lat = synth.host_esdf_tracked(vox, case.plane, case.unk, uc.res_of(case))
    assert rc == 0, rc
    return a, b, lat


@pytest.mark.parametrize("name", uc.NAMES)
def test_update_equals_the_tracked_build_of_the_new_grid(name):
    """after every refresh: A, B, lattice == a tracked host build of that grid; the line counts == the lines on which the
    tracked arrays of the grid before and after differ"""
    case = uc.by_name(name)
    a0, b0, l0 = uc.tracked_start(case.start, case.plane, case.unk)
    for k, ((vox, a, b, lat, stats), (_, lo, n)) in enumerate(zip(uc.chain(name), uc.refreshes(case))):
        a1, b1, l1 = tracked(vox, case)
        assert np.array_equal(a, a1) and np.array_equal(b, b1) and ec.same_bits(lat, l1), (name, k)
        y_lines = int((a0 != a1).any(axis=1).sum())           # lines (x, z) of the z-pass result
        x_lines = int((b0 != b1).any(axis=0).sum())           # lines (y, z) of the y-pass result
        print(name, k, stats, "numpy count:", y_lines, x_lines)
        assert (stats["y_lines"], stats["x_lines"]) == (y_lines, x_lines), (name, k)
        if 0 in n:
            assert stats["box_n"] == (0, 0, 0) and stats["box_lo"] == (0, 0, 0)
        else:
            assert stats["box_lo"] == tuple(lo) and stats["box_n"] == tuple(n)
        if case.zero_lines:
            assert y_lines == 0 and x_lines == 0 and ec.same_bits(lat, l0), (name, k)
        if case.interior:
            assert x_lines <= vox.shape[1] * vox.shape[2] // 4, (name, x_lines)
        a0, b0, l0 = a1, b1, l1


@pytest.mark.parametrize("name", uc.NAMES)
def test_updated_lattice_equals_the_untracked_twin_and_the_all_pairs_definition(name):
    case = uc.by_name(name)
    vox, _, _, lat, _ = uc.chain(name)[-1]
    rc, want = ec.host_twin_raw(vox, case.plane, case.unk, uc.res_of(case))
    assert rc == 0 and ec.same_bits(lat, want), name
    if vox.size <= BRUTE_MAX_VOXELS:
        assert ec.same_bits(lat, ec.brute_lattice(vox, case.plane, case.unk, uc.res_of(case))), name


def test_the_cases_change_something():
    """the first site and its removal move the sentinel: every x line is flagged; the unknown bit changes sites only with
    unknown_is_site; a three-update case is refreshed once with the union box"""
    first, removed = uc.chain("5x7x33_first_site_then_removed")
    assert first[4]["x_lines"] == 7 * 33 and removed[4]["x_lines"] == 7 * 33
    E = 5 * 5 + 7 * 7 + 33 * 33
    assert np.all(removed[3] == np.float32(np.sqrt(float(E)) * 0.1)) and not np.all(first[3] == removed[3])
    assert uc.chain("5x7x33_unknown_bit_is_site")[-1][4]["x_lines"] > 0
    assert uc.chain("5x7x33_unknown_bit_is_no_site")[-1][4]["x_lines"] == 0
    (_, lo, n), = uc.refreshes(uc.by_name("9x70x31_three_updates_one_refresh"))
    assert (lo, n) == ((0, 0, 0), (9, 70, 31))
    (_, lo, n), = uc.refreshes(uc.by_name("9x70x31_plane0_inflate_edge"))
    assert (lo, n) == ((6, 65, 26), (3, 5, 5))                 # grown by 1 and clipped at the far faces
    assert len(uc.chain("world64_update_refresh_update_refresh")) == 4


def test_tracked_twin_refuses_what_the_untracked_one_refuses():
    lib = _lib.load()
    vox = np.zeros((4, 4, 4), dtype=np.uint8)
    a, b = np.full((4, 4, 4), 5, dtype=np.int32), np.full((4, 4, 4), 6, dtype=np.int32)
    out = np.full((4, 4, 4), 7.0, dtype=np.float32)
    pv, pa, pb, po = (x.ctypes.data_as(C.c_void_p) for x in (vox, a, b, out))
    f = lib.vigo_esdf_from_voxels_host_tracked
    for plane in (1, 3, -1):
        assert f(4, 4, 4, pv, plane, 0, 0.1, pa, pb, po) == -1
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4)):
        assert f(*dims, pv, 2, 0, 0.1, pa, pb, po) == -1, dims
    for args in ((None, pa, pb, po), (pv, None, pb, po), (pv, pa, None, po), (pv, pa, pb, None)):
        assert f(4, 4, 4, args[0], 2, 0, 0.1, *args[1:]) == -1
    for res in (0.0, -0.1, float("nan"), float("inf")):
        assert f(4, 4, 4, pv, 2, 0, res, pa, pb, po) == -1, res
    assert f(40000, 2, 2, pv, 2, 0, 0.1, pa, pb, po) == -6 and f(2048, 2048, 2049, pv, 2, 0, 0.1, pa, pb, po) == -6
    assert np.all(a == 5) and np.all(b == 6) and np.all(out == 7.0)                        # nothing was written
    assert f(4, 4, 4, pv, 2, 0, 0.1, pa, pb, po) == 0 and np.all(a == 48) and np.all(b == 48)   # no site: E = 48 everywhere


def test_update_twin_error_codes_and_nothing_written():
    lib = _lib.load()
    vox = ec.case("5x7x33-rand50")[0]
    rc, a, b, lat = synth.host_esdf_tracked(vox, 2, False, 0.1)
    assert rc == 0
    keep = a.copy(), b.copy(), lat.copy()
    new = vox.copy()
    new[1:3, 2:4, 5:9] ^= 4
    pv, pa, pb, pl = (x.ctypes.data_as(C.c_void_p) for x in (new, a, b, lat))
    i3 = lambda v: (C.c_int32 * 3)(*v)
    st = _lib.VigoEsdfUpdateStats()
    f = lib.vigo_esdf_update_host
    lo, n = i3((1, 2, 5)), i3((2, 2, 4))
    assert f(5, 7, 33, None, 2, 0, 0.1, lo, n, pa, pb, pl, st) == -1
    assert f(5, 7, 33, pv, 2, 0, 0.1, None, n, pa, pb, pl, st) == -1 and f(5, 7, 33, pv, 2, 0, 0.1, lo, None, pa, pb, pl, st) == -1
    assert f(5, 7, 33, pv, 2, 0, 0.1, lo, n, None, pb, pl, st) == -1 and f(5, 7, 33, pv, 2, 0, 0.1, lo, n, pa, None, pl, st) == -1
    assert f(5, 7, 33, pv, 2, 0, 0.1, lo, n, pa, pb, None, st) == -1
    assert f(5, 7, 33, pv, 1, 0, 0.1, lo, n, pa, pb, pl, st) == -1 and f(5, 1, 33, pv, 2, 0, 0.1, lo, n, pa, pb, pl, st) == -1
    assert f(5, 7, 33, pv, 2, 0, float("nan"), lo, n, pa, pb, pl, st) == -1
    for blo, bn in (((-1, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, -1, 1)), ((4, 0, 0), (2, 1, 1)), ((0, 0, 32), (1, 1, 2)), ((0, 8, 0), (1, 0, 1))):
        assert f(5, 7, 33, pv, 2, 0, 0.1, i3(blo), i3(bn), pa, pb, pl, st) == -1, (blo, bn)
    assert f(40000, 2, 2, pv, 2, 0, 0.1, i3((0, 0, 0)), i3((1, 1, 1)), pa, pb, pl, st) == -6
    assert all(np.array_equal(x, y) for x, y in zip((a, b, lat), keep))                   # nothing was written
    # a zero extent: OK, nothing changes, the stats are zeros — although the grid differs
    st.y_lines = 9
    assert f(5, 7, 33, pv, 2, 0, 0.1, lo, i3((2, 0, 4)), pa, pb, pl, st) == 0 and st.as_dict() == dict(box_lo=(0, 0, 0), box_n=(0, 0, 0), y_lines=0, x_lines=0)
    assert all(np.array_equal(x, y) for x, y in zip((a, b, lat), keep))
    # stats may be NULL; the update itself
    assert f(5, 7, 33, pv, 2, 0, 0.1, lo, n, pa, pb, pl, None) == 0
    rc, a1, b1, l1 = synth.host_esdf_tracked(new, 2, False, 0.1)
    assert np.array_equal(a, a1) and np.array_equal(b, b1) and ec.same_bits(lat, l1)


# ---- the kernels' per-thread functions, walked over the launches' own grids under the sanitizers -------------------------
WALKED = [n for n in uc.NAMES if not n.startswith("world64")] + ["world64_fill_30_20_40_n4", "world64_three_updates_one_refresh"]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("esdf_update") / "esdf_update_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "esdf_update_check.cpp"), "-o", exe], check=True)

    def walk(case):
        """[(y_lines, x_lines, a, b, lattice)] after each refresh"""
        vox = uc.start_grid(case)
        refreshes = uc.refreshes(case)
        msg = [np.array(list(vox.shape) + [case.plane, int(case.unk), len(refreshes)], dtype=np.int32).tobytes(),
               np.array([uc.res_of(case)], dtype=np.float64).tobytes(), np.ascontiguousarray(vox).tobytes()]
        for (steps, lo, n), (grid, *_) in zip(refreshes, uc.chain(case.name)):
            msg += [np.array(list(lo) + list(n), dtype=np.int32).tobytes(), np.ascontiguousarray(grid).tobytes()]
        p = subprocess.run([exe], input=b"".join(msg), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out, at, v = [], 0, vox.size
        for _ in refreshes:
            counts = np.frombuffer(p.stdout, dtype=np.int64, count=2, offset=at)
            a = np.frombuffer(p.stdout, dtype=np.int32, count=v, offset=at + 16).reshape(vox.shape)
            b = np.frombuffer(p.stdout, dtype=np.int32, count=v, offset=at + 16 + 4 * v).reshape(vox.shape)
            lat = np.frombuffer(p.stdout, dtype=np.float32, count=v, offset=at + 16 + 8 * v).reshape(vox.shape)
            out.append((int(counts[0]), int(counts[1]), a, b, lat))
            at += 16 + 12 * v
        assert at == len(p.stdout)
        return out
    return walk


@pytest.mark.parametrize("name", WALKED)
def test_region_functions_walked_on_the_cpu_equal_the_twin(name, walk):
    """(the program itself compares the walk with the loops, with a rebuild and the bricked field with a whole re-tiling)"""
    for k, ((y_lines, x_lines, a, b, lat), (_, ta, tb, tl, stats)) in enumerate(zip(walk(uc.by_name(name)), uc.chain(name))):
        assert (y_lines, x_lines) == (stats["y_lines"], stats["x_lines"]), (name, k)
        assert np.array_equal(a, ta) and np.array_equal(b, tb) and ec.same_bits(lat, tl), (name, k)
