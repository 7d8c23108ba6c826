"""-m "not gpu": vigo_update_grid_region's rule before any GPU run.  The library's host twin
(vigo_grid_region_apply_host) against the numpy model of tests/grid_update_cases.py on every case; and
tests/grid_update_check.cpp, a program of its own built here with the address and undefined-behaviour sanitizers, which walks
the kernels' word functions (csrc/vigo_grid_update_core.hpp) over a packed snapshot thread index by thread index — its words
against sharding.pack_grid_reference of the expected bytes."""
import os
import subprocess

import numpy as np
import pytest

import grid_update_cases as gc
from trajectory_planner_amd import synth
from trajectory_planner_amd.sharding import pack_grid_reference

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "trajectory_planner_amd", "csrc")
CODES = {"OK": 0, "INVALID_ARG": -1, "UNSUPPORTED": -6}

CASES = gc.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def expected():
    return {c.name: gc.expected(c) for c in CASES}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid_update") / "grid_update_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1",
                    "-I", CSRC, os.path.join(HERE, "grid_update_check.cpp"), "-o", exe], check=True)

    def walk(vox, updates):
        """[(RegionCheck, packed words)] after each update"""
        msg = [np.array(list(vox.shape) + [len(updates)], dtype=np.int32).tobytes(), pack_grid_reference(vox).tobytes()]
        for u in updates:
            r = (0, 0, 0) if u.r is None else u.r
            msg.append(np.array(list(u.lo) + list(u.box.shape) + [u.r is not None] + list(r), dtype=np.int32).tobytes())
            msg.append(np.ascontiguousarray(u.box).tobytes())
        p = subprocess.run([exe], input=b"".join(msg), capture_output=True)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        words = pack_grid_reference(vox).size
        out = np.frombuffer(p.stdout, dtype=np.int32).reshape(len(updates), 1 + words)
        return [(int(row[0]), row[1:]) for row in out]
    return walk


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_twin_equals_the_numpy_model(case, expected):
    cur = case.vox
    for k, (u, want) in enumerate(zip(case.updates, expected[case.name])):
        rc, cur = synth.host_grid_region_apply(cur, u.lo, u.box, u.r)
        assert rc == 0
        assert np.array_equal(cur, want), f"update {k} (lo {u.lo}, n {u.box.shape}, r {u.r})"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_word_functions_walked_on_the_cpu_equal_the_packed_expectation(case, expected, walk):
    got = walk(case.vox, case.updates)
    for k, ((rc, words), want, u) in enumerate(zip(got, expected[case.name], case.updates)):
        assert rc == (1 if 0 in u.box.shape else 0)              # kRegionEmpty / kRegionOk
        assert np.array_equal(words, pack_grid_reference(want)), f"update {k} (lo {u.lo}, n {u.box.shape}, r {u.r})"


@pytest.mark.parametrize("case", [c for c in CASES if not c.name.startswith("sweep")], ids=lambda c: c.name)
def test_raw_mode_is_plain_assignment(case):
    for u in case.updates:
        if u.r is not None or 0 in u.box.shape:
            continue
        rc, got = synth.host_grid_region_apply(case.vox, u.lo, u.box, None)
        want = case.vox.copy()
        want[tuple(slice(l, l + n) for l, n in zip(u.lo, u.box.shape))] = u.box
        assert rc == 0 and np.array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inflate_mode_on_an_inflated_grid_equals_whole_grid_inflation(case):
    """plane 0 = the r-dilation of plane 2 before => the same after: the grid vigo_inflate_grid makes of the updated bytes"""
    for u in case.updates:
        if u.r is None or 0 in u.box.shape:
            continue
        before = gc.inflated(case.vox, u.r)
        rc, got = synth.host_grid_region_apply(before, u.lo, u.box, u.r)
        assigned = before.copy()
        assigned[tuple(slice(l, l + n) for l, n in zip(u.lo, u.box.shape))] = u.box
        assert rc == 0 and np.array_equal(got, gc.inflated(assigned, u.r)), f"lo {u.lo}, n {u.box.shape}, r {u.r}"


def test_removed_obstacle_keeps_the_halo_of_the_one_that_remains(expected):
    c = gc.removed_obstacle_case()
    rc, got = synth.host_grid_region_apply(c.vox, c.updates[0].lo, c.updates[0].box, c.updates[0].r)
    assert rc == 0 and np.array_equal(got, expected[c.name][0])
    assert c.vox[4, 3, 21] & 1 and c.vox[4, 3, 19] & 1 and c.vox[4, 3, 20] == 5
    assert got[4, 3, 21] & 1                                      # still within r of B = (4,3,22)
    assert not got[4, 3, 19] & 1 and not got[4, 3, 20] & 1 and not got[3, 2, 20] & 1
    assert got[4, 3, 20] == 0 and got[4, 3, 22] == 5 and got[1, 1, 5] == 2


def test_sequence_keeps_the_grid_inflated(expected):
    """after 20 mixed updates bit 0 is still the r-dilation wherever an inflate update or nothing touched it: the final grid of
    the all-inflate variant of the sequence equals the inflation of its bytes"""
    c = gc.sequence_case()
    cur = c.vox
    for u in c.updates:
        rc, cur = synth.host_grid_region_apply(cur, u.lo, u.box, gc.SEQUENCE_R)
        assert rc == 0
    assert np.array_equal(cur, gc.inflated(cur, gc.SEQUENCE_R))


@pytest.mark.parametrize("name,lo,n,r,code", gc.ERROR_ARGS, ids=[e[0] for e in gc.ERROR_ARGS])
def test_error_codes_and_nothing_written(name, lo, n, r, code, walk):
    vox = gc.random_bytes(np.random.default_rng(5), gc.ERROR_DIMS)
    box = np.full([max(v, 0) for v in n], 7, dtype=np.uint8)
    import ctypes as C
    from trajectory_planner_amd import _lib
    out = vox.copy()
    i3 = lambda v: (C.c_int32 * 3)(*v)
    rc = _lib.load().vigo_grid_region_apply_host(*vox.shape, out.ctypes.data_as(C.c_void_p), i3(lo), i3(n), C.c_void_p(box.ctypes.data or 1),
                                                 None if r is None else i3(r))
    assert rc == CODES[code] and np.array_equal(out, vox)
    (check, words), = walk(vox, [gc.Update(lo, box, r)]) if min(n) >= 0 else [(2, pack_grid_reference(vox))]
    assert check == {"INVALID_ARG": 2, "UNSUPPORTED": 3}[code] and np.array_equal(words, pack_grid_reference(vox))


def test_null_arguments_and_empty_boxes():
    import ctypes as C
    from trajectory_planner_amd import _lib
    lib = _lib.load()
    vox = gc.random_bytes(np.random.default_rng(6), gc.ERROR_DIMS)
    out = vox.copy()
    p, box = out.ctypes.data_as(C.c_void_p), np.zeros(8, dtype=np.uint8)
    b = C.c_void_p(box.ctypes.data)
    i3 = lambda v: (C.c_int32 * 3)(*v)
    lo, n = i3((1, 1, 1)), i3((2, 2, 2))
    assert lib.vigo_grid_region_apply_host(9, 7, 41, None, lo, n, b, None) == -1
    assert lib.vigo_grid_region_apply_host(9, 7, 41, p, None, n, b, None) == -1
    assert lib.vigo_grid_region_apply_host(9, 7, 41, p, lo, None, b, None) == -1
    assert lib.vigo_grid_region_apply_host(9, 7, 41, p, lo, n, None, None) == -1
    assert lib.vigo_grid_region_apply_host(0, 7, 41, p, lo, n, b, None) == -1
    for empty in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        assert lib.vigo_grid_region_apply_host(9, 7, 41, p, lo, i3(empty), b, i3((1, 1, 1))) == 0
    assert np.array_equal(out, vox)


# ---- the facade's side: the dirty journal and the sub-box rasterisation (host library, no GPU) ---------------------------
HOST_LIB = os.path.join(HERE, "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")


def journal(recorded, since, now):
    """vigo_host_dirty_journal: None when changesSince is false, else [(version, index of the record)]"""
    import ctypes as C
    lib = C.CDLL(HOST_LIB)
    lib.vigo_host_dirty_journal.restype = C.c_int
    lib.vigo_host_dirty_journal.argtypes = [C.c_int, C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_void_p, C.c_void_p]
    rec = np.array(recorded, dtype=np.uint64)
    vers, idx = np.zeros(32, dtype=np.uint64), np.zeros(32, dtype=np.int32)
    k = lib.vigo_host_dirty_journal(len(rec), rec.ctypes.data, since, now, 32, vers.ctypes.data, idx.ctypes.data)
    assert k >= -1, k
    return None if k < 0 else list(zip(vers[:k].tolist(), idx[:k].tolist()))


def test_dirty_journal_complete_run():
    assert journal([2, 3, 4], 1, 4) == [(2, 0), (3, 1), (4, 2)]
    assert journal([2, 3, 4], 2, 4) == [(3, 1), (4, 2)]
    assert journal([2, 3, 4], 3, 4) == [(4, 2)]
    assert journal([2, 3, 4], 4, 4) == []                       # nothing to send, and no hole
    assert journal([2, 3, 4], 4, 5) is None                     # version 5 was never recorded
    assert journal([2, 3, 4], 5, 4) is None


def test_dirty_journal_hole_left_by_a_bare_bump():
    rec = [2, 4, 5]                                              # version 3: a bare ++version
    assert journal(rec, 1, 5) is None and journal(rec, 2, 5) is None and journal(rec, 2, 4) is None
    assert journal(rec, 3, 5) == [(4, 1), (5, 2)] and journal(rec, 1, 2) == [(2, 0)]


def test_dirty_journal_more_than_16_entries():
    rec = list(range(2, 22))                                     # 20 entries: the ring holds versions 6 .. 21
    assert journal(rec, 5, 21) == [(v, v - 2) for v in range(6, 22)]
    assert journal(rec, 4, 21) is None and journal(rec, 1, 21) is None and journal(rec, 4, 10) is None
    assert journal(rec, 20, 21) == [(21, 19)]


def test_dirty_journal_since_zero_is_never_complete():
    assert journal([1, 2], 0, 2) is None and journal([], 0, 0) is None and journal([1], 0, 1) is None


RB_DIMS, RB_ORIGIN, RB_RES = (24, 20, 10), np.array([-1.5, -1.25, 0.0]), 0.125   # every coordinate exact in binary
RB_REGIONS = {"aligned": ([-1.0, -0.75, 0.125], [1.0, 0.75, 1.0]), "unaligned": ([-0.93, -0.77, 0.13], [1.04, 0.81, 0.97]),
              "beyond_the_map": ([-1.7, -0.3, -0.2], [0.4, 1.6, 0.6])}
RB_SUBS = {"inside": ([-0.4, -0.3, 0.3], [0.2, 0.1, 0.6]), "one_voxel": ([0.01, 0.01, 0.51], [0.02, 0.02, 0.52]),
           "on_the_min_faces": ("min", [-0.5, -0.4, 0.4]), "on_the_max_faces": ([0.3, 0.2, 0.5], "max"), "the_region": ("min", "max"),
           "partly_outside": ([-2.0, -0.2, -1.0], [-0.6, 0.3, 0.4]), "around_the_region": ([-5.0, -5.0, -5.0], [5.0, 5.0, 5.0]),
           "wholly_outside": ([1.2, -0.2, 0.2], [1.4, 0.2, 0.6]), "outside_in_z_only": ([-0.2, -0.2, 1.1], [0.2, 0.2, 1.2])}


@pytest.mark.parametrize("rname", list(RB_REGIONS))
@pytest.mark.parametrize("sname", list(RB_SUBS))
def test_rasterise_box_patch_equals_the_whole_rasterised_again(rname, sname):
    import ctypes as C
    lib = C.CDLL(HOST_LIB)
    rmin, rmax = (np.array(v, dtype=np.float64) for v in RB_REGIONS[rname])
    smin, smax = RB_SUBS[sname]
    smin = rmin.copy() if isinstance(smin, str) else np.array(smin, dtype=np.float64)
    smax = rmax.copy() if isinstance(smax, str) else np.array(smax, dtype=np.float64)
    rng = np.random.default_rng(len(rname) * 100 + len(sname))
    vox = gc.random_bytes(rng, RB_DIMS, 0.0) & np.uint8(3)
    # the sub-box and the region in voxels of the zero-based lattice; the edit: new bytes for the map's voxels the sub-box touches
    key = lambda v, f: f(v / RB_RES).astype(np.int64)
    s0, s1, r0, r1 = key(smin, np.floor), key(smax, np.ceil), key(rmin, np.floor), key(rmax, np.ceil)
    m0 = key(RB_ORIGIN, np.floor)
    e0, e1 = np.clip(s0 - m0, 0, RB_DIMS), np.clip(s1 - m0, 0, RB_DIMS)
    edit_n = np.maximum(e1 - e0, 0).astype(np.int32)
    edit_lo = np.where(edit_n > 0, e0, 0).astype(np.int32)
    if 0 in edit_n:
        edit_n[:] = 0
    edit = (gc.random_bytes(rng, tuple(edit_n), 0.0) ^ np.uint8(1)) & np.uint8(3)
    c0, c1 = np.maximum(s0, r0), np.minimum(s1, r1)
    want_n = np.maximum(c1 - c0, 0) if (c1 > c0).all() else np.zeros(3, dtype=np.int64)
    want_lo = (c0 - r0) if want_n.all() else np.zeros(3, dtype=np.int64)
    cap = int(np.prod(r1 - r0))
    dims, lo, n = (np.zeros(3, dtype=np.int32) for _ in range(3))
    patched, whole = np.zeros(cap, dtype=np.uint8), np.ones(cap, dtype=np.uint8)
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.c_void_p)
    lib.vigo_host_rasterise_box.restype = C.c_int
    lib.vigo_host_rasterise_box.argtypes = [C.c_int] * 3 + [C.c_void_p, C.c_double] + [C.c_void_p] * 8 + [C.c_longlong] + [C.c_void_p] * 5
    rc = lib.vigo_host_rasterise_box(*RB_DIMS, dp(RB_ORIGIN), RB_RES, vox.ctypes.data, dp(rmin), dp(rmax), edit_lo.ctypes.data, edit_n.ctypes.data,
                                     np.ascontiguousarray(edit).ctypes.data or 1, dp(smin), dp(smax), cap, dims.ctypes.data, lo.ctypes.data,
                                     n.ctypes.data, patched.ctypes.data, whole.ctypes.data)
    assert rc == 0
    assert dims.tolist() == (r1 - r0).tolist() and n.tolist() == want_n.tolist() and lo.tolist() == want_lo.tolist()
    assert np.array_equal(patched, whole)
    if sname in ("wholly_outside", "outside_in_z_only") and rname != "beyond_the_map":
        assert not n.any()
    if sname in ("inside", "one_voxel", "the_region", "partly_outside"):
        assert n.all()
    # the whole is the map seen through the four methods: bits 0, 1 of the edited map, 3 outside it
    after = vox.copy()
    after[tuple(slice(l, l + k) for l, k in zip(edit_lo, edit_n))] = edit
    pad = np.full(tuple(r1 - r0), 7, dtype=np.uint8)
    a, b = np.maximum(r0, m0), np.minimum(r1, m0 + RB_DIMS)
    src = after[tuple(slice(x - m, y - m) for x, y, m in zip(a, b, m0))]
    pad[tuple(slice(x - r, y - r) for x, y, r in zip(a, b, r0))] = (src & 3) | ((src & 1) << 2)
    assert np.array_equal(whole.reshape(pad.shape), pad)
