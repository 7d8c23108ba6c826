"""vigo_traj_validate_host (csrc/vigo_validate_core.hpp compiled for the CPU) on every case of tests/validate_cases.py against
the composition of the oracle by the text of the rule: status, first index, position (bits), dynamic index and the list, the
untouched entries included; at ratio 0 both rules against vgo_traj_collision and vgo_traj_dynamic_collision; the closed form
of the BY_INDEX prefix against the literal loop; the cases' own conditions; the refusals; the per-lane functions walked 64
lanes at a time by a program built with the sanitizers; the header, the exports and the prototype table.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gate_cases as gc
import oracle_lib as ol
import validate_cases as vc
from trajectory_planner_amd import _lib, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "trajectory_planner_amd", "csrc")
CASES = vc.cases()
INVALID_ARG, UNSUPPORTED_N = -1, -4


def assert_same(case, got, want, what):
    assert isinstance(got, dict), f"vigo_traj_validate_host refused {case.name}: {got}"
    bad = vc.same(got, want)
    assert not bad, f"{case.name} {what}: {bad} differ; status {got['status'].tolist()} != {want['status'].tolist()}, first {got['first'].tolist()} != {want['first'].tolist()}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_twin_equals_the_oracle_composition(case):
    assert_same(case, vc.run_host(case), vc.expected_of(case.name), "host twin")


@pytest.mark.parametrize("name", ["mixed:to_65_in_65", "place:by_time", "dyn:before_at_after_the_static_hit", "odd:one_coordinate_not_finite",
                                  "odd:leaving_the_grid"] + [c.name for c in vc.clock_cases()])
def test_at_ratio_0_both_rules_are_the_oracles_gates(name):
    case = vc.by_name(name).with_(ratio=0.0)
    O = ol.oracle()
    g, keep = ol.make_grid(case.world)
    for rule in vc.RULES:
        got = vc.run_host(case, rule=rule)
        for b in range(case.B):
            n = case.n_of(b)
            c, o = np.ascontiguousarray(case.ctrl[b, :n]), case.obs_of(b)
            fi = C.c_int()
            flag = O.vgo_traj_collision(C.byref(g), n, ol._d(c), case.ts_ctrl, case.dt, C.byref(fi))
            dyn = O.vgo_traj_dynamic_collision(n, ol._d(c), case.ts_ctrl, case.dt, len(o), ol._d(o) if len(o) else None)
            assert (flag, fi.value) == (int(got["status"][b] & vc.STATIC), got["first"][b]), (name, rule, b)
            assert dyn == int(got["dyn_first"][b] >= 0) == (got["status"][b] & vc.DYNAMIC) >> 1, (name, rule, b)


def test_edited_worlds():
    for ec in vc.edit_cases():
        for world in ec.worlds():
            assert_same(ec.case, vc.run_host(ec.case, world=world), vc.expected(ec.case, world=world), "host twin on the edited world")


def test_a_row_does_not_depend_on_its_call():
    """the same rows at Ns = 65 and at Ns = 256, alone, and in reverse order"""
    a, b = vc.by_name("mixed:to_65_in_65"), vc.by_name("mixed:to_65_in_256")
    ea, eb = vc.run_host(a), vc.run_host(b)
    assert not vc.same(ea, eb)
    for r in range(a.B):
        n = a.n_of(r)
        alone = synth.host_traj_validate(a.world, a.ts_ctrl, a.ctrl[r:r + 1, :n], a.dt, not_check_ratio=a.ratio, rule=a.rule)
        for k in ("status", "first", "dyn_first"):
            assert alone[k][0] == ea[k][r], (r, k)
        if ea["first"][r] >= 0:
            assert alone["pos"][0].tobytes() == ea["pos"][r].tobytes()
    rev = vc.run_host(a.with_(ctrl=a.ctrl[::-1], n_pts=a.n_pts[::-1]))
    assert np.array_equal(rev["status"], ea["status"][::-1]) and np.array_equal(rev["first"], ea["first"][::-1])


def test_closed_form_of_the_by_index_prefix():
    """C(n) = min(ceil((1.0 - ratio) * S), S), 0 for a product that is not positive (validate_checked_by_index), against the
    trip count of the literal `for (i = 0; i < (1.0 - ratio) * int(S); ++i)` for every count 4 .. 256 and every ratio; and
    through the host twin on rows that stand still in an all-occupied world: first is 0 exactly when C > 0
    (tests/validate_core_check.cpp holds the library's own function against the literal loop for every count, and
    test_by_index_prefix_on_the_marked_sample probes the library's C sample by sample)"""
    world = gc.empty_world((4, 4, 4), 1.0, (0.0, 0.0, 0.0))
    world.voxels[:] = 1
    ts, dt = 0.2, 0.05
    counts = np.arange(4, 257, dtype=np.int32)
    ctrl = np.full((len(counts), 256, 3), 0.5)
    for ratio in vc.RATIOS + (0.1, 0.9, 0.999, 1e-9):
        lit = [vc.checked_by_index_literal(ratio, vc.n_samples(int(n), ts, dt)) for n in counts]
        got = synth.host_traj_validate(world, ts, ctrl, dt, n_pts=counts, not_check_ratio=ratio, rule=vc.BY_INDEX)
        assert [int(f) for f in got["first"]] == [0 if c > 0 else -1 for c in lit], ratio
        for n, c in zip(counts, lit):
            S = vc.n_samples(int(n), ts, dt)
            x = (1.0 - ratio) * S
            closed = 0 if not x > 0.0 else min(int(np.ceil(x)), S)
            assert closed == c, (ratio, n, closed, c)


def test_by_index_prefix_on_the_marked_sample():
    """the library's C(n), sample by sample: the row's only occupied voxel is sample k's; it is hit for k = C - 1 and not for k = C"""
    for case in vc.place_cases() + vc.ratio_cases():
        if case.rule != vc.BY_INDEX:
            continue
        got = vc.run_host(case)
        for b, k in enumerate(case.notes["k"]):
            if k is None:
                continue
            C_lit = vc.checked_by_index_literal(case.ratio, vc.n_samples(case.n_of(b), case.ts_ctrl, case.dt))
            assert (got["first"][b] == k) == (k < C_lit) and (got["first"][b] == -1) == (k >= C_lit), (case.name, b, k, C_lit)


def test_each_case_is_about_what_its_name_says():
    vc.check_conditions()


def test_the_stream_decoy_gives_another_answer():
    real, decoy, _ = vc.stream_inputs()
    assert set(real) == set(decoy) and all(real[k].shape == decoy[k].shape and real[k].dtype == decoy[k].dtype for k in real)
    a, b = vc.stream_twin(real), vc.stream_twin(decoy)
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, b))
    assert len(set(real["n_pts"].tolist())) == 3 and (a[0] == 0).any() and (a[0] != 0).any()


def test_refusals_of_the_host_twin_write_nothing():
    case = vc.by_name("ratio:0.5_by_index")
    w = case.world
    call = lambda world=w, ts_ctrl=case.ts_ctrl, ctrl=case.ctrl, dt=case.dt, **kw: synth.host_traj_validate(
        world, ts_ctrl, ctrl, dt, **{**dict(n_pts=case.n_pts, not_check_ratio=case.ratio, rule=case.rule), **kw})
    assert isinstance(call(), dict)
    for bad in (0.0, -0.1, np.inf, np.nan):
        assert call(dt=bad) == INVALID_ARG and call(ts_ctrl=bad) == INVALID_ARG
        assert call(world=gc.World(w.voxels, w.origin, bad)) == INVALID_ARG
    for bad in (-0.01, 1.01, np.nan, np.inf):
        assert call(not_check_ratio=bad) == INVALID_ARG
    for bad in (-1, 2, 7):
        assert call(rule=bad) == INVALID_ARG
    assert call(dt=1e-9) == INVALID_ARG                                # more than 2^24 samples
    assert call(ctrl=np.zeros((2, 3, 3)), n_pts=None) == UNSUPPORTED_N
    assert call(ctrl=np.zeros((1, 257, 3)), n_pts=None) == UNSUPPORTED_N
    # straight through the C ABI: sentinel-filled outputs stay as they are
    lib = _lib.load()
    B, Ns = case.B, case.Ns
    vox, origin = np.ascontiguousarray(w.voxels), np.ascontiguousarray(w.origin, dtype=np.float64)
    ctrl, n_pts = np.ascontiguousarray(case.ctrl), np.ascontiguousarray(case.n_pts)
    ints = [np.full(B, vc.SENTINEL_IDX, dtype=np.int32) for _ in range(4)]
    n_inv, pos = np.full(1, vc.SENTINEL_IDX, dtype=np.int32), np.full((B, 3), vc.SENTINEL_POS)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    args = [vox.shape[0], vox.shape[1], vox.shape[2], origin.ctypes.data_as(C.POINTER(C.c_double)), w.res, p(vox), case.ts_ctrl, B, Ns, p(n_pts), p(ctrl),
            case.dt, case.ratio, case.rule, None, None, 0, p(ints[0]), p(ints[1]), p(pos), p(ints[2]), p(ints[3]), p(n_inv)]
    f = lib.vigo_traj_validate_host
    for k, bad in ((0, 0), (1, -1), (2, 0), (3, None), (5, None), (7, -1), (16, -1), (10, None), (17, None), (18, None), (21, None), (22, None)):
        broken = list(args)
        broken[k] = bad
        assert f(*broken) == INVALID_ARG, k
    for k, bad in ((8, 3), (8, 257)):
        broken = list(args)
        broken[k] = bad
        assert f(*broken) == UNSUPPORTED_N, k
    assert all((a == vc.SENTINEL_IDX).all() for a in ints + [n_inv]) and (pos == vc.SENTINEL_POS).all()
    empty = list(args)
    empty[7] = 0
    assert f(*empty) == 0 and n_inv[0] == vc.SENTINEL_IDX              # B == 0: VIGO_OK, the count untouched
    assert f(*args) == 0
    e = vc.expected_of(case.name)
    assert np.array_equal(ints[0], e["status"]) and np.array_equal(ints[3], e["invalid"]) and n_inv[0] == e["n_invalid"][0]
    # the optional outputs may be NULL
    got = vc.run_host(case, out=None, want_pos=False, want_dyn=False, want_list=False)
    assert got["pos"] is None and got["dyn_first"] is None and got["invalid"] is None and np.array_equal(got["first"], e["first"])


def test_per_lane_functions_under_the_sanitizers(tmp_path):
    """tests/validate_core_check.cpp: the kernel's walk over blocks of 64 lanes on the host, every table at its exact size,
    counts at and beyond both ends of 4 .. Ns — address and undefined-behaviour sanitizers on the host code, no GPU"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "validate_core_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-O1", "-I", CSRC,
                    os.path.join(HERE, "validate_core_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    m = re.fullmatch(r"rows (\d+) hits (\d+) differences 0\n", r.stdout)
    assert m and int(m.group(1)) >= 1000 and int(m.group(2)) >= 100, r.stdout


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "vigo_validate.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vigo_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_prototype_table(tmp_path):
    names = declared_symbols()
    assert names == ["vigo_traj_validate", "vigo_traj_validate_host"]
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), f"libvigo_hip.so does not export {n}"
    assert set(names) == set(_lib.VALIDATE_PROTOTYPES) and not set(names) & set(_lib.PROTOTYPES)
    for n in names:
        assert getattr(lib, n).argtypes == _lib.VALIDATE_PROTOTYPES[n][1]
    # the header compiles on its own as C99 and as C++14, and its entry points link
    src = tmp_path / "use_validate.c"
    src.write_text('#include "vigo_validate.h"\nint main(void) { return vigo_traj_validate(0, 0, 7, 0, 0, 0.1, 0.0, VIGO_VALIDATE_BY_INDEX, 0, 0, 0, 0, 0, 0, 0, 0, 0)'
                   ' != VIGO_ERR_INVALID_ARG || VIGO_VALID_BAD_COUNT != 4; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)], check=True)
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-I", inc, str(src)], check=True)
    lib_dir = os.path.join(ROOT, "trajectory_planner_amd", "lib")
    exe = str(tmp_path / "use_validate")
    subprocess.run(["gcc", "-std=c99", "-I", inc, str(src), "-o", exe, "-L", lib_dir, "-lvigo_hip", "-Wl,-rpath," + lib_dir], check=True)
    assert subprocess.run([exe]).returncode == 0                       # a NULL handle is refused; nothing touches a GPU
