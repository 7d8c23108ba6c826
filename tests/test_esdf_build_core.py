"""-m "not gpu": the rule of the ESDF build (csrc/vigo_esdf_core.hpp) through its host twin
vigo_esdf_from_voxels_host — against the all-pairs brute-force definition on every small shape and content, against
synth.edt_esdf's expression (scipy) on the 64^3 world and the random fills, the empty-set and the padding rule, and the
refused arguments."""
import ctypes as C

import numpy as np
import pytest

import esdf_build_cases as ec
from trajectory_planner_amd import _lib, synth


@pytest.mark.parametrize("name", ec.SMALL_NAMES)
def test_host_twin_equals_the_all_pairs_definition(name):
    vox, plane, unk, res = ec.case(name)
    want = ec.brute_lattice(vox, plane, unk, res)
    got = ec.host_twin(name)
    assert ec.same_bits(got, want), (name, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


@pytest.mark.parametrize("name", ec.WORLD_CASES + [n for n in ec.SMALL_NAMES if n.split("-")[1] in ec.RANDOM_FILLS])
def test_host_twin_equals_the_scipy_expression(name):
    pytest.importorskip("scipy")
    vox, plane, unk, res = ec.case(name)
    s = ec.sites_of(vox, plane, unk)
    got = ec.host_twin(name)
    if not s.any() or s.all():
        # a 2 % or 98 % fill of a handful of voxels can come out with no site or no free voxel; scipy's transform has no
        # defined value for an empty set, so there the twin is held to this library's own: the empty-set rule
        assert name.split("-")[1] in ("rand02", "rand98") and s.size <= 2000
        far = np.float32(np.sqrt(float(sum(n * n for n in s.shape))) * res)
        assert np.all(got == (-far if s.all() else far)), name
        return
    assert ec.same_bits(got, ec.edt_lattice(vox, plane, unk, res)), name


def test_synth_helper_is_the_host_twin_and_equals_edt_esdf():
    pytest.importorskip("scipy")
    w = ec.world64()
    got, origin = synth.host_esdf(w)
    assert ec.same_bits(got, ec.host_twin("world64_p2")) and np.array_equal(origin, w.origin)
    want, _ = synth.edt_esdf(w)
    assert ec.same_bits(got, want)
    # the other planes differ from it: the arguments are not ignored
    assert not ec.same_bits(ec.host_twin("world64_p0"), got) and not ec.same_bits(ec.host_twin("world64_p2_unknown"), got)


@pytest.mark.parametrize("shape", ec.SMALL_SHAPES)
def test_empty_set_rule(shape):
    """no site: d2_site = nx^2 + ny^2 + nz^2 everywhere and d2_free = 0; all sites: the reverse"""
    tag = "x".join(str(n) for n in shape)
    E = float(sum(n * n for n in shape))
    far = np.float32(np.sqrt(E) * 0.1)
    none, full = ec.host_twin(f"{tag}-none"), ec.host_twin(f"{tag}-all")
    assert np.all(none == far) and np.all(full == -far) and np.isfinite(far)


def test_padding_rule():
    """nz = 33 with every voxel a site: the 31 padding bits of the second word are clear in the packed row — they are
    not non-site voxels: d2_free must be nx^2 + ny^2 + nz^2, not the distance to a padding bit (1 at z = 32)."""
    shape = (5, 7, 33)
    vox = np.full(shape, 4, dtype=np.uint8)
    rc, got = ec.host_twin_raw(vox, 2, False, 0.1)
    assert rc == 0
    E = 5 * 5 + 7 * 7 + 33 * 33
    assert np.all(got == np.float32(-np.sqrt(float(E)) * 0.1))
    assert got[0, 0, 32] != np.float32(-0.1)
    # and with no site, padding is no site either: z = 32 is not at distance 1 of one
    rc, got = ec.host_twin_raw(np.zeros(shape, dtype=np.uint8), 2, False, 0.1)
    assert rc == 0 and np.all(got == np.float32(np.sqrt(float(E)) * 0.1))
    # one free voxel next to the padding: distances are measured to it, along z too
    vox[2, 3, 32] = 0
    rc, got = ec.host_twin_raw(vox, 2, False, 1.0)
    assert rc == 0 and got[2, 3, 32] == 1.0 and got[2, 3, 31] == -1.0 and got[2, 3, 0] == -32.0


def test_unknown_flag_and_plane_select_the_sites():
    vox, _, _, res = ec.case("5x7x33-unknown_on")
    off, on = ec.host_twin("5x7x33-unknown_off"), ec.host_twin("5x7x33-unknown_on")
    unknown = (vox & 2) != 0
    assert unknown.any() and np.all(on[unknown] < 0) and np.all(off[unknown] > 0)
    vox, _, _, _ = ec.case("9x70x31-inflated_p0")
    p0, p2 = ec.host_twin("9x70x31-inflated_p0"), ec.host_twin("9x70x31-inflated_p2")
    assert np.array_equal(p0 < 0, (vox & 1) != 0) and np.array_equal(p2 < 0, (vox & 4) != 0)


def test_refused_arguments():
    lib = _lib.load()
    vox = np.zeros((4, 4, 4), dtype=np.uint8)
    out = np.full((4, 4, 4), 7.0, dtype=np.float32)
    pv, po = vox.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    INVALID = -1
    assert lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, 1, 0, 0.1, po) == INVALID          # plane 1 is the unknown plane
    assert lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, 3, 0, 0.1, po) == INVALID
    assert lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, -1, 0, 0.1, po) == INVALID
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (4, -3, 4)):
        assert lib.vigo_esdf_from_voxels_host(*dims, pv, 2, 0, 0.1, po) == INVALID, dims
    assert lib.vigo_esdf_from_voxels_host(4, 4, 4, None, 2, 0, 0.1, po) == INVALID
    assert lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, 2, 0, 0.1, None) == INVALID
    for res in (0.0, -0.1, float("nan"), float("inf")):
        assert lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, 2, 0, res, po) == INVALID, res
    assert np.all(out == 7.0)                                                              # nothing was written
    assert lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, 2, 0, 0.1, po) == 0 and lib.vigo_esdf_from_voxels_host(4, 4, 4, pv, 0, 1, 0.1, po) == 0
    # squared distances are int32: a lattice whose nx^2 + ny^2 + nz^2 passes 2^30 is refused before anything is read
    assert lib.vigo_esdf_from_voxels_host(40000, 2, 2, pv, 2, 0, 0.1, po) == -6            # VIGO_ERR_UNSUPPORTED
    # and so is one of more than 2^33 voxels (16384^3 has nx^2 + ny^2 + nz^2 = 3 * 2^28): no attempt to allocate it
    before = out.copy()
    assert lib.vigo_esdf_from_voxels_host(16384, 16384, 16384, pv, 2, 0, 0.1, po) == -6
    assert lib.vigo_esdf_from_voxels_host(2048, 2048, 2049, pv, 2, 0, 0.1, po) == -6       # 2^33 + 2^22 voxels
    assert np.array_equal(out, before)
    assert lib.vigo_abi_version() == 4
