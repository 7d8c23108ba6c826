"""-m gpu: vigo_build_esdf_tracked + vigo_update_grid_region + vigo_update_esdf on the device against the host twins
(vigo_esdf_from_voxels_host_tracked / vigo_esdf_update_host, pinned on the CPU by test_esdf_update_core.py), bit for bit, on
every case of esdf_update_cases.py: the returned lattice, the stats, and the installed field through both queries; NULL
lattice; a user stream without a synchronise; the tracking rules; the tracked build against the plain one.

Shapes: nothing is larger than 64^3 or a 300-long axis.  The update has ONE route per pass (csrc/vigo_esdf_build.hip: a
launch over the footprint, the slab, the lattice, the bricked field, with flag exits), so no shape is there for a second;
2x3x300, 3x300x2 and 300x2x3 put the long axis on each pass, the world on more than one block per launch."""
import numpy as np
import pytest
import torch

import esdf_build_cases as ec
import esdf_update_cases as uc
from gpu_util import to_dev
from test_gpu_esdf_build import ORIGIN, assert_same_field, bits, query_points
from trajectory_planner_amd.vigo import Vigo

pytestmark = pytest.mark.gpu

NO_GRID = -5


@pytest.fixture(scope="module")
def handle():
    """one handle for the module: consecutive cases change dims, so the tracking buffer is grown and reused throughout"""
    v = Vigo(0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def ref():
    """the second handle: it only ever takes vigo_set_esdf of a twin's lattice"""
    v = Vigo(0)
    yield v
    v.close()


def start(v, case, return_lattice=False):
    v.set_grid(to_dev(uc.start_grid(case), v.device), ORIGIN, uc.res_of(case))
    return v.build_esdf(plane=case.plane, unknown_is_site=case.unk, return_lattice=return_lattice, tracked=True)


def apply(v, steps, host=False):
    for s in steps:
        if host:
            v.update_grid_region_host(s.lo, np.ascontiguousarray(s.box), s.r)
        else:
            v.update_grid_region(s.lo, to_dev(s.box, v.device), s.r)


def same_field_as_twin(v, ref, lattice, shape, res):
    ref.set_esdf(to_dev(np.array(lattice), ref.device), ORIGIN, res)
    return assert_same_field(v, ref, shape, res)


@pytest.mark.parametrize("name", uc.NAMES)
def test_lattice_stats_and_field_equal_the_host_twin(handle, ref, name):
    case = uc.by_name(name)
    start(handle, case)
    for k, ((steps, _, _), (vox, _, _, want, want_stats)) in enumerate(zip(uc.refreshes(case), uc.chain(name))):
        apply(handle, steps)
        lat, stats = handle.update_esdf(return_lattice=True, stats=True)
        got = lat.cpu().numpy()
        print(name, k, stats, "twin:", want_stats, "lattice values that differ:", int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert ec.same_bits(got, want), (name, k)
        assert stats == want_stats, (name, k)
    same_field_as_twin(handle, ref, want, vox.shape, uc.res_of(case))


@pytest.mark.parametrize("name", ["world64_fill_28_28_28_n8", "9x70x31_plane0_inflate_sequence", "300x2x3_first_site_then_removed",
                                  "5x7x33_unknown_bit_is_site", "3x300x2_whole"])
def test_null_lattice_goes_through_the_installed_field_only(handle, ref, name):
    """no out_lattice_dev, no stats, in either call: what the queries read afterwards is the twin's field"""
    case = uc.by_name(name)
    assert start(handle, case) is None
    for (steps, _, _), (vox, _, _, want, _) in zip(uc.refreshes(case), uc.chain(name)):
        apply(handle, steps)
        assert handle.update_esdf() is None
        same_field_as_twin(handle, ref, want, vox.shape, uc.res_of(case))


def test_region_update_refresh_and_query_on_a_user_stream_without_a_sync(ref):
    name = "world64_update_refresh_update_refresh"
    case = uc.by_name(name)
    vox, _, _, want, _ = uc.chain(name)[-1]
    res = uc.res_of(case)
    p = query_points(vox.shape, res)
    ref.set_esdf(to_dev(np.array(want), ref.device), ORIGIN, res)
    want_d, want_g = ref.esdf_query(to_dev(p, ref.device))
    torch.cuda.synchronize()
    v = Vigo(0)
    try:
        s = torch.cuda.Stream(device=v.device)
        with torch.cuda.stream(s):
            v.use_current_stream()
            p_d = to_dev(p, v.device)
            boxes = [[to_dev(st.box, v.device) for st in steps] for steps, _, _ in uc.refreshes(case)]
            start(v, case)
            for (steps, _, _), dev_boxes in zip(uc.refreshes(case), boxes):
                for st, box in zip(steps, dev_boxes):
                    v.update_grid_region(st.lo, box, st.r)
                v.update_esdf()                                                           # stats NULL: no host round trip
            d, g = v.esdf_query(p_d)                                                      # same stream, no sync in between
        s.synchronize()
        assert np.array_equal(bits(d), bits(want_d)) and np.array_equal(bits(g), bits(want_g))
    finally:
        v.close()


def test_tracking_rules(ref):
    case = uc.by_name("9x70x31_update_refresh_update_refresh")
    res = uc.res_of(case)
    grid0 = uc.start_grid(case)
    chain, refreshes = uc.chain(case.name), uc.refreshes(case)
    v = Vigo(0)
    try:
        lib, h = v._lib, v._h
        assert lib.vigo_update_esdf(None, None, None) == -1

        def not_tracking():
            assert lib.vigo_update_esdf(h, None, None) == NO_GRID and b"tracking" in lib.vigo_last_error(h)

        def tracks_again():
            """a tracked build works again, and the first refresh of the case after it"""
            lat = start(v, case, return_lattice=True)
            assert ec.same_bits(lat.cpu().numpy(), uc.tracked_start(case.start, case.plane, case.unk)[2])
            apply(v, refreshes[0][0])
            lat, stats = v.update_esdf(return_lattice=True, stats=True)
            assert ec.same_bits(lat.cpu().numpy(), chain[0][3]) and stats == chain[0][4]

        not_tracking()                                                                    # before any tracked build
        v.set_grid(to_dev(grid0, v.device), ORIGIN, res)
        not_tracking()
        tracks_again()
        v.set_grid(to_dev(grid0, v.device), ORIGIN, res)                                  # a whole-snapshot call
        not_tracking()
        tracks_again()
        v.set_grid_host(np.ascontiguousarray(grid0), ORIGIN, res)
        not_tracking()
        tracks_again()
        v.set_grid_packed(v.pack_grid(to_dev(grid0, v.device)), grid0.shape, ORIGIN, res)
        not_tracking()
        tracks_again()
        v.build_esdf(plane=case.plane)                                                    # the untracked build
        not_tracking()
        v.set_grid(to_dev(grid0, v.device), ORIGIN, res)
        tracks_again()
        v.set_esdf(to_dev(np.array(chain[0][3]), v.device), ORIGIN, res)
        not_tracking()
        v.set_grid(to_dev(grid0, v.device), ORIGIN, res)
        tracks_again()
        # parameters, metric bounds and the precision do not end it; an empty pending box is OK with zero stats
        v.set_params(v.params)
        v.set_metric_bounds((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
        v.set_precision(0)
        lat, stats = v.update_esdf(return_lattice=True, stats=True)
        assert stats == dict(box_lo=(0, 0, 0), box_n=(0, 0, 0), y_lines=0, x_lines=0) and ec.same_bits(lat.cpu().numpy(), chain[0][3])
        # the _host region form feeds the pending box too
        apply(v, refreshes[1][0], host=True)
        lat, stats = v.update_esdf(return_lattice=True, stats=True)
        assert ec.same_bits(lat.cpu().numpy(), chain[1][3]) and stats == chain[1][4] and stats["box_n"] != (0, 0, 0)
        # a tracked build with other dims regrows the buffer: small -> the world -> small
        for name in ("world64_fill_30_20_40_n4", "5x7x33_word", "world64_clear_28_28_28_n8"):
            other = uc.by_name(name)
            start(v, other)
            apply(v, other.steps)
            lat, stats = v.update_esdf(return_lattice=True, stats=True)
            vox, _, _, want, want_stats = uc.chain(name)[-1]
            assert ec.same_bits(lat.cpu().numpy(), want) and stats == want_stats, name
            same_field_as_twin(v, ref, want, vox.shape, uc.res_of(other))
    finally:
        v.close()


@pytest.mark.parametrize("name", ["world64_p2", "world64_p0", "9x70x31-rand50", "5x7x33-unknown_on", "300x2x3-rand02"])
def test_tracked_build_equals_the_plain_build(handle, name):
    vox, plane, unk, res = ec.case(name)
    handle.set_grid(to_dev(vox, handle.device), ORIGIN, res)
    plain = handle.build_esdf(plane=plane, unknown_is_site=unk, return_lattice=True)
    tracked = handle.build_esdf(plane=plane, unknown_is_site=unk, return_lattice=True, tracked=True)
    assert torch.equal(plain.view(torch.int32), tracked.view(torch.int32))
    assert ec.same_bits(tracked.cpu().numpy(), ec.host_twin(name))
