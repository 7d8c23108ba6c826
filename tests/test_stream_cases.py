"""CPU: the table of tests/stream_cases.py held against include/vigo.h — every `int vigo_*(vigo_handle_t h, ...)` prototype is
a row of the stream-order test or an entry of EXEMPT with its reason, so that a new entry point cannot land without a row —
and condition (d) of tests/test_gpu_stream_order.py shown before anything runs on a GPU: for every row with a host twin or an
oracle function, the decoy inputs give another answer than the real ones."""
import os
import re

import numpy as np
import pytest

import stream_cases as sc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vigo.h")
TWINS = ("inflate_grid", "set_grid", "set_grid_host", "update_grid_region", "update_grid_region_host", "query_points", "guides_unknown", "cost_grad",
         "optimize", "bspline_fit", "bspline_fit_mixed", "traj_collision", "traj_dynamic_collision", "ctrl_occupancy", "traj_finish", "corridor_check", "poly_sample", "seed_paths", "astar_search",
         "collision_segs", "path_search", "set_esdf", "esdf_query", "esdf_query_f32", "build_esdf", "build_esdf_tracked", "update_esdf", "update_esdf_stats")


def handle_entries():
    with open(HEADER) as f:
        return re.findall(r"^(?:int|const char\*) (vigo_\w+)\(vigo_handle_t h\b", f.read(), flags=re.M)     # (vigo_last_error returns its text)


def test_every_handle_entry_point_is_a_row_or_exempt_with_a_reason():
    entries = handle_entries()
    assert len(entries) >= 50 and len(set(entries)) == len(entries)            # (the pattern still finds the header's prototypes)
    rows = {r.entry for r in sc.rows()}
    missing = [e for e in entries if e not in rows and e not in sc.EXEMPT]
    assert not missing, f"handle entry points without a row of tests/stream_cases.py and without a reason in EXEMPT: {missing}"
    assert not [e for e in sc.EXEMPT if e in rows], "an entry is both a row and exempt"
    assert all(e in entries for e in sc.EXEMPT), "EXEMPT names an entry the header does not have"
    assert all(isinstance(why, str) and len(why.split()) >= 3 for why in sc.EXEMPT.values())
    assert all(r.entry in entries for r in sc.rows()), [r.entry for r in sc.rows() if r.entry not in entries]


def test_the_ids_and_the_no_round_trip_column_name_rows_that_exist():
    names = [r.name for r in sc.rows()]
    assert tuple(names) == sc.ROW_NAMES
    assert set(sc.NO_ROUND_TRIP) <= set(names) and len(set(sc.NO_ROUND_TRIP)) == len(sc.NO_ROUND_TRIP)
    assert {r.name for r in sc.rows() if r.no_round_trip} == set(sc.NO_ROUND_TRIP)
    assert set(TWINS) == {r.name for r in sc.rows() if r.twin is not None}


def test_decoys_are_valid_inputs_of_the_same_shapes():
    for r in sc.rows():
        for k, a in r.real.items():
            d = r.decoy[k]
            assert a.shape == d.shape and a.dtype == d.dtype and a.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"], (r.name, k)
            if a.dtype.kind == "f":
                assert np.isfinite(a).all() and np.isfinite(d).all(), (r.name, k)              # no NaN poison
            if k.endswith("_off"):                                                              # CSR offsets: from 0, monotone
                for off in (a, d):
                    assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all(), (r.name, k)
        assert any(not np.array_equal(r.real[k], r.decoy[k]) for k in r.real), r.name
        for side in (r.real, r.decoy):
            if "guide_off" in side and "guide_pv" in side:
                assert int(side["guide_off"][-1]) <= len(side["guide_pv"]), r.name
            if "obs_off" in side and "obs" in side:
                assert int(side["obs_off"][-1]) == len(side["obs"]), r.name
            if "seg_off" in side and "coeffs" in side:
                assert int(side["seg_off"][-1]) == len(side["coeffs"]), r.name
            if "n_pts" in side:
                assert ((side["n_pts"] >= 7) & (side["n_pts"] <= side["ctrl"].shape[1])).all(), r.name
            if "n_fit" in side:
                assert ((side["n_fit"] >= 4) & (side["n_fit"] <= side["points"].shape[1])).all(), r.name
    mixed = [r for r in sc.rows() if "n_pts" in r.real]
    assert len(mixed) >= 7
    for r in mixed:                                                    # three counts in one row stride, permuted in the decoy
        assert len(set(r.real["n_pts"].tolist())) == 3 and sorted(r.real["n_pts"]) == sorted(r.decoy["n_pts"]), r.name
        assert r.real["n_pts"].tolist() != r.decoy["n_pts"].tolist(), r.name


@pytest.mark.parametrize("name", TWINS)
def test_the_decoy_gives_another_answer_by_the_host_twin(name):
    r = sc.by_name(name)
    real, decoy = r.twin(dict(r.real)), r.twin(dict(r.decoy))
    assert real is not None and len(real) == len(decoy) > 0
    differs = [k for k, (a, b) in enumerate(zip(real, decoy)) if np.asarray(a).shape != np.asarray(b).shape or np.asarray(a).tobytes() != np.asarray(b).tobytes()]
    assert differs, f"{name}: the decoy's result equals the real one in every output: the row cannot tell a call that read too early"
