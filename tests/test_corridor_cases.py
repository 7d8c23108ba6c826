"""The case set of tests/corridor_cases.py on the CPU (no GPU):

  census       which route of k_corridor (csrc/vigo_corridor_core.hpp) every named segment and every run of every named
               trajectory takes, predicted by the numpy restatement of the kernel's routing predicates
               (tests/corridor_restatement.py: segment_route, per_sample_mask, filter_rejects), with a stated minimum
               per route — so that tests/test_gpu_corridor_cases.py, which compares the device with the oracle on exactly
               these cases, is known to walk every branch;
  obligations  the interval and counts obligations of the span certificates in TRAJECTORY mode: local clocks fl(t - k[i]) of the
               literal loop t += delT, Tu = (ke - kb)(1 + 2^-20), the drift term as the kernel writes it — on the
               large-knot cases, where that drift dominates 2 E by orders of magnitude."""
import collections

import numpy as np
import pytest

import corridor_cases as cc
import oracle_lib as ol
from corridor_restatement import (K_QUEUE_CAP, TILE_WORDS_CAP, U40, accumulated_clock, axis_constants, fast_form, filter_rejects,
                                  per_sample_mask, segment_route)

PER_SAMPLE = ("lane", "lane+L2", "pass1:clock", "pass1:box", "pass1:nonfinite", "pass1:speed")


def oracle_grid(world, bounds):
    g, keep = ol.make_grid(world)
    if bounds is not None:
        g.bmin[:] = list(bounds[0])
        g.bmax[:] = list(bounds[1])
    return g, keep


_census = {}


def segment_census():
    """per case: [(route dict, filter rejections on the per-sample path or None)], computed once"""
    if not _census:
        for c in cc.segment_cases():
            rows = []
            for s in range(len(c.n_samp)):
                n, dT = int(c.n_samp[s]), float(c.delT[s])
                r = segment_route(c.coeffs[s], n, dT, c.box, c.map_res, c.world.grid)
                rej = None
                if c.tags[s].startswith("cancelling"):
                    t = accumulated_clock(dT, n)
                    rejects, f = filter_rejects(c.coeffs[s], r["K"], t)
                    on_path = np.ones(n, bool) if r["route"] in PER_SAMPLE else per_sample_mask(
                        c.coeffs[s], n, dT, r["S1"], r["K"], c.box, c.map_res, c.world.grid, c.world.metric)
                    rej = int((rejects & on_path).sum())
                    r["certified_floats"] = (t, rejects, f)
                rows.append((r, rej))
            _census[c.name] = (c, rows)
    return _census


def test_the_generator_is_deterministic_and_small():
    a, b = cc.segment_cases(), cc.segment_cases()
    assert [c.name for c in a] == [c.name for c in b] and len({c.name for c in a}) == len(a)
    for x, y in zip(a, b):
        assert np.array_equal(x.coeffs, y.coeffs, equal_nan=True) and np.array_equal(x.n_samp, y.n_samp)
        assert np.array_equal(x.delT, y.delT, equal_nan=True) and x.tags == y.tags and len(x.tags) == len(x.n_samp)
        assert len(x.n_samp) <= 40 and x.n_samp.max() <= 2 * cc.SPAN_BATCH + 63
        assert x.world.voxels.shape[0] in (48, 96) and 0 <= x.deg <= 15
        q = x.world.origin / x.world.res
        assert np.abs(q - np.round(q)).max() < 1e-9                  # the origin is on the key lattice
    ta, tb = cc.traj_cases(), cc.traj_cases()
    for x, y in zip(ta, tb):
        assert x.name == y.name and len(x.trajs) == len(y.trajs)
        for (k0, c0, d0, e0), (k1, c1, d1, e1) in zip(x.trajs, y.trajs):
            assert np.array_equal(k0, k1) and np.array_equal(c0, c1, equal_nan=True) and d0 == d1 and np.array_equal(e0, e1, equal_nan=True)
            assert 1 <= len(c0) <= 6
    # what the issue lists: both resolutions, nz a multiple of 32 and not, bounds and none, the degrees, the map_res values
    ws = cc.worlds().values()
    assert {w.res for w in ws} == {0.1, 0.05} and {w.voxels.shape[2] % 32 == 0 for w in ws} == {True, False}
    assert {w.bounds is None for w in ws} == {True, False}
    assert {c.deg for c in a} >= {0, 3, 5, 7, 9, 15} and {c.map_res for c in a} >= {0.05, 0.1, 0.2, 0.25, 0.45}
    counts = set(int(n) for c in a for n in c.n_samp)
    assert counts >= {0, 1, 15, 16, 17, 511, 512, 513, 1025, cc.SPAN_BATCH - 1, cc.SPAN_BATCH, cc.SPAN_BATCH + 1}


def test_routing_census_of_the_segment_cases():
    """Every route of k_corridor in segment mode is reached by named cases, with these minima (conditions on the case
    set, not measurements).  Routes, and the cases that reach them:

      span64 / span32 / span16   PASS 0, certified spans of that length: 'routing: A / D' (segments scaled to just either
                                 side of lipmax * 32 / 16 / 8 = a quarter voxel), 'huggers: *', 'boxes: *'       >= 8 each
      lane                       PASS 0, n <= 512, a lane per sample: 'counts', 'huggers: *', 'degrees: *'       >= 8
      pass1:clock                no clock table (delT 0, negative, below 2^-1000, NaN, infinite, 1e300):
                                 'routing: A / D', 'filter' (the two 'clock negative' segments)                  >= 8
      pass1:box                  more than 3 map cells on one axis: 'boxes: more than 3 cells on x only',
                                 'boxes: 4 cells on y exactly'                                                   >= 8
      pass1:nonfinite            NaN / infinite / huge coefficients: 'routing: A / D'                            >= 8
      pass1:speed                n > 512 and samples further apart than 1/32 of a voxel: 'fast', 'S1 none'       >= 8
      span* + L2                 the tile exceeds tile_words_cap while S1 > 0: 'tile' (long diagonals at 0.05)   >= 4
      nlo != nhi on two axes     the cfg box and the mixed multiples                                             >= 2
      queue, modest              8 .. 256 filter rejections on PASS 0's per-sample path: 'cancelling: modest'    >= 1
      queue, overflow            >= 2048 rejections (4 x kQueueCap): PASS 0 hands the segment to PASS 1, whose
                                 `all` mode repeats the filter: 'cancelling: many, y' (span route, 20000
                                 rejections); 'cancelling: many' goes to PASS 1 by its speed and overflows there >= 1
      queue in PASS 1            'cancelling: clock negative, modest' (a queue below the cap) and '... many'
                                 (`all` mode); 'cancelling: n <= 512' fills a lane-per-sample queue that cannot
                                 overflow (500 of 500 samples rejected).

    Finite inputs within the entry's limits DO reach 2048 rejections: a shifted Chebyshev polynomial of degree 15 with
    0.03 mm amplitude has A = sum |c_d| T^d = 4.6e6 m, E = 2^-46 A = 6.5e-8 m — half the spacing of the floats at 1 m —
    so the filter rejects every one of its 20000 samples.  The counts below are far from kQueueCap on either side, as the
    device's fast form may differ from numpy's in the last place."""
    routes = collections.Counter()
    two_axes = 0
    rej = {}
    for name, (c, rows) in segment_census().items():
        for s, (r, nrej) in enumerate(rows):
            routes[r["route"]] += 1
            two_axes += r["nlo_ne_nhi"] >= 2 and r["route"].startswith(("span", "lane"))
            if nrej is not None:
                rej[c.tags[s]] = (r["route"], nrej)
    print(dict(routes), two_axes, rej)
    span = lambda S1: routes[f"span{S1}"] + routes[f"span{S1}+L2"]
    assert span(64) >= 8 and span(32) >= 8 and span(16) >= 8, routes
    assert routes["lane"] + routes["lane+L2"] >= 8, routes
    for why in ("clock", "box", "nonfinite", "speed"):
        assert routes[f"pass1:{why}"] >= 8, (why, routes)
    assert sum(v for k, v in routes.items() if k.startswith("span") and k.endswith("+L2")) >= 4, routes
    assert two_axes >= 2
    assert rej["cancelling: modest"][0].startswith("span") and 8 <= rej["cancelling: modest"][1] <= 256, rej
    assert rej["cancelling: many, y"][0].startswith("span") and rej["cancelling: many, y"][1] >= 2048, rej
    assert rej["cancelling: many"] == ("pass1:speed", 20000), rej
    assert rej["cancelling: n <= 512"][0] == "lane" and 8 <= rej["cancelling: n <= 512"][1] <= K_QUEUE_CAP, rej
    assert rej["cancelling: clock negative, modest"][0] == "pass1:clock" and 8 <= rej["cancelling: clock negative, modest"][1] <= 256, rej
    assert rej["cancelling: clock negative, many"][0] == "pass1:clock" and rej["cancelling: clock negative, many"][1] >= 4 * K_QUEUE_CAP, rej
    assert TILE_WORDS_CAP == 4608


def test_edge_segments_sit_either_side_of_their_threshold():
    """the 'edge' segments of 'routing: *' are scaled from the restatement: lipmax * factor within 0.2 % of a quarter voxel,
    on the side their tag names"""
    seen = collections.Counter()
    for name, (c, rows) in segment_census().items():
        for s, (r, _) in enumerate(rows):
            if not c.tags[s].startswith("edge"):
                continue
            want = c.tags[s].split("(")[0].strip()[len("edge S1 "):]
            got = "none" if r["route"] == "pass1:speed" else str(r["S1"])
            assert got == want, (name, s, c.tags[s], r["route"])
            factor = float(c.tags[s].split("(x")[1].split(",")[0])
            assert abs(r["lipmax"] * factor / r["cell"] - 1.0) < 2e-3
            seen[want] += 1
    assert all(seen[k] >= 6 for k in ("64", "32", "16", "none")), seen


def test_certified_floats_are_the_exact_chain(olib):
    """filter soundness on the cancelling cases: where the filter certifies, its float IS the float of the oracle's
    exact-power chain — with E = 2^-46 A at the size of the float spacing, this is where a filter that is too narrow shows"""
    O = ol.oracle()
    checked = 0
    with ol.pow_mode(True):
        for name, (c, rows) in segment_census().items():
            for s, (r, nrej) in enumerate(rows):
                if nrej is None:
                    continue
                t, rejects, f = r["certified_floats"]
                co = np.ascontiguousarray(c.coeffs[s])
                p = np.zeros(3)
                for k in np.nonzero(~rejects)[0][:: max(1, len(t) // 400)]:
                    O.vgo_poly_pos(c.deg, ol._d(co[0]), ol._d(co[1]), ol._d(co[2]), float(t[k]), ol._d(p))
                    assert np.array_equal(p.astype(np.float32), f[k]), (name, s, int(k))
                    checked += 1
    assert checked > 50


# ---- trajectory mode -------------------------------------------------------------------------------------------------
def trajectory_runs(knots, delT):
    """the literal loop of checkCollisionTraj (PO.cpp:638-653): global clock t += delT while t < k[K]; segment 0 owns
    t in [k0, k1], segment i >= 1 owns (k_i, k_{i+1}] -> (clock values, [(first index, count)] per segment)"""
    k = np.asarray(knots, np.float64)
    n = int(np.ceil(k[-1] / delT)) + 2
    t = accumulated_clock(delT, n)
    t = t[t < k[-1]]
    runs = []
    for i in range(len(k) - 1):
        m = (t >= k[i]) & (t <= k[i + 1]) if i == 0 else (t > k[i]) & (t <= k[i + 1])
        idx = np.nonzero(m)[0]
        assert len(idx) == 0 or idx[-1] - idx[0] + 1 == len(idx)
        runs.append((int(idx[0]) if len(idx) else 0, len(idx)))
    return t, runs


def test_routing_census_of_the_trajectory_cases():
    """The runs of the chained cases in TRAJ mode (k_corridor<PASS, DEG7, true>), with these minima:

      span*              runs of more than 512 samples: 'plain *' (delT 2^-10), 'long huggers *', 'large knots *'   >= 8
      lane               shorter runs: 'plain *'                                                                  >= 8
      pass1:box          'box more than 3 cells on x only A' (every run)                                          >= 8
      pass1:nonfinite    'non-finite coefficients A' (NaN, +-infinity, 1e300, 1e39, -4e38, 1e20, FLT_MAX)          >= 8
      pass1:speed        'plain *' runs of more than 512 fast samples, 'cancelling: many'                         >= 2
      span* + L2         'tile B' (long diagonals at 0.05), 'long huggers D'                                      >= 2
      queue              'cancelling runs A', the sample clock being fl(t - k[i]): 'modest' 8 .. 256 rejections on
                         PASS 0's per-sample path; 'many, y' >= 2048 there (overflow, hand-over, PASS 1's `all` mode
                         with accumulated_time(dT, first + k) - kb); 'many' the same in PASS 1 from the start;
                         'n <= 512' a lane-per-sample queue that cannot overflow.

    Also: samples exactly on knots, delT that does not divide the durations, and on the large-knot cases a drift term of
    at least 100 times 2 E."""
    routes = collections.Counter()
    on_knots = ragged = 0
    dominated = 0
    rej = {}
    for tc in cc.traj_cases():
        for ti, (knots, coeffs, delT, endpoint) in enumerate(tc.trajs):
            t, runs = trajectory_runs(knots, delT)
            on_knots += int(np.isin(knots[1:-1], t).sum())
            ragged += (knots[-1] - knots[0]) / delT != np.round((knots[-1] - knots[0]) / delT)
            for i, (first, n) in enumerate(runs):
                r = segment_route(coeffs[i], n, delT, tc.box, tc.map_res, tc.world.grid, traj=(knots[i], knots[i + 1]),
                                  table=len(t) > 0)
                routes[r["route"]] += 1
                if tc.name.startswith("large knots") and n > 0:
                    K = r["K"][0]
                    L = K["lipd"] / (abs(delT) * U40)
                    dominated += (K["base"] / U40 - 2.0 * K["E"]) >= 100.0 * 2.0 * K["E"] and L > 0
                if tc.tags and tc.tags[ti].startswith("cancelling") and i == 1:
                    tau = t[first:first + n] - knots[i]
                    rejects, f = filter_rejects(coeffs[i], r["K"], tau)
                    on_path = np.ones(n, bool) if r["route"] in PER_SAMPLE else per_sample_mask(
                        coeffs[i], n, delT, r["S1"], r["K"], tc.box, tc.map_res, tc.world.grid, tc.world.metric, tau=tau)
                    rej[tc.tags[ti]] = (r["route"], int((rejects & on_path).sum()))
    print(dict(routes), on_knots, ragged, dominated, rej)
    assert sum(v for k, v in routes.items() if k.startswith("span")) >= 8 and routes["lane"] >= 8, routes
    assert routes["pass1:box"] >= 8 and routes["pass1:nonfinite"] >= 8 and routes["pass1:speed"] >= 2, routes
    assert sum(v for k, v in routes.items() if k.startswith("span") and k.endswith("+L2")) >= 2, routes
    assert on_knots >= 6 and ragged >= 6 and dominated >= 8
    assert rej["cancelling: modest"][0].startswith("span") and 8 <= rej["cancelling: modest"][1] <= 256, rej
    assert rej["cancelling: many, y"][0].startswith("span") and rej["cancelling: many, y"][1] >= 4 * K_QUEUE_CAP, rej
    assert rej["cancelling: many"][0] == "pass1:speed" and rej["cancelling: many"][1] >= 4 * K_QUEUE_CAP, rej
    assert rej["cancelling: n <= 512"][0] == "lane" and 8 <= rej["cancelling: n <= 512"][1] <= K_QUEUE_CAP, rej


def _obligation_cases():
    tcs = {tc.name: tc for tc in cc.traj_cases()}
    return [n for n in tcs if n.startswith("large knots")] + [n for n in tcs if n.startswith("plain A")]


@pytest.mark.parametrize("name", _obligation_cases())
def test_trajectory_mode_interval_obligation(olib, name):
    """The interval and counts obligations of tests/test_corridor_certificates.py redone for TRAJ (keys is a function of the
    floats alone and carries over).  Obligation 1 of DESIGN §3.4 on the subtracted clock: every oracle float (vgo_poly_pos with the exact power, cast to
    float) of every sample of a span lies in [(float)(p - R), (float)(p + R)], p the fast form at the span's centre sample
    tau_c = fl(t_c - kb), R = (base + lipd * hs)(1 + 2^-40), base = 2 E + L * drift with
    drift = (2 Tm + n (|ke| (1 + 2^-20) + |delT|)) 2^-52 as k_corridor writes it.  Spans of 64, 16 and 4 samples at the
    start of each run, at its end, and at seeded places in between."""
    tc = next(t for t in cc.traj_cases() if t.name == name)
    O = ol.oracle()
    rng = np.random.default_rng(5)
    spans = 0
    p3 = np.zeros(3)
    with ol.pow_mode(True):
        for knots, coeffs, delT, endpoint in tc.trajs:
            t, runs = trajectory_runs(knots, delT)
            for i, (first, n) in enumerate(runs):
                if n < 4:
                    continue
                kb, ke = float(knots[i]), float(knots[i + 1])
                tau = t[first:first + n] - kb                       # fl(t - k[i])
                co = np.ascontiguousarray(coeffs[i])
                K = [axis_constants([float(x) for x in co[a]], n, delT, tc.box[a], tc.map_res, (kb, ke)) for a in range(3)]
                assert tau.min() >= 0.0 and tau.max() <= K[0]["Tu"]
                counted = np.zeros(3, bool)
                for length in (64, 16, 4):
                    if n < length:
                        continue
                    starts = {0, n - length} | {int(x) for x in rng.integers(0, n - length + 1, size=3)}
                    for k0 in sorted(starts):
                        cidx = k0 + length // 2
                        hs = max(cidx - k0, k0 + length - 1 - cidx)
                        f = np.zeros((length, 3), np.float32)
                        for j in range(length):
                            O.vgo_poly_pos(tc.deg, ol._d(co[0]), ol._d(co[1]), ol._d(co[2]), float(tau[k0 + j]), ol._d(p3))
                            f[j] = p3.astype(np.float32)
                        for a in range(3):
                            # counts: nlo, nhi and thr come from A = sum |c_d| Tm^d with Tm from the knots; every sample's
                            # lattice count lies in [nlo, nhi] and equals nhi exactly where the difference reaches thr
                            h = tc.box[a] / 2
                            diff = (f[:, a].astype(np.float64) + h) - (f[:, a].astype(np.float64) - h)
                            num = (diff / tc.map_res).astype(np.int64)
                            assert K[a]["thr_ok"] and K[a]["nhi"] - K[a]["nlo"] <= 1
                            assert num.min() >= K[a]["nlo"] and num.max() <= K[a]["nhi"], (name, i, a, K[a]["nlo"], K[a]["nhi"], int(num.min()), int(num.max()))
                            assert np.array_equal(num == K[a]["nhi"], diff >= K[a]["thr"])
                            counted[a] = True
                            p = fast_form([float(x) for x in co[a]], float(tau[cidx]))
                            R = (K[a]["base"] + K[a]["lipd"] * hs) * U40
                            flo, fhi = np.float32(p - R), np.float32(p + R)
                            assert flo <= f[:, a].min() and f[:, a].max() <= fhi, (name, i, a, length, k0, float(flo), float(f[:, a].min()),
                                                                                   float(f[:, a].max()), float(fhi))
                            # ... and the real-number inequality behind it, with the margin the drift term leaves: the
                            # clock distance of any sample of the span from the centre against |j - c| delT + drift
                            dt_bound = hs * abs(delT) + (2.0 * abs(K[a]["Tu"]) + n * (abs(ke) * (1.0 + 2.0 ** -20) + abs(delT))) * 2.0 ** -52
                            assert np.abs(tau[k0:k0 + length] - tau[cidx]).max() <= dt_bound
                        spans += 1
    assert spans >= 30
