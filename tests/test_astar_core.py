"""-m "not gpu": the search core the A* kernel runs (csrc/vigo_astar_core.hpp), compiled for the host, against the
facade's host A* (host/src/astarOcc.cpp) and the Python restatement of the reference's algorithm
(tests/test_astar_restatement.py: reference_astar) — path for path, bit for bit, with the same pops, pushes and heap
peak: the same search, not only the same path.  Then the budgets that replace the reference's 0.2 s wall clock, and the
capacity the kernel ships with against the searches of the pipeline workload."""
import ctypes as C

import numpy as np
import pytest

import astar_cases as ac
from test_astar_restatement import reference_astar


@pytest.fixture(scope="module")
def lib():
    return ac.host_lib()


def _three_ways(lib, c):
    ref = reference_astar(c.vox, c.origin, c.res, c.pool, c.min_h, c.max_h, c.step, c.start, c.end)
    host, hs = ac.host_astar(lib, c)
    st, core, cs, _ = ac.core_astar(lib, c, **ac.UNBOUNDED)
    assert (ref is None) == (host is None), c.name
    assert st == (ac.NOT_FOUND if host is None else ac.FOUND), (c.name, st)
    if host is not None:
        assert host.shape == ref.shape and np.array_equal(host, ref), c.name
        assert core.shape == host.shape and np.array_equal(core, host), c.name
    # pops, pushed, heap peak, rewrites
    assert [cs[0], cs[1], cs[2], cs[3]] == [hs[0], hs[4], hs[2], hs[3]], (c.name, cs, hs)
    return host, hs


def test_core_is_the_host_search_on_the_restatement_worlds(lib):
    found = rewrites = 0
    for c in ac.restatement_cases():
        host, hs = _three_ways(lib, c)
        found += host is not None
        rewrites += int(hs[3])
    assert found >= 8
    assert rewrites >= 1            # the stale-heap rule is exercised: a better path rewrote an open node


def test_core_is_the_host_search_on_the_crafted_cases(lib):
    got = {}
    for c in ac.crafted_cases():
        host, hs = _three_ways(lib, c)
        got[c.name] = (host, hs)
    assert got["ties: axis-aligned, empty world"][0] is not None and got["ties: diagonal, empty world"][0] is not None
    assert len(got["ties: start == end"][0]) == 1
    assert got["wall: detour"][0] is not None and got["wall: detour"][1][3] >= 1             # rewrites happened
    for name in ("start inside the wall (pushed out)", "end inside the wall (pushed out)", "both ends inside obstacles"):
        assert got[name][0] is not None, name
    assert got["ends outside the pool"][0] is None and got["ends outside the pool"][1][0] == 0   # adjustEnds false: nothing popped
    assert got["start pushed out of the pool"][0] is None and got["start pushed out of the pool"][1][0] == 0
    assert got["enclosed goal (open set exhausted)"][0] is None and got["enclosed goal (open set exhausted)"][1][0] > 100
    assert got["enclosed goal, larger pool"][0] is None and got["enclosed goal, larger pool"][1][0] > 100


def test_budgets_defer_without_a_result_and_just_enough_is_enough(lib):
    c = next(k for k in ac.crafted_cases() if k.name == "wall: detour")
    host, hs = ac.host_astar(lib, c)
    pops, pushed, peak = int(hs[0]), int(hs[4]), int(hs[2])
    assert pops > 60 and pushed > 60
    # a table of a few dozen nodes; a small max_expansions; a small heap: DEFERRED, and the path buffer is untouched
    for kw in (dict(cap_log2=6, max_nodes=48, heap_cap=1 << 20, max_expansions=1 << 30),
               dict(cap_log2=20, max_nodes=(1 << 20) - 1, heap_cap=1 << 20, max_expansions=pops - 1),
               dict(cap_log2=20, max_nodes=(1 << 20) - 1, heap_cap=peak - 1, max_expansions=1 << 30),
               dict(cap_log2=20, max_nodes=(1 << 20) - 1, heap_cap=1 << 20, max_expansions=0)):
        st, path, _, buf = ac.core_astar(lib, c, **kw)
        assert st == ac.DEFERRED and path is None and np.all(buf == -7.0), kw
    # just large enough in all three: the unbounded result (the table at 1 << 13 slots holds `pushed` nodes exactly)
    log2 = max(1, int(np.ceil(np.log2(pushed + 1))))
    st, path, cs, _ = ac.core_astar(lib, c, cap_log2=log2, max_nodes=pushed, heap_cap=peak, max_expansions=pops)
    assert st == ac.FOUND and np.array_equal(path, host) and [cs[0], cs[1], cs[2]] == [pops, pushed, peak]
    # a found path longer than path_cap: reported with its length, not written
    st, path, _, buf = ac.core_astar(lib, c, path_cap=len(host) - 1, **ac.UNBOUNDED)
    assert st == ac.PATH_TOO_LONG and np.all(buf == -7.0)
    st, path, _, _ = ac.core_astar(lib, c, path_cap=len(host), **ac.UNBOUNDED)
    assert st == ac.FOUND and np.array_equal(path, host)
    # arguments the device entry refuses
    assert ac.core_astar(lib, c, cap_log2=6, max_nodes=64, heap_cap=64, max_expansions=10)[0] == -1     # max_nodes must leave a slot empty


def test_shipped_capacity_holds_the_pipeline_workload(lib):
    """Condition of the GPU parity test (it must not pass by deferring everything): at most 2 % of the prologue searches
    of the pipeline batch need more pushed nodes or a larger heap than vigo_astar_search holds."""
    from trajectory_planner_amd import _lib
    max_nodes, max_heap = C.c_int32(0), C.c_int32(0)
    assert _lib.load().vigo_astar_capacity(C.byref(max_nodes), C.byref(max_heap)) == 0
    _, pool, ends, ln, _, stats = ac.pipeline_searches(lib)
    pops, reached, peak, pushed = stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 4]
    q = lambda v: [int(x) for x in np.quantile(v, [0.5, 0.9, 0.98, 0.99, 1.0])]
    over = (pushed > max_nodes.value) | (peak > max_heap.value)
    print(f"\n{len(ends)} searches, pool {pool}; quantiles 50 / 90 / 98 / 99 / 100 %: pops {q(pops)}, reached {q(reached)}, pushed {q(pushed)}, "
          f"heap peak {q(peak)}; over the shipped capacity ({max_nodes.value} nodes, {max_heap.value} heap entries): {over.mean() * 100:.2f} %")
    assert len(ends) >= 400
    assert over.mean() <= 0.02
