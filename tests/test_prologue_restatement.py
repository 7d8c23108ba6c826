"""bsplineTraj's host prologue of makePlan() in the facade (host/src/bsplineTraj.cpp: findCollisionSeg -> pathSearch ->
shortcutPath(s) -> findGuidePointSemiCircle / assignGuidePointsSemiCircle) against a pure-Python restatement of the
reference's bsplineTraj.cpp (BT.cpp) / bsplineTraj.h (BT.h) — what decides WHICH guide points and directions the
optimizer's distance term gets.  A* inside it is tests/test_astar_restatement.py's restatement.  The restatement keeps the
reference's oddities: the `i == endIdx - 1` corner case of findCollisionSeg (BT.cpp:428-432), the truncated PI_const, the
0.1-step bisection of findGuidePointSemiCircle with its first-iteration `prevAngleDiff = 0`, the merge bookkeeping of
pathSearch that drops the unmerged segments (BT.cpp:496-511).  The map is the in-tree dense grid (its own
isInflatedOccupiedLine).  This restatement and the facade are themselves held to the COMPILED reference sources by
tests/test_oracle_ref_bspline.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_astar_restatement import reference_astar

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")
PI_const = 3.1415926
DEG = 3                                                                                 # bsplineDegree, BT.h:16


def _host():
    lib = C.CDLL(LIB)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    lib.vigo_host_bspline_prologue.argtypes = [C.c_void_p, ip, dp, C.c_double, C.c_int, dp, dp, dp, ip, ip, ip, ip, dp, ip, dp, C.c_int]
    lib.vigo_host_bspline_prologue.restype = C.c_int
    return lib


class DenseMap:
    def __init__(self, vox, origin, res):
        self.vox, self.origin, self.res = vox, origin, res

    def occ(self, p):
        i = [int(math.floor((p[a] - self.origin[a]) / self.res)) for a in range(3)]
        if any(i[a] < 0 or i[a] >= self.vox.shape[a] for a in range(3)):
            return True
        return bool(self.vox[i[0], i[1], i[2]] & 1)

    def occ_line(self, p1, p2):                                                         # standin/dense_occmap.h
        if self.occ(p1) or self.occ(p2):
            return True
        diff = p2 - p1
        dist = math.sqrt(float(diff @ diff))
        inc = diff / dist * self.res
        for i in range(1, int(dist / self.res)):
            if self.occ(p1 + i * inc):
                return True
        return False


def collision_segments(n, occ, occ_line, not_check_ratio=0.0):                          # BT.cpp:403-444
    """findCollisionSeg over two predicates: occ(i) — control point i is inflated-occupied; occ_line(i) — the line from
    control point i - 1 to i is (asked only where both ends are free)"""
    segs, prev = [], False
    end_idx = int((n - DEG - 1) - not_check_ratio * (n - 2 * DEG))
    start = DEG
    for i in range(DEG, end_idx + 1):
        hit = bool(occ(i))
        if hit != prev:
            if hit:
                start = i - 1
            else:
                segs.append((start, i))
        if hit and i == end_idx - 1:
            segs.append((start, n - 1))
        if i != DEG and not prev and not hit and occ_line(i):
            segs.append((i - 1, i))
        prev = hit
    return segs


def find_collision_seg(m, c):
    return collision_segments(c.shape[0], lambda i: m.occ(c[i]), lambda i: m.occ_line(c[i - 1], c[i]))


def check_collision_line(m, p1, p2):                                                    # BT.h:196-204
    a = 0.0
    while a <= 1.0:
        if m.occ(a * p1 + (1 - a) * p2):
            return True
        a += m.res
    return False


def shortcut_path(m, path):                                                             # BT.h:206-247
    sc = [path[0]]
    if len(path) == 1:
        return sc
    if len(path) == 2:
        return sc + [path[1]]
    p1i, p2i = 0, 2
    while True:
        if p2i > len(path) - 1:
            break
        if not check_collision_line(m, path[p1i], path[p2i]):
            if p2i >= len(path) - 1:
                sc.append(path[p2i])
                break
            p2i += 1
        else:
            sc.append(path[p2i - 1])
            p1i = p2i - 1
            p2i = p1i + 2
    return sc


def angle_between(a, b):                                                                # utils.h:84-86
    cr = np.cross(a, b)
    return math.atan2(math.sqrt(float(cr @ cr)), float(a @ b))


def find_guide_point(idx, seg, path):                                                   # BT.h:259-304
    num = seg[1] - seg[0] - 1
    if num != 0:
        target = (idx - seg[0]) * PI_const / (num + 2)
        target = min(max(PI_const * 0.0 / 4.0, target), PI_const * 4.0 / 4.0)
        ratio = float(idx - seg[0]) / float(num + 1.0)
        pseudo = ratio * (path[-1] - path[0]) + path[0]
    else:
        target = PI_const / 2.0
        pseudo = (path[0] + path[-1]) / 2.0
    direction = path[0] - pseudo
    for i in range(len(path) - 1):
        cur, nxt = path[i], path[i + 1]
        if angle_between(direction, cur - pseudo) <= target <= angle_between(direction, nxt - pseudo):
            prev_diff, prev_pt = 0.0, None
            a = 1.0
            while a >= 0.0:
                tp = a * cur + (1 - a) * nxt
                diff = angle_between(direction, tp - pseudo) - target
                if diff == 0:
                    return tp, True
                if diff * prev_diff < 0:
                    tot = abs(diff) + abs(prev_diff)
                    return abs(prev_diff) / tot * (tp - prev_pt) + prev_pt, True
                prev_diff, prev_pt = diff, tp
                a -= 0.1
    return None, False


def reference_prologue(vox, origin, res, c, cfg):
    m = DenseMap(vox, origin, res)
    segs = find_collision_seg(m, c)
    pool = tuple(2 * int(cfg[3 + a] / res) for a in range(3))                            # BT.cpp:191-194
    paths, merged, i = [], [], 0
    nseg = len(segs)
    while i < nseg:                                                                     # BT.cpp:446-513
        seg = segs[i]
        s, e = c[seg[0]], c[seg[1]]
        p = reference_astar(vox, origin, res, pool, cfg[1], cfg[2], res, s, e)
        if p is not None:
            paths.append([s] + [q for q in p[1:]] + [e])
        else:
            ok = False
            if i + 1 < nseg and segs[i + 1][0] - seg[1] <= 2:
                e2 = c[segs[i + 1][1]]
                p = reference_astar(vox, origin, res, pool, cfg[1], cfg[2], res, s, e2)
                if p is not None:
                    paths.append([s] + [q for q in p[1:]] + [e2])
                    merged.append(i)
                    i += 2
                    ok = True
            if not ok:
                return None
            continue
        i += 1
    if merged:                                                                          # BT.cpp:496-511: the unmerged ones are lost
        tmp, midx, i = [], 0, 0
        while i < nseg:
            if midx < len(merged) and i == merged[midx]:
                tmp.append((segs[i][0], segs[i + 1][1]))
                i += 1
                midx += 1
            i += 1
        segs = tmp
    n = c.shape[0]
    guides = [[] for _ in range(n)]
    sc = [shortcut_path(m, p) for p in paths]                                           # BT.cpp:517-571
    gp = None
    for i, seg in enumerate(segs):
        path = sc[i]
        for idx in range(seg[0] + 1, seg[1]):
            g, found = find_guide_point(idx, seg, path)
            if found:
                gp = g
            d = gp - c[idx]
            guides[idx].append((gp.copy(), d / math.sqrt(float(d @ d))))
        if seg[1] - seg[0] - 1 == 0:
            g, found = find_guide_point(seg[0], seg, path)
            if found:
                gp = g
            mid = (c[seg[0]] + c[seg[1]]) / 2.0
            d = gp - mid
            gd = d / math.sqrt(float(d @ d))
            for idx in range(seg[0] - 1, seg[1] + 2):
                if DEG <= idx <= n - DEG - 1:
                    guides[idx].append((gp.copy(), gd))
    return segs, paths, guides


def _world(rng, n=96):
    vox = np.zeros((n, n, 30), dtype=np.uint8)
    for _ in range(int(rng.integers(3, 8))):
        c = rng.integers(20, n - 20, size=2)
        h = rng.integers(2, 6, size=2)
        vox[c[0] - h[0]:c[0] + h[0], c[1] - h[1]:c[1] + h[1], :] |= 1
    return vox, np.array([-4.8, -4.8, 0.0])


@pytest.mark.parametrize("seed", range(5))
def test_facade_prologue_is_the_references_collision_segments_paths_and_guide_points(seed):
    host = _host()
    rng = np.random.default_rng(500 + seed)
    compared = with_guides = 0
    for case in range(6):
        vox, origin = _world(rng)
        res = 0.1
        y0, y1 = rng.uniform(-2.5, 2.5, size=2)
        n_path = 33
        xs = np.linspace(-4.0, 4.0, n_path)
        path = np.stack([xs, np.linspace(y0, y1, n_path), np.full(n_path, 1.0)], axis=1)
        cfg = np.array([0.5, 0.7, 1.3, 4.0, 4.0, 4.0])
        cap = 200000
        ctrl, nctrl = np.zeros(cap), C.c_int()
        seg, nseg = np.zeros(cap, dtype=np.int32), C.c_int()
        goff, gout = np.zeros(cap, dtype=np.int32), np.zeros(cap)
        poff, pout = np.zeros(cap, dtype=np.int32), np.zeros(cap)
        dims = (C.c_int * 3)(*vox.shape)
        vv = np.ascontiguousarray(vox)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        rc = host.vigo_host_bspline_prologue(vv.ctypes.data_as(C.c_void_p), dims, origin.ctypes.data_as(dp), res, n_path,
                                             np.ascontiguousarray(path).ctypes.data_as(dp), cfg.ctypes.data_as(dp), ctrl.ctypes.data_as(dp),
                                             C.byref(nctrl), seg.ctypes.data_as(ip), C.byref(nseg), goff.ctypes.data_as(ip),
                                             gout.ctypes.data_as(dp), poff.ctypes.data_as(ip), pout.ctypes.data_as(dp), cap)
        if rc == -1:
            continue                                              # the goal lies in an obstacle: updatePath refuses
        assert rc == 0
        n = nctrl.value
        c = ctrl[:3 * n].reshape(n, 3)
        ref = reference_prologue(vox, origin, res, c, cfg)
        if ref is None:
            assert nseg.value == -1, (seed, case)
            continue
        segs, paths, guides = ref
        compared += 1
        assert nseg.value == len(segs) and [tuple(x) for x in seg[:2 * nseg.value].reshape(-1, 2)] == segs, (seed, case)
        for i, p in enumerate(paths):
            got = pout[3 * poff[i]:3 * poff[i + 1]].reshape(-1, 3)
            assert got.shape[0] == len(p) and np.array_equal(got, np.array(p)), (seed, case, i)
        for idx in range(n):
            got = gout[6 * goff[idx]:6 * goff[idx + 1]].reshape(-1, 6)
            assert got.shape[0] == len(guides[idx]), (seed, case, idx)
            for j, (gp, gd) in enumerate(guides[idx]):
                assert np.allclose(got[j, :3], gp, rtol=0, atol=1e-12) and np.allclose(got[j, 3:], gd, rtol=0, atol=1e-12), (seed, case, idx, j)
        with_guides += any(len(g) for g in guides)
    assert compared >= 2 and with_guides >= 1
