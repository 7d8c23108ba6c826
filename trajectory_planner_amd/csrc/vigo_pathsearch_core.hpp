// vigo_pathsearch_core.hpp — the rules of steps 1 and 2 of bsplineTraj's prologue around the A* searches themselves, as
// the kernels of vigo_pathsearch.hip run them and the host compiles too (host/src/cabi_host.cpp:
// vigo_host_path_search_core; tests/test_pathsearch_core.py pins it against the facade's findCollisionSeg / pathSearch /
// applyMerges and the Python restatement of tests/test_prologue_restatement.py).
//
//   collision_segs   findCollisionSeg (BT.cpp:403-445; host/src/bsplineTraj.cpp:409): the serial scan over the control
//                    points' occupancy, with endIdx = int((N - 4) - notCheckRatio * (N - 6)), the `i == endIdx - 1` corner
//                    case that can push a segment a second time, and the line test asked only where both ends are free.
//   retry_list       which second-choice searches a trajectory's failures ask for (the rule of pathSearchBatch: start of
//                    segment k to the end of segment k + 1 when the first choice fails and the gap is <= 2, the next
//                    segment then skipped, every retry taken to succeed when looking for the next one).
//   path_walk        pathSearch's loop (BT.cpp:447-514) replayed on the searches' results, and applyMerges with its quirk:
//                    once one merge is taken the unmerged segments are dropped, so the trajectory keeps the merged
//                    segments alone, and (the min(collisionSeg.size(), paths.size()) bound of BT.cpp:523) as many paths
//                    from the front of the path list.
//   line_interior_occupied / line_occupied   isInflatedOccupiedLine of the dense map contract (include/vigo.h) over a
//                    point predicate: the walk between the ends, and the ends first.  k_ctrl_occupancy (vigo_map.hip) and
//                    the rebound loop's kernels (vigo_reguide.hip) have the ends' flags already and run the interior walk;
//                    the host twins ask line_occupied.
//   FlagOcc          occ(i) / line(i) of the rules here and in vigo_reguide_core.hpp, read from an array of flags.
//   paths_cut_by_bound   for a caller that wants the unbounded path list: did the bound cut paths off a trajectory.
//
// Integer logic only, apart from endIdx and the line test; every fp64 expression is compiled without contraction.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef VIGO_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_HD __host__ __device__ __forceinline__
#else
#define VIGO_HD inline
#endif
#endif

namespace vigo {

// per-trajectory status (include/vigo.h VIGO_PATHS_*)
enum {
    kPathsOk = 0,
    kPathsFailed = 1,        // "Path Search Error. Force return.": no segments, no paths
    kPathsDeferred = 2,      // a consulted search has no result on the device, or too many segments: the host steps decide
};
constexpr int kPathsMaxSegs = 48;            // VIGO_MAX_COLLISION_SEGS
constexpr int kPathsSecond = 1 << 30;        // in a pick: the path is the second-choice search of that segment

// findCollisionSeg's endIdx; a ratio that no int follows (NaN, beyond +-1e9) ends the scan before it starts, as the
// conversion's INT_MIN does on x86
VIGO_HD int collision_end_idx(int N, double not_check_ratio) {
    const double v = (N - 3 - 1) - not_check_ratio * (N - 2 * 3);
    return (v > -1e9 && v < 1e9) ? (int)v : -2147483647 - 1;
}

// occ(i): control point i is inflated-occupied; line(i): isInflatedOccupiedLine(c[i-1], c[i]).  Returns the number of
// segments; the first min(that, cap) are written to seg[][2].
template <class Occ, class Line>
VIGO_HD int collision_segs(int N, double not_check_ratio, const Occ& occ, const Line& line, int cap, int32_t* seg) {
    int n = 0;
    auto push = [&](int a, int e) {
        if (n < cap) { seg[2 * n] = a; seg[2 * n + 1] = e; }
        ++n;
    };
    bool previousHasCollision = false;
    const int endIdx = collision_end_idx(N, not_check_ratio);
    int pairStartIdx = 3;
    for (int i = 3; i <= endIdx; ++i) {
        const bool hasCollision = occ(i);
        if (hasCollision != previousHasCollision) {
            if (hasCollision) pairStartIdx = i - 1;
            else push(pairStartIdx, i);
        }
        if (hasCollision && i == endIdx - 1) push(pairStartIdx, N - 1);
        if (i != 3 && !previousHasCollision && !hasCollision) {
            if (line(i)) push(i - 1, i);
        }
        previousHasCollision = hasCollision;
    }
    return n;
}

// occ(i) / line(i) from the flags of k_ctrl_occupancy, or of a wave's LDS
struct FlagOcc {
    const uint8_t* f;
    VIGO_HD bool operator()(int i) const { return f[i] != 0; }
};

// isInflatedOccupiedLine(q, p) between two FREE ends, over the point predicate occ(x, y, z): int(dist / res) - 1 interior
// steps of length res from q (standin/dense_occmap.h).  A line no int counts the steps of (not finite, or absurdly long)
// has no interior: both ends are inside a grid, it is never that long.
template <class Occ>
VIGO_HD bool line_interior_occupied(const Occ& occ, double res, const double* q, const double* p) {
    const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    const double dist = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const double i0 = d0 / dist * res, i1 = d1 / dist * res, i2 = d2 / dist * res;
    const double fsteps = dist / res;
    const int steps = fsteps < 2147483647.0 ? (int)fsteps : 0;
    for (int s = 1; s < steps; ++s)
        if (occ(q[0] + s * i0, q[1] + s * i1, q[2] + s * i2)) return true;
    return false;
}

// the whole test: the end points first (vigo_ctrl_occupancy's line flag)
template <class Occ>
VIGO_HD bool line_occupied(const Occ& occ, double res, const double* q, const double* p) {
    return occ(q[0], q[1], q[2]) || occ(p[0], p[1], p[2]) || line_interior_occupied(occ, res, q, p);
}

VIGO_HD bool paths_search_decided(int st) { return st == 0 || st == 1; }      // kAstarFound / kAstarNotFound

// the second-choice searches of a trajectory with n segments: emit(k) for every segment k whose first choice is decided
// NOT found and whose successor starts at most 2 after its end — the search from seg[k].first to seg[k + 1].second.  A
// first choice without a result ends the list (the walk defers there).  Returns their number.
template <class St1, class Emit>
VIGO_HD int retry_list(int n, const int32_t* seg, const St1& st1, const Emit& emit) {
    int m = 0;
    for (int k = 0; k < n; ++k) {
        const int s = st1(k);
        if (s == 0) continue;
        if (s != 1) break;
        if (k + 1 >= n || seg[2 * (k + 1)] - seg[2 * k + 1] > 2) break;
        emit(k);
        ++m;
        ++k;
    }
    return m;
}

// pathSearch's loop on the results: st1(k) the status of segment k's first-choice search, st2(k) that of its second
// choice (asked only for a segment retry_list lists).  kPathsOk: *n_out segments in out_seg[][2] (the trajectory's
// collisionSeg_ after applyMerges, bounded by the path count) and path j of them the j-th path pathSearch pushed: the
// search of segment k = pick[j] & ~kPathsSecond of the list `seg`, from ctrl[seg[k].first] to ctrl[seg[k].second] — or,
// when pick[j] & kPathsSecond, its second choice, to ctrl[seg[k + 1].second].  (After a merge out_seg[j] and path j need
// not belong together: the reference pairs them by position.)  Otherwise *n_out = 0.  out_seg and pick hold n entries.
template <class St1, class St2>
VIGO_HD int path_walk(int n, const int32_t* seg, const St1& st1, const St2& st2, int32_t* out_seg, int32_t* pick, int* n_out) {
    *n_out = 0;
    int n_paths = 0, n_merged = 0;
    for (int i = 0; i < n; ++i) {
        const int s = st1(i);
        if (!paths_search_decided(s)) return kPathsDeferred;
        if (s == 0) {
            pick[n_paths++] = i;
            continue;
        }
        if (i + 1 < n && seg[2 * (i + 1)] - seg[2 * i + 1] <= 2) {
            const int s2 = st2(i);
            if (!paths_search_decided(s2)) return kPathsDeferred;
            if (s2 == 0) {
                pick[n_paths++] = i | kPathsSecond;
                ++n_merged;
                ++i;
                continue;
            }
        }
        return kPathsFailed;
    }
    if (n_merged == 0) {
        for (int j = 0; j < n; ++j) { out_seg[2 * j] = seg[2 * j]; out_seg[2 * j + 1] = seg[2 * j + 1]; }
        *n_out = n;                              // (one path per segment)
        return kPathsOk;
    }
    // applyMerges: the merged segments alone, in order; segment j goes with path j of the list (n_merged <= n_paths)
    int m = 0;
    for (int j = 0; j < n_paths; ++j) {
        if (!(pick[j] & kPathsSecond)) continue;
        const int k = pick[j] & ~kPathsSecond;
        out_seg[2 * m] = seg[2 * k];
        out_seg[2 * m + 1] = seg[2 * (k + 1) + 1];
        ++m;
    }
    *n_out = m;
    return kPathsOk;
}

// Did the min(collisionSeg.size(), paths.size()) bound cut paths off a kPathsOk trajectory?  From what the entry returns:
// searches_run (out_counts[b][0]) and n_out (its segments).  With n scanned segments and m merges taken, a kPathsOk walk
// consulted every second choice retry_list listed and found it (a listed retry that fails is kPathsFailed, and retry_list
// stops listing where the walk stops), so searches_run = n + m; the walk pushed n - m paths (a merge spends two segments
// on one path).  m == 0: n_out = n = searches_run, nothing cut.  m > 0: n_out = m, and n - m > m paths exist exactly
// when n != 2m, that is when searches_run != 3 * n_out.  This holds as long as retry_list lists the walk's own retries
// and no others for a trajectory that ends kPathsOk: change the two together.  (The crafted merges of
// tests/test_pathsearch_core.py are one case of each: 3 searches / 1 segment, nothing cut; 4 / 1, path 1 of 2 cut.)
VIGO_HD bool paths_cut_by_bound(int searches_run, int n_out) { return searches_run != n_out && searches_run != 3 * n_out; }

}  // namespace vigo
