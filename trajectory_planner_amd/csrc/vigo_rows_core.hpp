// vigo_rows_core.hpp — the index arithmetic of "mixed control-point counts" in the prologue and re-guide entries
// (vigo_collision_segs_mixed, vigo_path_search_mixed, vigo_guide_assign_mixed, vigo_rebound_reguide_mixed): a batch of
// rows of Ns control points of which trajectory b owns the first n_pts[b], and guide CSRs over all B * Ns + 1 entries in
// which the control points beyond a count own empty ranges.  Written once for the kernels (vigo_pathsearch.hip,
// vigo_guides.hip, vigo_reguide.hip) and for the host (tests/prologue_mixed_check.cpp walks them between guard bytes).
// The uniform entries pass n_pts == NULL and Ns == N: every function is then what those kernels did before.
#pragma once

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

// the control points of trajectory b: Ns without counts; a count outside [7, Ns] is device data and reads as -1 (the
// trajectory is deferred: nothing of it is indexed by its count)
VIGO_HD int row_count(const int32_t* n_pts, int b, int Ns) {
    if (!n_pts) return Ns;
    const int n = n_pts[b];
    return (n >= 7 && n <= Ns) ? n : -1;
}

// the offsets of one row: off_row[i] = at for EVERY i < Ns, `at` advanced by pairs(i) for i < n only — the control
// points n .. Ns - 1 own the empty range at the row's end.  Returns the next row's first offset.
template <class Pairs>
VIGO_HD long long row_offsets(int Ns, int n, long long at, int32_t* off_row, const Pairs& pairs) {
    for (int i = 0; i < Ns; ++i) {
        off_row[i] = (int32_t)at;
        if (i < n) at += pairs(i);
    }
    return at;
}

// the control point of slot q of a row, off_row[0] <= q < off_row[Ns]: the last i in [0, Ns) with off_row[i] <= q.  The
// search is bounded by the row, not by a count (the empty ranges of the padding all start at the row's end, above q);
// off_row[Ns] itself is never read
VIGO_HD int row_slot_owner(const int32_t* off_row, int Ns, int q) {
    int lo = 0, hi = Ns - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off_row[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace vigo
