// vigo_fit_plan.hpp — the work plan of vigo_bspline_fit_mixed: which paths of a batch are fitted, how they are regrouped
// by point count into wave-groups of one K, how many wave-groups a launch has to provide for, and where the operator of
// each K lies in the handle's table.  ONE copy for host and device: vigo_fit.hip's kernels execute it, vigo_api.cpp sizes
// the table, the workspace and the grid with it, tests/fit_plan_check.cpp holds it against a restatement on a machine
// without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_FIT_HD __host__ __device__ __forceinline__
#else
#define VIGO_FIT_HD inline
#endif

namespace vigo {

constexpr int kFitMixedMinK = 4;     // bspline.cpp:83-87
constexpr int kFitMixedMaxK = 62;    // K + 2 <= 64, the mixed solve entries' largest stride
constexpr int kFitBins = kFitMixedMaxK - kFitMixedMinK + 1;   // 59: bin k holds the paths of K = k + 4
constexpr int kFitSmallBins = 27;    // bins of K + 2 <= 32 (K <= 30): the 9 k-step class; the others take 17 steps
constexpr int kFitGroupPaths = 5;    // paths per wave-group: 15 of the 16 columns of an MFMA tile
constexpr int kFitMixedMinStride = 7, kFitMixedMaxStride = 64;

// bin of a path, -1: not fitted.  K and status are device data: nothing is indexed with them before this has passed.
VIGO_FIT_HD int fit_mixed_bin(int K, int status, int Ns, int point_stride) {
    const int top = Ns - 2 < point_stride ? Ns - 2 : point_stride;
    if (status != 0 || K < kFitMixedMinK || K > kFitMixedMaxK || K > top) return -1;
    return K - kFitMixedMinK;
}

// the table: the transposed operators A+ (pinvT[j][row], (K + 4) x (K + 2) doubles) of K = 4 .. 62 back to back;
// fit_table_offset(63) is its size.  sum_{k < K} (k + 4)(k + 2) in closed form, less the terms of k < 4.
VIGO_FIT_HD size_t fit_table_offset(int K) {
    const size_t n = (size_t)K;
    return (n - 1) * n * (2 * n - 1) / 6 + 3 * n * (n - 1) + 8 * n - 82;
}
VIGO_FIT_HD size_t fit_table_doubles() { return fit_table_offset(kFitMixedMaxK + 1); }
// the factorisations' work matrices [A | I], (K + 4) x (2K + 6) doubles each, laid out the same way
VIGO_FIT_HD size_t fit_table_work_offset(int K) {
    const size_t n = (size_t)K;
    return (n - 1) * n * (2 * n - 1) / 3 + 7 * n * (n - 1) + 24 * n - 208;
}
VIGO_FIT_HD size_t fit_table_work_doubles() { return fit_table_work_offset(kFitMixedMaxK + 1); }

// wave-groups of a bin of cnt paths, and the wave-groups a launch provides for without knowing the counts: every
// non-empty bin ends in at most one partly filled group
VIGO_FIT_HD int fit_bin_groups(int cnt) { return (cnt + kFitGroupPaths - 1) / kFitGroupPaths; }
VIGO_FIT_HD long long fit_mixed_max_groups(long long T) { return (T + kFitGroupPaths - 1) / kFitGroupPaths + kFitBins; }

// exclusive prefixes over the bins, kFitBins + 1 entries each: of the paths (= where a bin starts in the sorted order)
// and of the wave-groups
VIGO_FIT_HD void fit_plan_prefix(const int* cnt, int* path_prefix, int* group_prefix) {
    int p = 0, g = 0;
    for (int k = 0; k < kFitBins; ++k) {
        path_prefix[k] = p;
        group_prefix[k] = g;
        p += cnt[k];
        g += fit_bin_groups(cnt[k]);
    }
    path_prefix[kFitBins] = p;
    group_prefix[kFitBins] = g;
}

// wave-group g: its K, the position of its first member in the sorted order and its members (1 .. 5); K = 0: g is
// beyond the last group
struct FitGroup {
    int K, first, members;
};
VIGO_FIT_HD FitGroup fit_group_of(const int* path_prefix, const int* group_prefix, int g) {
    if (g < 0 || g >= group_prefix[kFitBins]) return {0, 0, 0};
    int lo = 0, hi = kFitBins;   // the last bin with group_prefix[bin] <= g (empty bins before it share its prefix)
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (group_prefix[mid] <= g) lo = mid; else hi = mid;
    }
    const int local = g - group_prefix[lo];
    const int cnt = path_prefix[lo + 1] - path_prefix[lo];
    const int left = cnt - kFitGroupPaths * local;
    return {lo + kFitMixedMinK, path_prefix[lo] + kFitGroupPaths * local, left < kFitGroupPaths ? left : kFitGroupPaths};
}

}  // namespace vigo
