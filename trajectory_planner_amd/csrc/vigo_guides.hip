// vigo_guides.hip — vigo_guide_assign: the guide assignment of bsplineTraj's prologue (host/src/bsplineTraj.cpp:494-595)
// for B trajectories on the handle's grid snapshot, each the step of vigo_guide_core.hpp with vigo_atan2, bit for bit.
//
// Two kernels.  k_guide_offsets (one workgroup, one scan, as k_rebound_compact): the pair counts follow from the
// segments alone, so it checks the lists, marks the trajectories with a path longer than the LDS buffer DEFERRED (they
// own no pairs), sums the pairs and — only when the lists are good and the pairs fit pair_cap — writes statuses and
// offsets.  The host reads its two result words before anything else is launched.
// k_guide_assign: one wavefront (one workgroup of 64) per trajectory, the segment's path and its shortcut in LDS.
//   shortcutPath          the samples of the line checks spread over the lanes, 64 / samples candidate ptr2 values per
//                         round; the first colliding candidate by ballot
//   bracket test          one path segment per lane, the first match by ballot
//   bisection             one step per lane (11 of them), the previous step's values by a lane shift, the first event
//                         by ballot
// Control points are taken in order (the guide point of a failed search is the previous one).  Lane 0 writes a pair in
// place: its slot is the control point's offset plus the pushes of the earlier segments.  Plain vector stores, no atomics.
// The work is latency-bound (a chain of dependent fp64 divisions, square roots and atan2 per control point).
#include "vigo_guide_core.hpp"
#include "vigo_rows_core.hpp"
#include "vigo_grid.hpp"
#include "vigo_scan.hpp"

namespace vigo {
namespace {

struct GuideArgs {
    int B, N;
    const int32_t* n_pts;  // (vigo_guide_assign_mixed) not NULL: N is the row stride, trajectory b has n_pts[b] control points
    const double* ctrl;
    const int32_t* seg_off;
    const int32_t* seg;
    const int32_t* path_off;
    const double* path;
    long long pair_cap;
    int32_t* off;
    double* pv;
    uint8_t* unk;
    int32_t* status;
    long long* result;     // [0] the pairs of the call, [1] != 0: a bad list
};

__global__ void __launch_bounds__(1024) k_guide_offsets(GuideArgs A) {
    __shared__ long long s_cnt[1024];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const auto [lo, hi] = batch_slice(A.B);
    // pass 1: checks, deferral, the pairs of my trajectories
    long long n = 0;
    bool bad = false;
    if (tid == 0 && A.seg_off[0] < 0) bad = true;
    for (int b = lo; b < hi && !bad; ++b) {
        const int s0 = A.seg_off[b], s1 = A.seg_off[b + 1];
        if (s0 < 0 || s1 < s0) { bad = true; break; }
        const int N = row_count(A.n_pts, b, A.N);         // (a bad count: DEFERRED, its segments are not judged by it)
        bool deferred = N < 0;
        long long nb = 0;
        for (int k = s0; k < s1; ++k) {
            const int p0 = A.path_off[k], p1 = A.path_off[k + 1];
            if (p0 < 0 || p1 < p0 || (N > 0 && !guide_segment_ok(N, A.seg[2 * k], A.seg[2 * k + 1], p1 - p0))) { bad = true; break; }
            if (p1 - p0 > kGuidePathCap) deferred = true;
            if (N > 0) nb += guide_pushes_total(N, A.seg[2 * k], A.seg[2 * k + 1]);
        }
        n += deferred ? 0 : nb;
    }
    if (bad) s_bad = 1;
    long long total;
    const long long mine_end = scan1024(s_cnt, n, &total);
    const bool good = s_bad == 0 && total <= A.pair_cap && total <= 0x7fffffffLL;
    if (tid == 0) {
        A.result[0] = total;
        A.result[1] = s_bad;
    }
    if (!good) return;                                    // nothing else is written
    // pass 2: statuses and offsets of my trajectories
    long long at = mine_end - n;
    for (int b = lo; b < hi; ++b) {
        const int s0 = A.seg_off[b], s1 = A.seg_off[b + 1];
        const int N = row_count(A.n_pts, b, A.N);
        bool deferred = N < 0;
        for (int k = s0; k < s1; ++k)
            if (A.path_off[k + 1] - A.path_off[k] > kGuidePathCap) deferred = true;
        A.status[b] = deferred ? kGuideDeferred : kGuideOk;
        at = row_offsets(A.N, deferred ? 0 : N, at, A.off + (size_t)b * A.N, [&](int i) {
            int n_i = 0;
            for (int k = s0; k < s1; ++k) n_i += guide_pushes(N, A.seg[2 * k], A.seg[2 * k + 1], i);
            return n_i;
        });
    }
    if (tid == 1023) A.off[(size_t)A.B * A.N] = (int32_t)total;
}

__device__ __forceinline__ G3 shfl_g3(const G3& p, int lane) {
    return g3(__shfl(p.v[0], lane), __shfl(p.v[1], lane), __shfl(p.v[2], lane));
}
__device__ __forceinline__ G3 shfl_up_g3(const G3& p) {
    return g3(__shfl_up(p.v[0], 1), __shfl_up(p.v[1], 1), __shfl_up(p.v[2], 1));
}

// findGuidePointSemiCircle over the lanes; every lane returns the same found flag and (when found) guidePoint
__device__ bool find_guide_wave(int lane, int idx, int first, int second, const G3* sc, int n, G3& guidePoint) {
    const GuideAtan2 at;
    GuideFrame F;
    guide_frame(F, idx, first, second, sc[0], sc[n - 1]);
    const int steps = guide_bisect_steps();               // 11 (<= 64: one per lane)
    for (int base = 0; base + 1 < n; base += 64) {
        const int j = base + lane;
        const bool br = j + 1 < n && guide_bracket(at, F, sc[j], sc[j + 1]);
        unsigned long long mask = __ballot(br);
        while (mask) {
            const int j0 = base + (__ffsll((long long)mask) - 1);
            mask &= mask - 1;
            const G3 wpCurr = sc[j0], wpNext = sc[j0 + 1];
            G3 tempPoint = g3(0, 0, 0);
            double angleDiff = 0.0;
            if (lane < steps) angleDiff = guide_bisect_eval(at, F, wpCurr, wpNext, guide_bisect_a(lane), tempPoint);
            double prevAngleDiff = __shfl_up(angleDiff, 1);
            G3 prevTempPoint = shfl_up_g3(tempPoint);
            if (lane == 0) { prevAngleDiff = 0.0; prevTempPoint = g3(0, 0, 0); }
            const int ev = lane < steps ? guide_bisect_event(angleDiff, prevAngleDiff) : 0;
            const unsigned long long hit = __ballot(ev != 0);
            if (hit) {
                const G3 mine = guide_bisect_point(ev != 0 ? ev : 1, angleDiff, prevAngleDiff, tempPoint, prevTempPoint);
                guidePoint = shfl_g3(mine, __ffsll((long long)hit) - 1);
                return true;
            }
        }
    }
    return false;
}

__global__ void __launch_bounds__(64) k_guide_assign(GridOcc occ, GuideArgs A) {
    __shared__ G3 s_path[kGuidePathCap];
    __shared__ G3 s_sc[kGuidePathCap];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    if (A.status[b] != kGuideOk) return;                  // (the workgroup's: one value for all lanes)
    const int N = row_count(A.n_pts, b, A.N);             // > 0: k_guide_offsets defers a bad count
    const double* ctrl = A.ctrl + (size_t)b * A.N * 3;
    const int32_t* off = A.off + (size_t)b * A.N;
    const int s0 = A.seg_off[b], s1 = A.seg_off[b + 1];
    const double res = occ.g.res;
    const int ns = guide_line_samples(res);
    const int per_round = ns <= 64 ? 64 / ns : 1;         // candidate ptr2 values of one round of line checks
    G3 guidePoint = g3(0, 0, 0);

    // lane 0: segment k pushes (p, d) onto idx (a segment pushes at most one pair onto a control point)
    auto emit = [&](int k, int idx, const G3& p, const G3& d) {
        int at = off[idx];
        for (int e = s0; e < k; ++e) at += guide_pushes(N, A.seg[2 * e], A.seg[2 * e + 1], idx);
        double* o = A.pv + (size_t)at * 6;
        for (int a = 0; a < 3; ++a) { o[a] = p.v[a]; o[3 + a] = d.v[a]; }
        if (A.unk) A.unk[at] = (uint8_t)grid_plane_pos(occ.g, 1, p.v[0], p.v[1], p.v[2]);
    };

    for (int k = s0; k < s1; ++k) {
        const int first = A.seg[2 * k], second = A.seg[2 * k + 1];
        const int n = A.path_off[k + 1] - A.path_off[k];              // 1 .. kGuidePathCap (k_guide_offsets)
        const double* src = A.path + (size_t)A.path_off[k] * 3;
        __syncthreads();                                              // (the previous segment's readers are done)
        for (int i = lane; i < n; i += 64) s_path[i] = g3_load(src + 3 * (size_t)i);
        __syncthreads();
        // shortcutPath: every lane keeps ptr1, ptr2 and the count; lane 0 stores the points
        int m = 0;
        if (lane == 0) s_sc[0] = s_path[0];
        m = 1;
        if (n == 2) {
            if (lane == 0) s_sc[1] = s_path[1];
            m = 2;
        } else if (n > 2) {
            int ptr1 = 0, ptr2 = 2;
            while (ptr2 <= n - 1) {
                const int ncand = min(per_round, n - ptr2);
                bool hit = false;
                int my_cand = 0;
                for (int w = lane; w < ncand * ns && !hit; w += 64) {
                    const int cand = w / ns;
                    const G3 p = guide_line_point(s_path[ptr1], s_path[ptr2 + cand], guide_line_a(res, w % ns));
                    if (occ(p.v[0], p.v[1], p.v[2])) { hit = true; my_cand = cand; }
                }
                const unsigned long long mask = __ballot(hit);
                if (mask == 0) {                                      // ptr2 .. ptr2 + ncand - 1 are all free lines
                    if (ptr2 + ncand - 1 >= n - 1) {
                        if (lane == 0) s_sc[m] = s_path[n - 1];
                        ++m;
                        break;
                    }
                    ptr2 += ncand;
                } else {
                    const int c2 = ptr2 + __shfl(my_cand, __ffsll((long long)mask) - 1);
                    if (lane == 0) s_sc[m] = s_path[c2 - 1];
                    ++m;
                    ptr1 = c2 - 1;
                    ptr2 = ptr1 + 2;
                }
            }
        }
        __syncthreads();
        const int lo = first + 1 > 0 ? first + 1 : 0, hi = second < N ? second : N;
        for (int idx = lo; idx < hi; ++idx) {
            find_guide_wave(lane, idx, first, second, s_sc, m, guidePoint);
            if (lane == 0) {
                G3 dir;
                guide_direction(guidePoint, g3_load(ctrl + 3 * (size_t)idx), dir);
                emit(k, idx, guidePoint, dir);
            }
        }
        if (second - first - 1 == 0) {
            find_guide_wave(lane, first, first, second, s_sc, m, guidePoint);
            if (lane == 0) {
                const G3 midPoint = g3_div(g3_add(g3_load(ctrl + 3 * (size_t)first), g3_load(ctrl + 3 * (size_t)second)), 2.0);
                G3 dir;
                guide_direction(guidePoint, midPoint, dir);
                for (int idx = first - 1; idx <= second + 1; ++idx)
                    if (idx >= 3 && idx <= N - 3 - 1) emit(k, idx, guidePoint, dir);
            }
        }
    }
}

}  // namespace

int guide_path_capacity() { return kGuidePathCap; }

int launch_guide_offsets(hipStream_t s, int B, int N, const int32_t* n_pts, const int32_t* seg_off, const int32_t* seg, const int32_t* path_off,
                         long long pair_cap, int32_t* out_off, int32_t* out_status, long long* result) {
    GuideArgs a{B, N, n_pts, nullptr, seg_off, seg, path_off, nullptr, pair_cap, out_off, nullptr, nullptr, out_status, result};
    hipLaunchKernelGGL(k_guide_offsets, dim3(1), dim3(1024), 0, s, a);
    return (int)hipGetLastError();
}

int launch_guide_assign(hipStream_t s, const GridView& g, int B, int N, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off,
                        const int32_t* seg, const int32_t* path_off, const double* path, const int32_t* off, double* out_pv, uint8_t* out_unk,
                        const int32_t* status) {
    GuideArgs a{B, N, n_pts, ctrl, seg_off, seg, path_off, path, 0, const_cast<int32_t*>(off), out_pv, out_unk, const_cast<int32_t*>(status), nullptr};
    hipLaunchKernelGGL(k_guide_assign, dim3(B), dim3(64), 0, s, GridOcc{g}, a);
    return (int)hipGetLastError();
}

}  // namespace vigo
