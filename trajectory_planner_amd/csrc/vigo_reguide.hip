// vigo_reguide.hip — the rebound loop of bsplineTraj::optimizeTrajectory (BT.cpp:611-685) between two solves: the gate
// + decision pass and the compaction of vigo_rebound_rounds, and vigo_rebound_reguide, the re-guide step (the
// `if (hasCollision)` block of BT.cpp:656-679; host/src/bsplineTraj.cpp: reboundStep) for the trajectories the rounds
// left VIGO_RB_NEEDS_HOST.  The rules are vigo_reguide_core.hpp's (reguide_rules is asked by both: the yes/no by
// k_rebound_decide, the list by k_reguide_list), around the gates of vigo_grid.hpp, the path search of
// vigo_pathsearch.hip and the guide step of vigo_guides.hip (both unchanged: the re-guide list is a caller-supplied list
// to the first, its output the input of the second).
//
// A round of vigo_rebound_rounds: k_rebound_decide (a wave per trajectory), k_rebound_compact (one workgroup), the solve.
// The kernels of one vigo_rebound_reguide call, in stream order (vigo_api.cpp reads back the words marked <-):
//   k_reguide_list          a wave per trajectory   eligibility; the map queries of findCollisionSeg one control point per
//                                                   lane; lane 0 walks reguide_rules over the flags in LDS: the new
//                                                   segments and the re-guide list, at a fixed stride  <- bad guide_off
//   k_ps_* / k_astar        vigo_path_search's chain on the lists                      <- its three counts
//   k_guide_offsets / k_guide_assign   vigo_guide_assign's pair on its output          <- the new pairs
//   k_guide_merge_offsets   one workgroup           the outcome of every trajectory (reguide_outcome), its pairs per
//                                                   control point (old + appended), scanned; the offsets are written
//                                                   only when the total fits pair_cap            <- the merged pairs
//   k_guide_merge           a wave per trajectory   the merged CSR, a pair per lane: old pairs, then this step's
//   k_reguide_commit        a thread per trajectory reguide_commit: state, weights, out_status
// Nothing of the caller's is written before k_guide_merge_offsets has passed.  Plain vector stores, no atomics.
#include "vigo_reguide_core.hpp"
#include "vigo_guide_core.hpp"
#include "vigo_rows_core.hpp"
#include "vigo_grid.hpp"
#include "vigo_scan.hpp"

namespace vigo {
namespace {

constexpr int kSegs = VIGO_MAX_COLLISION_SEGS;
static_assert(kSegs == kPathsMaxSegs, "the state holds what the path search takes");

// the map queries of findCollisionSeg (BT.cpp:412, :435) for one trajectory over the lanes of its wave, a control point
// per lane: s_pt[i] the point flag, then s_ln[i] the line (i - 1, i) from the flags of its ends.  Every lane calls it.
__device__ __forceinline__ void ctrl_flags_wave(const GridView& g, const double* c, int N, int lane, uint8_t* s_pt, uint8_t* s_ln) {
    for (int i = lane; i < N; i += 64) s_pt[i] = (uint8_t)grid_plane_pos(g, 0, c[3 * i], c[3 * i + 1], c[3 * i + 2]);
    __syncthreads();
    for (int i = lane; i < N; i += 64) {
        unsigned line = 0;
        if (i > 0) {
            line = s_pt[i - 1] | s_pt[i];
            if (!line) line = line_interior_occupied(GridOcc{g}, g.res, c + 3 * (i - 1), c + 3 * i) ? 1u : 0u;
        }
        s_ln[i] = (uint8_t)line;
    }
    __syncthreads();
}

// isControlPointRequireNewGuide (BT.h:417-429) of control point i of one trajectory: off its guide offsets [N + 1] or
// NULL, pv the pairs, c its control points.  A control point without guide arrays needs a guide.
struct NeedGuide {
    const int32_t* off;
    const double* pv;
    const double* c;
    double dthresh;
    __device__ bool operator()(int i) const {
        if (!off || !pv) return true;
        const int j0 = off[i], j1 = off[i + 1];
        if (j0 < 0) return true;                          // (a bad list: the call is refused, read nothing)
        for (int j = j0; j < j1; ++j)
            if (!reguide_guide_far(dthresh, c + 3 * i, pv + 6 * (size_t)j)) return false;
        return true;
    }
};

// ---- vigo_rebound_rounds: gates + the loop body of bsplineTraj::optimizeTrajectory (BT.cpp:619-679) ----------
// One 64-lane wave per ACTIVE trajectory.  The gates are the walks of vigo_grid.hpp (lanes stride over the samples); the
// map queries of findCollisionSeg run one control point per lane; the segment bookkeeping, the comparison with the
// previous segments and the guide test (reguide_rules) are a serial scan by lane 0 over a few dozen bytes in LDS.
__global__ void __launch_bounds__(64) k_rebound_decide(GridView g, ReboundArgs A) {
    __shared__ uint8_t s_pt[VIGO_MAX_CTRL_POINTS], s_ln[VIGO_MAX_CTRL_POINTS];
    __shared__ int s_need_host;
    const int b = blockIdx.x;
    if (b >= A.B) return;
    // a trajectory of an EARLIER round waits for the host (A*): the queued rounds that follow are no-ops for the whole
    // batch, like the lock-step of the host-driven loop — the waiting trajectories are on the batch's critical path
    if (A.flags[1] != 0) return;
    vigo_rebound_state_t& st = A.state[b];
    if (st.status != VIGO_RB_ACTIVE) return;
    // (vigo_rebound_rounds_mixed) rows of A.N control points, n_pts[b] of them this trajectory's, and its gates' sample
    // counts from the per-count table; k_rebound_check_counts has taken every count outside [7, A.N] out of the ACTIVE set
    const int lane = threadIdx.x;
    const int N = A.n_pts ? min(max(A.n_pts[b], 7), A.N) : A.N;   // (device data: never index beyond the row)
    const int T = A.n_pts ? A.count_tab[2 * (N - 7)] : A.T, T_static = A.n_pts ? A.count_tab[2 * (N - 7) + 1] : A.T_static;
    const double* c = A.ctrl + (size_t)b * A.N * 3;

    const int col = __any(gate_static_first(g, c, N, A.ts_ctrl, T_static, A.times, lane) != INT_MAX) ? 1 : 0;
    const int dyn = __any(gate_dynamic_hit(c, N, A.ts_ctrl, T, A.times, A.obs_off, A.obs, A.n_obs_shared, b, lane)) ? 1 : 0;
    if (lane == 0) {
        st.gate_static = col;
        st.gate_dynamic = dyn;
        st.rounds += 1;
    }
    if (!col && !dyn) {                                   // BT.cpp:628-631
        if (lane == 0) st.status = VIGO_RB_DONE;
        return;
    }
    if (st.fail_count >= 4) {                             // BT.cpp:640-654: forced A* re-guide, the host's
        if (lane == 0) { st.status = VIGO_RB_NEEDS_HOST; A.flags[2] = 1; }
        return;
    }
    if (col) {
        ctrl_flags_wave(g, c, N, lane, s_pt, s_ln);
        if (lane == 0) {
            // isReguideRequired, BT.cpp:573-608: a trajectory with a re-guide list (or more segments than the state
            // holds) asks for A*
            int32_t seg[2 * kSegs];
            uint8_t listed[kSegs];
            int n_list = 0;
            const int n_prev = min(max(st.n_seg, 0), kSegs);   // (device data: never index beyond the array)
            const NeedGuide need_guide{A.guide_off ? A.guide_off + (size_t)b * A.N : nullptr, A.guide_pv, c, A.dthresh};
            const int n = reguide_rules(N, A.not_check_ratio, FlagOcc{s_pt}, FlagOcc{s_ln}, n_prev, st.seg, need_guide, kSegs, seg, listed, &n_list);
            const bool need_host = n > kSegs || n_list != 0;
            s_need_host = need_host ? 1 : 0;
            if (need_host) {
                st.status = VIGO_RB_NEEDS_HOST;           // untouched state: the host repeats the step with its own A*
                A.flags[2] = 1;
            } else {
                st.n_seg = n;                             // collisionSeg_ = the new segments (BT.cpp:575)
                for (int k = 0; k < 2 * n; ++k) st.seg[k] = seg[k];
                A.weights[4 * (size_t)b + 0] *= 2.0;      // BT.cpp:672
                st.fail_count += 1;
            }
        }
        __syncthreads();
        if (s_need_host) return;
    }
    if (dyn && lane == 0) A.weights[4 * (size_t)b + 3] *= 2.0;   // BT.cpp:677-679
}

// ascending indices of the trajectories a launch works on: one block, a scan over per-thread counts
// flags: [0] = count (out), [1] = "a trajectory waits for the host since an earlier round" (read by this round's
// kernels), [2] = the same as raised by this round's decide pass; mode 1 publishes [2] into [1] for the next round
__global__ void __launch_bounds__(1024) k_rebound_compact(int B, vigo_rebound_state_t* __restrict__ state, int mode,
                                                          int32_t* __restrict__ idx, int32_t* __restrict__ flags) {
    __shared__ int s_cnt[1024];
    const int tid = threadIdx.x;
    int32_t* count = flags;
    if (mode == 1 && flags[1] != 0) {            // (uniform: every thread reads the same word)
        if (tid == 0) *count = 0;
        return;
    }
    const auto [lo, hi] = batch_slice(B);
    if (mode == 1 && flags[2] != 0) {            // (uniform too)
        // this round's decisions hand a trajectory to the host: the optimize() the still-active trajectories owe is
        // deferred to the caller's next call (solve_first), where it shares ONE launch with the re-guided ones —
        // two launches in a row would put two solve latencies on the batch's critical path
        for (int b = lo; b < hi; ++b)
            if (state[b].status == VIGO_RB_ACTIVE) state[b].solve_first = 1;
        if (tid == 0) { *count = 0; flags[1] = 1; }
        return;
    }
    auto wanted = [&](int b) {
        return state[b].status == VIGO_RB_ACTIVE && (mode == 1 || state[b].solve_first != 0);
    };
    int n = 0;
    for (int b = lo; b < hi; ++b) n += wanted(b) ? 1 : 0;
    int total;
    int at = scan1024(s_cnt, n, &total) - n;
    for (int b = lo; b < hi; ++b) {
        if (wanted(b)) {
            idx[at++] = b;
            if (mode == 0) state[b].solve_first = 0;
        }
    }
    if (tid == 1023) {
        *count = total;
        if (mode == 1) flags[1] = flags[2];
    }
}

__global__ void __launch_bounds__(64) k_reguide_list(GridView g, ReguideArgs A) {
    __shared__ uint8_t s_pt[VIGO_MAX_CTRL_POINTS], s_ln[VIGO_MAX_CTRL_POINTS];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int32_t* off = A.guide_off ? A.guide_off + (size_t)b * A.N : nullptr;
    if (off) {                                            // (every trajectory's offsets, the whole row: the merge copies them all)
        bool bad = b == 0 && lane == 0 && off[0] < 0;
        for (int i = lane; i < A.N; i += 64) bad = bad || off[i + 1] < off[i];
        if (bad) A.result[0] = 1;                         // (the same value from whoever sees one)
    }
    // (vigo_rebound_reguide_mixed) the trajectory's own count in a row of A.N; a bad count defers it, state untouched
    const int N = row_count(A.n_pts, b, A.N);
    if (N < 0) {                                          // (the workgroup's)
        if (lane == 0) { A.kind[b] = kReguideDeferred; A.n_list[b] = 0; A.n_new[b] = 0; }
        return;
    }
    const vigo_rebound_state_t& st = A.state[b];
    if (!(st.status == VIGO_RB_NEEDS_HOST && st.gate_static != 0 && st.fail_count < 4)) {     // (the workgroup's)
        if (lane == 0) { A.kind[b] = kReguideSkipped; A.n_list[b] = 0; A.n_new[b] = 0; }
        return;
    }
    const double* c = A.ctrl + (size_t)b * A.N * 3;
    ctrl_flags_wave(g, c, N, lane, s_pt, s_ln);
    if (lane != 0) return;
    int32_t seg[2 * kSegs];
    uint8_t listed[kSegs];
    int n_list = 0;
    const int n_prev = min(max(st.n_seg, 0), kSegs);      // (device data: never index beyond the array)
    const NeedGuide need_guide{off, A.guide_pv, c, A.dthresh};
    const int n = reguide_rules(N, A.not_check_ratio, FlagOcc{s_pt}, FlagOcc{s_ln}, n_prev, st.seg, need_guide, kSegs, seg, listed, &n_list);
    if (n > kSegs) {
        A.kind[b] = kReguideDeferred; A.n_list[b] = 0; A.n_new[b] = 0;
        return;
    }
    int32_t* dst_new = A.new_seg + 2 * (size_t)kSegs * b;
    int32_t* dst_list = A.list + 2 * (size_t)kSegs * b;
    int m = 0;
    for (int k = 0; k < n; ++k) {
        dst_new[2 * k] = seg[2 * k];
        dst_new[2 * k + 1] = seg[2 * k + 1];
        if (listed[k]) {
            dst_list[2 * m] = seg[2 * k];
            dst_list[2 * m + 1] = seg[2 * k + 1];
            ++m;
        }
    }
    A.kind[b] = -1;
    A.n_list[b] = m;
    A.n_new[b] = n;
}

__global__ void __launch_bounds__(1024) k_guide_merge_offsets(ReguideArgs A) {
    __shared__ long long s_cnt[1024];
    const int tid = threadIdx.x, N = A.N;
    const auto [lo, hi] = batch_slice(A.B);
    auto old_pairs = [&](size_t at) { return A.guide_off ? A.guide_off[at + 1] - A.guide_off[at] : 0; };
    // pass 1: the outcomes and the pairs of my trajectories
    long long n = 0;
    for (int b = lo; b < hi; ++b) {
        const int kind = A.kind[b], ps = A.ps_status[b];
        const bool cut = ps == kPathsOk && paths_cut_by_bound(A.ps_counts[2 * b], A.ps_seg_off[b + 1] - A.ps_seg_off[b]);
        const int outcome = reguide_outcome(kind != kReguideSkipped, kind == kReguideDeferred, A.n_list[b], ps, cut, A.g_status[b] == kGuideDeferred);
        A.outcome[b] = outcome;
        if (A.guide_off) n += (long long)A.guide_off[(size_t)(b + 1) * N] - A.guide_off[(size_t)b * N];
        if (outcome == kReguideDone) n += (long long)A.g_off[(size_t)(b + 1) * N] - A.g_off[(size_t)b * N];
    }
    long long total;
    const long long mine_end = scan1024(s_cnt, n, &total);
    if (tid == 0) A.result[1] = total;
    if (total > A.pair_cap || total > 0x7fffffffLL) return;                   // nothing else is written
    // pass 2: the merged offsets of my trajectories
    // (every control point of the row, whatever the count: the old pairs are copied, the padding's ranges are empty)
    long long at = mine_end - n;
    for (int b = lo; b < hi; ++b) {
        const bool done = A.outcome[b] == kReguideDone;
        at = row_offsets(N, N, at, A.out_guide_off + (size_t)b * N, [&](int i) {
            const size_t q = (size_t)b * N + i;
            return old_pairs(q) + (done ? A.g_off[q + 1] - A.g_off[q] : 0);
        });
    }
    if (tid == 1023) A.out_guide_off[(size_t)A.B * N] = (int32_t)total;
}

__global__ void __launch_bounds__(64) k_guide_merge(GridView g, ReguideArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x, N = A.N;
    const int32_t* out_off = A.out_guide_off + (size_t)b * N;
    const bool done = A.outcome[b] == kReguideDone;       // (one value for all lanes; the offsets hold new pairs only then)
    for (int q = out_off[0] + lane; q < out_off[N]; q += 64) {
        const int lo = row_slot_owner(out_off, N, q);     // the control point of slot q, searched over the whole row
        const size_t at = (size_t)b * N + lo;
        const int j = q - out_off[lo];
        const int n_old = A.guide_off ? A.guide_off[at + 1] - A.guide_off[at] : 0;
        const double* src;
        unsigned unk = 0;
        if (j < n_old) {
            const size_t s = (size_t)A.guide_off[at] + j;
            src = A.guide_pv + 6 * s;
            if (A.out_guide_unk) unk = A.guide_unk ? A.guide_unk[s] : grid_plane_pos(g, 1, src[0], src[1], src[2]);
        } else {
            if (!done) continue;                          // (cannot be: the slot would not exist)
            const size_t s = (size_t)A.g_off[at] + (j - n_old);
            src = A.g_pv + 6 * s;
            if (A.out_guide_unk) unk = A.g_unk[s];
        }
        double* dst = A.out_guide_pv + 6 * (size_t)q;
        for (int a = 0; a < 6; ++a) dst[a] = src[a];
        if (A.out_guide_unk) A.out_guide_unk[q] = (uint8_t)unk;
    }
}

__global__ void __launch_bounds__(256) k_reguide_commit(ReguideArgs A) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    const int outcome = A.outcome[b];
    A.out_status[b] = outcome;
    if (outcome == kReguideDeferred || outcome == kReguideSkipped) return;
    vigo_rebound_state_t& st = A.state[b];
    const int n = A.n_new[b];                             // <= kSegs (k_reguide_list)
    const int32_t* src = A.new_seg + 2 * (size_t)kSegs * b;
    st.n_seg = n;                                         // collisionSeg_ = the new segments (BT.cpp:575)
    for (int k = 0; k < 2 * n; ++k) st.seg[k] = src[k];
    reguide_commit(outcome, st.gate_dynamic != 0, A.weights + 4 * (size_t)b, &st.fail_count, &st.status, &st.solve_first);
}

}  // namespace

// vigo_rebound_rounds_mixed, before anything else: a count that breaks the contract (outside [7, Ns], or of the other
// shape class than Ns) takes its ACTIVE trajectory out of the set — NEEDS_HOST with LBFGSERR_INVALID_N (-1021), no wait
// flag: the host solves such a planner itself, the rest of the batch goes on
__global__ void __launch_bounds__(256) k_rebound_check_counts(int B, int Ns, const int32_t* __restrict__ n_pts, vigo_rebound_state_t* __restrict__ state) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B || state[b].status != VIGO_RB_ACTIVE) return;
    const int n = n_pts[b];
    if (n >= 7 && n <= Ns && (n <= 32) == (Ns <= 32)) return;
    state[b].status = VIGO_RB_NEEDS_HOST;
    state[b].lbfgs_status = -1021;
}
int launch_rebound_check_counts(hipStream_t s, int B, int Ns, const int32_t* n_pts, vigo_rebound_state_t* state) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rebound_check_counts, dim3((B + 255) / 256), dim3(256), 0, s, B, Ns, n_pts, state);
    return (int)hipGetLastError();
}

int launch_rebound_decide(hipStream_t s, const GridView& g, const ReboundArgs& a) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rebound_decide, dim3(a.B), dim3(64), 0, s, g, a);
    return (int)hipGetLastError();
}

int launch_rebound_compact(hipStream_t s, int B, vigo_rebound_state_t* state, int mode, int32_t* idx, int32_t* flags) {
    hipLaunchKernelGGL(k_rebound_compact, dim3(1), dim3(1024), 0, s, B, state, mode, idx, flags);
    return (int)hipGetLastError();
}

int launch_reguide_list(hipStream_t s, const GridView& g, const ReguideArgs& a) {
    hipLaunchKernelGGL(k_reguide_list, dim3(a.B), dim3(64), 0, s, g, a);
    return (int)hipGetLastError();
}

int launch_guide_merge_offsets(hipStream_t s, const ReguideArgs& a) {
    hipLaunchKernelGGL(k_guide_merge_offsets, dim3(1), dim3(1024), 0, s, a);
    return (int)hipGetLastError();
}

int launch_guide_merge(hipStream_t s, const GridView& g, const ReguideArgs& a) {
    hipLaunchKernelGGL(k_guide_merge, dim3(a.B), dim3(64), 0, s, g, a);
    return (int)hipGetLastError();
}

int launch_reguide_commit(hipStream_t s, const ReguideArgs& a) {
    hipLaunchKernelGGL(k_reguide_commit, dim3((a.B + 255) / 256), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

}  // namespace vigo
