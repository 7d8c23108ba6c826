// vigo_traj_core.hpp — the per-trajectory stages of the whole-trajectory checkers, shared by vigo_traj_corridor_check
// (vigo_traj_corridor.hip: box sweep, PO.cpp:634-656) and vigo_traj_point_check (vigo_traj_point.hip: point lookup,
// PM.cpp:524-546).  Around a middle stage of each entry's own, which fills the runs' flag / first hit / count:
//   k_traj_csr     is seg_off a CSR over [0, S]?
//   k_traj_runs    a thread per trajectory: status, sample count, clock table, the segments' runs (vigo_traj_runs.hpp)
//   k_traj_finish  a thread per trajectory: the leading default-pose run, the runs in segment order, the endpoint, the
//                  attribution — templated on the entry's test of one pose
// No atomics on results: every output has one writer.  (An anonymous-namespace header like vigo_corridor_core.hpp:
// each translation unit gets its own instantiations.)
#pragma once

#include "vigo_internal.hpp"
#include "vigo_traj_runs.hpp"

namespace vigo {
namespace {

struct TrajWork {
    const int32_t* seg_off;
    const double* knots;
    const double* delT;
    const double* endpoint;
    int T, S;
    int t_lo, t_hi;
    const int* csr_bad;          // set by k_traj_csr: seg_off is no CSR over [0, S], every trajectory is rejected
    ClockTable* clocks;          // [t_hi - t_lo]
    int32_t* slot_status;        // [t_hi - t_lo] each
    int32_t* slot_n;
    int32_t* slot_lead;
    int32_t* slot_end_seg;
    int32_t* run_first;          // [S] each
    int32_t* run_len;
    int32_t* seg_traj;
    int* todo;
    uint8_t* run_flag;
    int32_t* run_hit;            // first colliding sample of the run, local index, or -1
    int32_t* run_count;
};

// the workspace of one call: [T_chunk] clock tables, [T_chunk] x 4 per-trajectory ints, [S] x 6 per-segment ints, the
// CSR flag, [S] flags
inline size_t traj_work_bytes(int S, int T_chunk) {
    const size_t seg = (size_t)S * (6 * sizeof(int32_t) + 1);
    return (size_t)T_chunk * (sizeof(ClockTable) + 4 * sizeof(int32_t)) + seg + 64;
}

__global__ void k_traj_csr(int T, int S, const int32_t* __restrict__ seg_off, int* bad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > T) return;
    const int a = seg_off[i];
    if (a < 0 || a > S || (i < T && a > seg_off[i + 1])) atomicOr(bad, 1);
}

__global__ void __launch_bounds__(64) k_traj_runs(TrajWork W) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = W.t_lo + slot;
    if (t >= W.t_hi) return;
    ClockTable& C = W.clocks[slot];
    C.n = -1;
    W.slot_n[slot] = 0;
    W.slot_lead[slot] = 0;
    W.slot_end_seg[slot] = -1;
    if (*W.csr_bad) { W.slot_status[slot] = kTrajBadOffsets; return; }   // (segments left alone: nobody owns them)
    const int a = W.seg_off[t], K = W.seg_off[t + 1] - a;
    const double* k = W.knots + a + t;
    const double d = W.delT[t];
    int st = traj_knots_status(K, k);
    int64_t n = 0;
    if (st == kTrajOk) st = traj_sample_count(k[K], d, &n);
    W.slot_status[slot] = st;
    for (int i = 0; i < K; ++i) {
        W.seg_traj[a + i] = t;
        W.run_first[a + i] = 0;
        W.run_len[a + i] = 0;
        W.todo[a + i] = 0;
        W.run_flag[a + i] = 0;
        W.run_hit[a + i] = -1;
        W.run_count[a + i] = 0;
    }
    if (st != kTrajOk) return;
    (void)build_clock_table(d, (int)n, C);
    int32_t lead, end_seg;
    traj_runs(K, k, d, n, &C, &lead, W.run_first + a, W.run_len + a, 1, &end_seg);
    W.slot_n[slot] = (int32_t)n;
    W.slot_lead[slot] = lead;
    W.slot_end_seg[slot] = end_seg;
}

// Hit: the entry's test of one fp64 pose, `__device__ bool operator()(double x, double y, double z) const`
template <class Hit>
__global__ void __launch_bounds__(64) k_traj_finish(Hit hit, TrajWork W, int32_t* __restrict__ out_status,
                                                    int32_t* __restrict__ out_n, uint8_t* __restrict__ out_flag,
                                                    int32_t* __restrict__ out_first, int32_t* __restrict__ out_count,
                                                    uint8_t* __restrict__ out_seg) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = W.t_lo + slot;
    if (t >= W.t_hi) return;
    const int st = W.slot_status[slot];
    out_status[t] = st;
    int first = -1, count = 0;
    if (st == kTrajOk) {
        const int n = W.slot_n[slot], lead = W.slot_lead[slot];
        // the leading run: samples before k[0], all at the default pose — one test decides them all (no segment)
        if (lead > 0 && hit(0.0, 0.0, 0.0)) { first = 0; count = lead; }
        const int a = W.seg_off[t], b = W.seg_off[t + 1];
        for (int sg = a; sg < b; ++sg) {                      // runs in segment order = ascending sample indices
            if (!W.run_flag[sg]) continue;
            if (first < 0) first = W.run_first[sg] + W.run_hit[sg];
            count += W.run_count[sg];
            out_seg[sg] = 1;
        }
        // the endpoint (sample n): the last waypoint as given, attributed when its clock equals k[K]
        const double* e = W.endpoint + (size_t)t * 3;
        if (hit(e[0], e[1], e[2])) {
            if (first < 0) first = n;
            ++count;
            if (W.slot_end_seg[slot] >= 0) out_seg[a + W.slot_end_seg[slot]] = 1;
        }
        out_n[t] = n + 1;
    } else {
        out_n[t] = 0;
    }
    out_flag[t] = (uint8_t)(count > 0);
    out_first[t] = first;
    if (out_count) out_count[t] = count;
}

// The common start of a call: clears out_seg; for T > 0 lays W over ws (traj_work_bytes(S, T_chunk) bytes), clears the
// CSR flag and the segment owners and launches k_traj_csr.  W.t_lo / W.t_hi are the caller's, per chunk.
inline hipError_t traj_prepare(hipStream_t s, void* ws, int T, int S, int T_chunk, const int32_t* seg_off, const double* knots,
                               const double* delT, const double* endpoint, uint8_t* out_seg, TrajWork& W) {
    if (S > 0) {
        hipError_t e = hipMemsetAsync(out_seg, 0, (size_t)S, s);
        if (e != hipSuccess) return e;
    }
    if (T <= 0) return hipSuccess;
    char* p = static_cast<char*>(ws);
    W = TrajWork{};
    W.seg_off = seg_off; W.knots = knots; W.delT = delT; W.endpoint = endpoint;
    W.T = T; W.S = S;
    W.clocks = reinterpret_cast<ClockTable*>(p); p += (size_t)T_chunk * sizeof(ClockTable);
    W.slot_status = reinterpret_cast<int32_t*>(p); p += (size_t)T_chunk * 4;
    W.slot_n = reinterpret_cast<int32_t*>(p); p += (size_t)T_chunk * 4;
    W.slot_lead = reinterpret_cast<int32_t*>(p); p += (size_t)T_chunk * 4;
    W.slot_end_seg = reinterpret_cast<int32_t*>(p); p += (size_t)T_chunk * 4;
    W.run_first = reinterpret_cast<int32_t*>(p); p += (size_t)S * 4;
    W.run_len = reinterpret_cast<int32_t*>(p); p += (size_t)S * 4;
    W.seg_traj = reinterpret_cast<int32_t*>(p); p += (size_t)S * 4;
    W.todo = reinterpret_cast<int*>(p); p += (size_t)S * 4;
    W.run_hit = reinterpret_cast<int32_t*>(p); p += (size_t)S * 4;
    W.run_count = reinterpret_cast<int32_t*>(p); p += (size_t)S * 4;
    int* bad = reinterpret_cast<int*>(p); p += 4;
    W.run_flag = reinterpret_cast<uint8_t*>(p);
    W.csr_bad = bad;
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), s);
    if (e == hipSuccess && S > 0) e = hipMemsetAsync(W.seg_traj, 0xff, (size_t)S * 4, s);   // -1: no trajectory (yet)
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_traj_csr, dim3((T + 1 + 255) / 256), dim3(256), 0, s, T, S, seg_off, bad);
    return hipSuccess;
}

}  // namespace
}  // namespace vigo
