// vigo_finish.hip — vigo_traj_finish: steps 5-6 of bsplineTraj::makePlan() and the samples of evalTrajToMsg for a batch,
// by the rule of vigo_finish_core.hpp, and vigo_traj_finish_host, the same rule on the host.  One launch, one wavefront
// (= one workgroup) per trajectory, as the gates of vigo_map.hip:
//   lanes    the row's control points into LDS, once
//   lanes    stride over the ts clock for the two maxima, then an xor-shuffle reduction with the rule's own `>` (the
//            maximum of non-NaN values does not depend on the order: the serial loop's bits)
//   lane 0   the factor, the maxima, the sample count (a binary search of the dt clock) and the status
//   lanes    stride over the output samples: consecutive lanes write consecutive pos / vel rows
// Both clocks are tables shared by the whole call (the handle caches them): no lane calls accumulated_time.
// LDS: 3 * VIGO_MAX_CTRL_POINTS doubles (6 KiB).  No atomics; every output has one writer.
#include <vector>

#include "vigo_finish_core.hpp"

namespace vigo {
namespace {

__global__ void __launch_bounds__(64) k_traj_finish(FinishArgs A) {
    __shared__ double s_ctrl[3 * VIGO_MAX_CTRL_POINTS];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= A.B) return;
    // (every branch below is wave-uniform)
    const int n = A.n_pts ? A.n_pts[b] : A.Ns;
    if (n < 7 || n > A.Ns) {                                  // nothing of the row is read, no sample row is touched
        if (lane == 0) {
            A.out_factor[b] = finish_nan();
            if (A.out_max) { A.out_max[2 * (size_t)b] = finish_nan(); A.out_max[2 * (size_t)b + 1] = finish_nan(); }
            A.out_n[b] = 0;
            A.out_status[b] = kFinishInvalidN;
        }
        return;
    }
    const double* row = A.ctrl + (size_t)b * A.Ns * 3;
    for (int i = lane; i < 3 * n; i += 64) s_ctrl[i] = row[i];
    __syncthreads();

    const double duration = finish_duration(n, A.ts_ctrl);
    double maxV = 0.0, maxA = 0.0;
    finish_maxima(s_ctrl, n, A.ts_ctrl, duration, A.T_ts, A.times_ts, lane, 64, maxV, maxA);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        finish_take_max(maxV, __shfl_xor(maxV, m, 64));
        finish_take_max(maxA, __shfl_xor(maxA, m, 64));
    }
    const int n_samp = finish_count(A.times_dt, A.T_dt, duration);
    const int n_out = n_samp < A.S_cap ? n_samp : A.S_cap;
    if (lane == 0) {
        A.out_factor[b] = finish_factor(A.limits[2 * (size_t)b], A.limits[2 * (size_t)b + 1], maxV, maxA);
        if (A.out_max) { A.out_max[2 * (size_t)b] = maxV; A.out_max[2 * (size_t)b + 1] = maxA; }
        A.out_n[b] = n_samp;
        A.out_status[b] = n_samp > A.S_cap ? kFinishCapacity : kFinishOk;
    }
    const size_t off = (size_t)b * A.S_cap * 3;
    finish_samples(s_ctrl, n, A.ts_ctrl, A.sample_dt, n_out, A.times_dt, lane, 64, A.out_pos + off, A.out_vel ? A.out_vel + off : nullptr);
}

}  // namespace

int launch_traj_finish(hipStream_t s, const FinishArgs& A) {
    if (A.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_traj_finish, dim3((unsigned)A.B), dim3(64), 0, s, A);
    return (int)hipGetLastError();
}

}  // namespace vigo

extern "C" int vigo_traj_finish_host(double ts_ctrl, double ts, int B, int Ns, const int32_t* n_pts, const double* ctrl, const double* limits,
                                     double sample_dt, int S_cap, double* out_factor, double* out_max, int32_t* out_n, double* out_pos,
                                     double* out_vel, int32_t* out_status) {
    using namespace vigo;
    if (B < 0 || S_cap < 1 || !finish_step_ok(sample_dt) || !finish_step_ok(ts) || !finish_step_ok(ts_ctrl) ||
        (B > 0 && (!ctrl || !limits || !out_factor || !out_n || !out_pos || !out_status)))
        return VIGO_ERR_INVALID_ARG;
    if (Ns < 7 || Ns > VIGO_MAX_CTRL_POINTS) return VIGO_ERR_UNSUPPORTED_N;
    if (B == 0) return VIGO_OK;
    // the two clocks as the reference runs them (t += step), up to the longest duration
    const double longest = finish_duration(Ns, ts_ctrl);
    std::vector<double> times_ts, times_dt;
    for (double t = 0.0; t < longest; t += ts) {
        if (times_ts.size() >= ((size_t)1 << 24)) return VIGO_ERR_INVALID_ARG;
        times_ts.push_back(t);
    }
    for (double t = 0.0; t <= longest; t += sample_dt) {
        if (times_dt.size() >= ((size_t)1 << 24)) return VIGO_ERR_INVALID_ARG;
        times_dt.push_back(t);
    }
    for (int b = 0; b < B; ++b) {
        const int n = n_pts ? n_pts[b] : Ns;
        if (n < 7 || n > Ns) {
            out_factor[b] = finish_nan();
            if (out_max) { out_max[2 * (size_t)b] = finish_nan(); out_max[2 * (size_t)b + 1] = finish_nan(); }
            out_n[b] = 0;
            out_status[b] = kFinishInvalidN;
            continue;
        }
        const double* row = ctrl + (size_t)b * Ns * 3;
        const double duration = finish_duration(n, ts_ctrl);
        double maxV = 0.0, maxA = 0.0;
        finish_maxima(row, n, ts_ctrl, duration, (int)times_ts.size(), times_ts.data(), 0, 1, maxV, maxA);
        const int n_samp = finish_count(times_dt.data(), (int)times_dt.size(), duration);
        const int n_out = n_samp < S_cap ? n_samp : S_cap;
        out_factor[b] = finish_factor(limits[2 * (size_t)b], limits[2 * (size_t)b + 1], maxV, maxA);
        if (out_max) { out_max[2 * (size_t)b] = maxV; out_max[2 * (size_t)b + 1] = maxA; }
        out_n[b] = n_samp;
        out_status[b] = n_samp > S_cap ? kFinishCapacity : kFinishOk;
        const size_t off = (size_t)b * S_cap * 3;
        finish_samples(row, n, ts_ctrl, sample_dt, n_out, times_dt.data(), 0, 1, out_pos + off, out_vel ? out_vel + off : nullptr);
    }
    return VIGO_OK;
}
