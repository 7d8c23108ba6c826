// vigo_validate.hip — vigo_traj_validate: which of a batch of held plans are still valid on the current map, by the rule of
// vigo_validate_core.hpp, and vigo_traj_validate_host, the same rule on the host.  Two launches:
//   k_traj_validate       a wavefront per trajectory, kWaves per workgroup
//     lanes   the row's n control points into the wave's slice of LDS, once
//     lanes   sample base + lane of a block of 64, evaluated once for the static and the dynamic check; two ballots give
//             the block's first hits (the lane that holds the static one writes the position); one uniform test
//             (validate_done) decides whether a later block can still matter, and the wave leaves when none can
//     lane 0  status, first, dyn_first
//   k_validate_list       one workgroup: the rows with a status, ascending, by a scan over the statuses
// The clock and the per-count sample counts are tables shared by the whole call (the handle caches them).
// LDS: kWaves * 3 * VIGO_MAX_CTRL_POINTS doubles (24 KiB).  No atomics; every output has one writer.
#include <vector>

#include "vigo_scan.hpp"
#include "vigo_seed_core.hpp"
#include "vigo_validate_core.hpp"

#include "../../include/vigo_validate.h"

namespace vigo {
namespace {

static_assert(kValidStatic == VIGO_VALID_STATIC && kValidDynamic == VIGO_VALID_DYNAMIC && kValidBadCount == VIGO_VALID_BAD_COUNT &&
                  kValidateByTime == VIGO_VALIDATE_BY_TIME && kValidateByIndex == VIGO_VALIDATE_BY_INDEX,
              "the core's constants are the header's");

constexpr int kWaves = 4;

__global__ void __launch_bounds__(64 * kWaves) k_traj_validate(GridView g, ValidateArgs A) {
    __shared__ double s_ctrl[kWaves][3 * VIGO_MAX_CTRL_POINTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWaves + wave;
    // (every branch below is wave-uniform; the barrier is reached by every wave of the workgroup)
    const bool row = b < A.B;
    const int n = !row ? 0 : (A.n_pts ? A.n_pts[b] : A.Ns);
    const bool good = row && validate_count_ok(n, A.Ns);
    double* c = s_ctrl[wave];
    if (good) {
        const double* src = A.ctrl + (size_t)b * A.Ns * 3;
        for (int i = lane; i < 3 * n; i += 64) c[i] = src[i];
    }
    __syncthreads();
    if (!row) return;
    if (!good) {                                              // nothing of the row is read, out_pos is not touched
        if (lane == 0) {
            A.out_status[b] = kValidBadCount;
            A.out_first[b] = -1;
            if (A.out_dyn_first) A.out_dyn_first[b] = -1;
        }
        return;
    }
    ValidateRow r;
    r.n = n;
    r.S = min(A.count_tab[2 * (n - kValidateMinN)], A.T);     // (never beyond the clock table)
    r.C = min(A.count_tab[2 * (n - kValidateMinN) + 1], r.S);
    validate_obs_range(A.obs_off, A.obs, A.n_obs_shared, b, r.o0, r.o1);
    const GridOcc occ{g};
    int first = -1, dyn_first = -1;
    for (int base = 0; base < r.S; base += 64) {
        double p[3];
        const int bits = validate_sample(c, r, A.ts_ctrl, A.times, base + lane, occ, A.obs, first < 0, dyn_first < 0, p);
        const unsigned long long ms = __ballot(bits & kValidStatic), md = __ballot(bits & kValidDynamic);
        if (first < 0 && ms) {
            const int l = __ffsll((long long)ms) - 1;
            first = base + l;
            if (lane == l && A.out_pos)
                for (int a = 0; a < 3; ++a) A.out_pos[3 * (size_t)b + a] = finish_sample(p[a]);
        }
        if (dyn_first < 0 && md) dyn_first = base + __ffsll((long long)md) - 1;
        if (validate_done(r, base, 64, first, dyn_first)) break;
    }
    if (lane == 0) {
        A.out_status[b] = validate_status(first, dyn_first);
        A.out_first[b] = first;
        if (A.out_dyn_first) A.out_dyn_first[b] = dyn_first;
    }
}

// out_invalid[0 .. *out_n_invalid): the b with out_status[b] != 0, ascending; entries beyond are not written
__global__ void __launch_bounds__(1024) k_validate_list(int B, const int32_t* __restrict__ status, int32_t* __restrict__ out_invalid,
                                                        int32_t* __restrict__ out_n_invalid) {
    __shared__ int s_cnt[1024];
    const auto [lo, hi] = batch_slice(B);
    int n = 0;
    for (int b = lo; b < hi; ++b) n += status[b] != 0 ? 1 : 0;
    int total;
    int at = scan1024(s_cnt, n, &total) - n;
    for (int b = lo; b < hi; ++b)
        if (status[b] != 0) out_invalid[at++] = b;
    if (threadIdx.x == 0) *out_n_invalid = total;
}

}  // namespace

int launch_traj_validate(hipStream_t s, const GridView& g, const ValidateArgs& A) {
    if (A.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_traj_validate, dim3((unsigned)((A.B + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s, g, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !A.out_invalid) return (int)e;
    hipLaunchKernelGGL(k_validate_list, dim3(1), dim3(1024), 0, s, A.B, A.out_status, A.out_invalid, A.out_n_invalid);
    return (int)hipGetLastError();
}

}  // namespace vigo

extern "C" int vigo_traj_validate_host(int nx, int ny, int nz, const double origin[3], double res, const uint8_t* voxels_host, double ts_ctrl,
                                       int B, int Ns, const int32_t* n_pts, const double* ctrl, double dt, double not_check_ratio, int rule,
                                       const int32_t* obs_off, const double* obs, int n_obs_shared, int32_t* out_status, int32_t* out_first,
                                       double* out_pos, int32_t* out_dyn_first, int32_t* out_invalid, int32_t* out_n_invalid) {
    using namespace vigo;
    if (nx < 1 || ny < 1 || nz < 1 || !origin || !voxels_host || !finish_step_ok(res) || B < 0 || !finish_step_ok(dt) || !finish_step_ok(ts_ctrl) ||
        !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0) || (rule != kValidateByTime && rule != kValidateByIndex) || n_obs_shared < 0 ||
        (B > 0 && (!ctrl || !out_status || !out_first)) || (!out_invalid != !out_n_invalid))
        return VIGO_ERR_INVALID_ARG;
    if (Ns < kValidateMinN || Ns > VIGO_MAX_CTRL_POINTS) return VIGO_ERR_UNSUPPORTED_N;
    if (B == 0) return VIGO_OK;
    std::vector<int32_t> tab((size_t)validate_tab_entries(Ns));
    for (int n = kValidateMinN; n <= Ns; ++n)
        if (!validate_counts(dt, ts_ctrl, not_check_ratio, rule, n, &tab[2 * (n - kValidateMinN)], &tab[2 * (n - kValidateMinN) + 1]))
            return VIGO_ERR_INVALID_ARG;
    // the clock as the reference runs it (t += dt), up to the longest duration
    const int T = tab[2 * (Ns - kValidateMinN)];
    std::vector<double> times((size_t)T);
    double t = 0.0;
    for (int k = 0; k < T; ++k, t += dt) times[k] = t;
    const SeedByteGrid occ{voxels_host, nx, ny, nz, {origin[0], origin[1], origin[2]}, res};
    int n_invalid = 0;
    for (int b = 0; b < B; ++b) {
        const int n = n_pts ? n_pts[b] : Ns;
        if (!validate_count_ok(n, Ns)) {
            out_status[b] = kValidBadCount;
            out_first[b] = -1;
            if (out_dyn_first) out_dyn_first[b] = -1;
        } else {
            ValidateRow r;
            r.n = n;
            r.S = tab[2 * (n - kValidateMinN)];
            r.C = tab[2 * (n - kValidateMinN) + 1];
            validate_obs_range(obs_off, obs, n_obs_shared, b, r.o0, r.o1);
            const double* c = ctrl + (size_t)b * Ns * 3;
            int first = -1, dyn_first = -1;
            for (int k = 0; k < r.S; ++k) {
                double p[3];
                const int bits = validate_sample(c, r, ts_ctrl, times.data(), k, occ, obs, first < 0, dyn_first < 0, p);
                if (first < 0 && (bits & kValidStatic)) {
                    first = k;
                    if (out_pos)
                        for (int a = 0; a < 3; ++a) out_pos[3 * (size_t)b + a] = finish_sample(p[a]);
                }
                if (dyn_first < 0 && (bits & kValidDynamic)) dyn_first = k;
                if (validate_done(r, k, 1, first, dyn_first)) break;
            }
            out_status[b] = validate_status(first, dyn_first);
            out_first[b] = first;
            if (out_dyn_first) out_dyn_first[b] = dyn_first;
        }
        if (out_invalid && out_status[b] != 0) out_invalid[n_invalid++] = b;
    }
    if (out_n_invalid) *out_n_invalid = n_invalid;
    return VIGO_OK;
}
