// vigo_seed.hip — vigo_seed_paths: the seed-path stage between polyTrajOccMap and bsplineTraj (getTrajectory(dt), the
// inputPathCheck search with its dt *= 0.8 retries, updatePath's map-dependent head) for many trajectories, by the rules
// of vigo_seed_core.hpp.  One wavefront (= one workgroup) per trajectory.  Per try:
//   lanes    the trip count (uniform), then t_j from the clock's closed form and the sample into LDS
//   lanes    per consecutive pair: line flag, step length, distance from the first point — independent per pair
//   lane 0   rule 3 over those arrays (serial by definition, a few hundred steps)
//   lanes    rule 4 as a wave-wide any
// then lane 0 thins the adjusted prefix in place (rule 5), and rule 6 reuses the pair phase and lane 0's walk on the kept
// points.  No atomics: every output has one writer, the points leave LDS with coalesced vector stores.
// LDS: 3 (cap + 1) + 2 cap doubles and cap bytes (63 136 B with the fill points) at cap = kSeedCapacity = 1536, inside the 64 KiB a workgroup
// gets without asking; two one-wave workgroups fit a CU (very low occupancy: the walks and the per-sample clock are
// latency).  A try with more samples ends the trajectory as kSeedDeferred.
#include "vigo_grid.hpp"
#include "vigo_seed_core.hpp"

namespace vigo {
namespace {

struct SeedArgs {
    int T, S, deg;
    const int32_t* seg_off;
    const double* coeffs;
    const double* knots;
    const double *duration, *dt0, *cpd, *max_len, *prev_seed, *prev_fit;
    int max_tries, point_cap;
    int32_t *out_status, *out_tries;
    double *out_dt, *out_final_time;
    int32_t* out_seed_n;
    double* out_seed;
    int32_t* out_fit_n;
    double* out_fit;
    double *out_prev_seed, *out_prev_fit;
};

__global__ void __launch_bounds__(64) k_seed_paths(GridOcc occ, SeedArgs A) {
    __shared__ double s_pts[3 * (kSeedCapacity + 1)];
    __shared__ double s_step[kSeedCapacity], s_dist[kSeedCapacity];
    __shared__ uint8_t s_line[kSeedCapacity];
    __shared__ double s_fill[15];
    __shared__ double s_prev;
    __shared__ int s_count;
    const int t = blockIdx.x, lane = threadIdx.x;
    if (t >= A.T) return;
    const double res = occ.g.res;

    SeedIn in;
    SeedOut o;
    const int a = A.seg_off[t], b = A.seg_off[t + 1];
    const bool offsets_ok = a >= 0 && b >= a && b <= A.S;
    in.K = offsets_ok ? b - a : 0;
    in.deg = A.deg;
    in.knots = A.knots + (offsets_ok ? (size_t)a + t : 0);
    in.coeffs = A.coeffs + (offsets_ok ? (size_t)a * 3 * (A.deg + 1) : 0);
    in.duration = A.duration[t]; in.dt0 = A.dt0[t];
    in.control_point_distance = A.cpd[t]; in.max_path_length = A.max_len[t];
    in.prev_seed = A.prev_seed[t]; in.prev_fit = A.prev_fit[t];
    in.max_tries = A.max_tries; in.point_cap = A.point_cap;

    // every branch below is wave-uniform: the values it tests are the same in all lanes
    int status = -1;                                       // -1: still running
    if (!offsets_ok) {
        status = kSeedBadInput;
    } else {
        bool bad = !seed_finite(in.duration) || !seed_finite(in.dt0) || !(in.dt0 > 0.0);
        for (int i = lane; i <= in.K; i += 64) bad = bad || !seed_finite(in.knots[i]);
        if (__any(bad)) status = kSeedBadInput;
    }
    const SeedPowExact power;
    double dt = in.dt0, prev = in.prev_seed;
    int tries = 0, c = 0;
    bool found = false;
    while (status < 0 && tries < in.max_tries) {
        int64_t n64;
        const int st = seed_sample_count(in.duration, dt, kSeedCapacity, &n64);
        if (st != kSeedOk) { status = st; break; }
        const int n = (int)n64;
        ++tries;
        for (int j = lane; j < n; j += 64)
            seed_sample(in.K, in.knots, in.coeffs, in.deg, accumulated_time(dt, j), in.duration, power, s_pts + 3 * j);
        __syncthreads();
        for (int i = lane; i + 1 < n; i += 64) seed_pair(occ, res, s_pts, i, s_line + i, s_step + i, s_dist + i);
        __syncthreads();
        if (lane == 0) {
            double p;
            s_count = seed_adjust(n, prev, in.max_path_length, s_line, s_step, s_dist, &p);
            s_prev = p;
        }
        __syncthreads();
        c = s_count;
        prev = s_prev;
        bool far = false;
        for (int i = lane; i + 1 < c; i += 64) far = far || seed_too_far(i, c, s_step, in.control_point_distance);
        const bool any_far = __any(far);
        __syncthreads();                                    // (s_count / s_prev are read before the next try rewrites them)
        if (!any_far) { found = true; break; }
        dt = dt * 0.8;
    }
    o.tries = tries; o.dt = dt; o.prev_seed = prev; o.prev_fit = in.prev_fit;
    o.seed_n = 0; o.fit_n = 0; o.final_time = 0.0;
    bool from_fill = false;
    if (status < 0) {
        if (!found) {
            status = kSeedNoSpacing;
        } else if (c == 0) {
            status = kSeedTooShort;
        } else {
            if (lane == 0) s_count = seed_thin(s_pts, c, in.control_point_distance);
            __syncthreads();
            const int sn = s_count;
            __syncthreads();
            if (sn > in.point_cap) {
                status = kSeedDeferred;
            } else {
                o.final_time = (double)(c - 1) * dt;
                o.seed_n = sn;
                const double* goal = s_pts + 3 * (sn - 1);
                if (occ(goal[0], goal[1], goal[2])) {
                    status = kSeedGoalOccupied;
                } else {
                    for (int i = lane; i + 1 < sn; i += 64) seed_pair(occ, res, s_pts, i, s_line + i, s_step + i, s_dist + i);
                    __syncthreads();
                    if (lane == 0) {
                        double p;
                        s_count = seed_adjust(sn, in.prev_fit, in.max_path_length, s_line, s_step, s_dist, &p);
                        s_prev = p;
                        if (s_count < 4 && sn < 4) seed_fill(s_pts, sn, s_fill);
                    }
                    __syncthreads();
                    o.prev_fit = s_prev;
                    o.fit_n = seed_fit_count(sn, s_count, &from_fill);
                    status = o.fit_n > in.point_cap ? kSeedDeferred : kSeedOk;
                }
            }
        }
    }
    if (status == kSeedBadInput) seed_reset(in, status, &o);
    if (lane == 0) A.out_status[t] = status;
    if (status == kSeedDeferred) return;                   // the host runs it: nothing else is written
    if (lane == 0) {
        A.out_tries[t] = o.tries;
        A.out_dt[t] = o.dt;
        A.out_final_time[t] = o.final_time;
        A.out_seed_n[t] = o.seed_n;
        A.out_fit_n[t] = o.fit_n;
        A.out_prev_seed[t] = o.prev_seed;
        A.out_prev_fit[t] = o.prev_fit;
    }
    double* seed = A.out_seed + (size_t)t * A.point_cap * 3;
    double* fit = A.out_fit + (size_t)t * A.point_cap * 3;
    for (int i = lane; i < 3 * o.seed_n; i += 64) seed[i] = s_pts[i];
    const double* src = from_fill ? s_fill : s_pts;
    for (int i = lane; i < 3 * o.fit_n; i += 64) fit[i] = src[i];
}

}  // namespace

int launch_seed_paths(hipStream_t s, const GridView& g, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                      const double* knots, const double* duration, const double* dt0, const double* control_point_distance,
                      const double* max_path_length, const double* prev_in_seed, const double* prev_in_fit, int max_tries,
                      int point_cap, int32_t* out_status, int32_t* out_tries, double* out_dt, double* out_final_time,
                      int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit, double* out_prev_seed,
                      double* out_prev_fit) {
    if (T <= 0) return (int)hipSuccess;
    SeedArgs A;
    A.T = T; A.S = S; A.deg = deg;
    A.seg_off = seg_off; A.coeffs = coeffs; A.knots = knots;
    A.duration = duration; A.dt0 = dt0; A.cpd = control_point_distance; A.max_len = max_path_length;
    A.prev_seed = prev_in_seed; A.prev_fit = prev_in_fit;
    A.max_tries = max_tries; A.point_cap = point_cap;
    A.out_status = out_status; A.out_tries = out_tries; A.out_dt = out_dt; A.out_final_time = out_final_time;
    A.out_seed_n = out_seed_n; A.out_seed = out_seed; A.out_fit_n = out_fit_n; A.out_fit = out_fit;
    A.out_prev_seed = out_prev_seed; A.out_prev_fit = out_prev_fit;
    hipLaunchKernelGGL(k_seed_paths, dim3(T), dim3(64), 0, s, GridOcc{g}, A);
    return (int)hipGetLastError();
}

}  // namespace vigo
