// vigo_pathsearch.hip — vigo_collision_segs and vigo_path_search: steps 1 and 2 of bsplineTraj's prologue
// (findCollisionSeg, host/src/bsplineTraj.cpp:409; pathSearch + applyMerges, :439-493) for B trajectories, the rules of
// vigo_pathsearch_core.hpp around the searches of vigo_astar.hip (launch_astar, unchanged).  The output is the
// seg_off / seg / path_off / path input of vigo_guide_assign.
//
// The kernels of one vigo_path_search call, in stream order (vigo_api.cpp reads back the words marked <-):
//   k_ctrl_occupancy (vigo_map.hip)   point and line flags of every control point           (seg == NULL only)
//   k_ps_count   one workgroup        segments per trajectory (the scan, or the checks of a supplied list), their
//                                     exclusive scan                                          <- searches, bad list
//   k_ps_fill    a thread per traj.   the segments, and the ends of every first-choice search
//   k_astar x 2                       the first-choice searches
//   k_ps_retry   one workgroup        the second-choice searches the failures ask for (retry_list), scanned; their ends
//                                                                                             <- searches
//   k_astar x 2                       those searches
//   k_ps_decide  one workgroup        path_walk per trajectory: status, segments after the merges, which search is which
//                                     path; segments and path points scanned               <- segments, points
//   k_ps_write   a wave per traj.     nothing is written before this one: statuses, offsets, segments, and the searches'
//                                     fixed-stride paths compacted into the CSR output (point 0 replaced by ctrl[first],
//                                     the end control point appended), a point per lane
// The serial parts (a scan over a few dozen flags, a walk over a handful of segments) run one trajectory per thread; the
// one-workgroup kernels are k_guide_offsets' shape (vigo_scan.hpp: a slice of the batch per thread, a 1024-thread scan).
// Plain vector stores, no atomics.
#include "vigo_pathsearch_core.hpp"
#include "vigo_rows_core.hpp"
#include "vigo_internal.hpp"
#include "vigo_scan.hpp"

namespace vigo {
namespace {

// the supplied list of trajectory b: CSR (seg_off_in), or seg_cnt_in[b] segments at a fixed stride (vigo_reguide.hip)
__device__ __forceinline__ int ps_list_first(const PathSearchArgs& A, int b) { return A.seg_cnt_in ? b * A.seg_stride_in : A.seg_off_in[b]; }
__device__ __forceinline__ int ps_list_end(const PathSearchArgs& A, int b) {
    return A.seg_cnt_in ? b * A.seg_stride_in + A.seg_cnt_in[b] : A.seg_off_in[b + 1];
}

__global__ void __launch_bounds__(1024) k_ps_count(PathSearchArgs A) {
    __shared__ long long s_cnt[1024];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const auto [lo, hi] = batch_slice(A.B);
    long long n = 0;
    bool bad = false;
    for (int b = lo; b < hi && !bad; ++b) {
        // (the _mixed entries) the trajectory's own count in a row of A.N; a bad count defers it: no segment, no search
        const int N = row_count(A.n_pts, b, A.N);
        int nb = 0;
        if (A.seg_in) {
            const int s0 = ps_list_first(A, b), s1 = ps_list_end(A, b);
            if (s0 < 0 || s1 < s0) { bad = true; break; }
            nb = s1 - s0;
            if (nb <= kPathsMaxSegs && N > 0)
                for (int k = s0; k < s1; ++k) {
                    const int f = A.seg_in[2 * k], e = A.seg_in[2 * k + 1];
                    if (f < 0 || f >= N || e < 0 || e >= N) { bad = true; break; }
                }
        } else if (N > 0) {
            nb = collision_segs(N, A.not_check_ratio, FlagOcc{A.pt + (size_t)b * A.N}, FlagOcc{A.ln + (size_t)b * A.N}, 0, nullptr);
        }
        const bool over = nb > kPathsMaxSegs || N < 0;
        A.pre[b] = over ? 1 : 0;
        A.n_in[b] = over ? 0 : nb;
        n += over ? 0 : nb;
    }
    if (bad) s_bad = 1;
    long long total;
    long long at = scan1024(s_cnt, n, &total) - n;
    for (int b = lo; b < hi && !bad; ++b) {
        A.in_off[b] = (int32_t)at;
        at += A.n_in[b];
    }
    if (tid == 1023) A.in_off[A.B] = (int32_t)total;
    if (tid == 0) {
        A.result[0] = total;
        A.result[1] = s_bad;
    }
}

// dst_seg: where the trajectories' segments go (at in_off); start / end: the first-choice ends, or NULL
__global__ void __launch_bounds__(256) k_ps_fill(PathSearchArgs A, int32_t* dst_seg, double* start, double* end) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= A.B) return;
    const int q0 = A.in_off[b], n = A.n_in[b];
    int32_t* seg = dst_seg + 2 * (size_t)q0;
    if (A.seg_in) {
        const int32_t* src = A.seg_in + 2 * (size_t)ps_list_first(A, b);
        for (int k = 0; k < 2 * n; ++k) seg[k] = src[k];
    } else if (n > 0) {                                   // (a bad count has none: k_ps_count)
        collision_segs(row_count(A.n_pts, b, A.N), A.not_check_ratio, FlagOcc{A.pt + (size_t)b * A.N}, FlagOcc{A.ln + (size_t)b * A.N}, n, seg);
    }
    if (!start) return;
    const double* c = A.ctrl + (size_t)b * A.N * 3;
    for (int k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) {
            start[(size_t)(q0 + k) * 3 + a] = c[3 * (size_t)seg[2 * k] + a];
            end[(size_t)(q0 + k) * 3 + a] = c[3 * (size_t)seg[2 * k + 1] + a];
        }
}

// vigo_collision_segs' outputs once the segments fit
__global__ void __launch_bounds__(256) k_ps_segs_out(PathSearchArgs A) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > A.B) return;
    A.out_seg_off[b] = A.in_off[b];
    if (b < A.B) A.out_status[b] = A.pre[b] ? kPathsDeferred : kPathsOk;
}

__global__ void __launch_bounds__(1024) k_ps_retry(PathSearchArgs A, PathSearchWork W) {
    __shared__ long long s_cnt[1024];
    const int tid = threadIdx.x;
    const auto [lo, hi] = batch_slice(A.B);
    long long n = 0;
    for (int b = lo; b < hi; ++b) {
        const int q0 = A.in_off[b];
        const int32_t* st = W.status1 + q0;
        for (int k = 0; k < A.n_in[b]; ++k) W.retry_of[q0 + k] = -1;
        n += retry_list(A.n_in[b], W.seg + 2 * (size_t)q0, [st](int k) { return st[k]; }, [](int) {});
    }
    long long total;
    long long at = scan1024(s_cnt, n, &total) - n;
    for (int b = lo; b < hi; ++b) {
        const int q0 = A.in_off[b];
        const int32_t* st = W.status1 + q0;
        const int32_t* seg = W.seg + 2 * (size_t)q0;
        const double* c = A.ctrl + (size_t)b * A.N * 3;
        retry_list(A.n_in[b], seg, [st](int k) { return st[k]; }, [&](int k) {
            const size_t r = (size_t)at++;
            W.retry_of[q0 + k] = (int32_t)r;
            for (int a = 0; a < 3; ++a) {
                W.start2[r * 3 + a] = W.start1[(size_t)(q0 + k) * 3 + a];
                W.end2[r * 3 + a] = c[3 * (size_t)seg[2 * (k + 1) + 1] + a];
            }
        });
    }
    if (tid == 0) A.result[2] = total;
}

__global__ void __launch_bounds__(1024) k_ps_decide(PathSearchArgs A, PathSearchWork W) {
    __shared__ long long s_cnt[1024];
    const int tid = threadIdx.x;
    const auto [lo, hi] = batch_slice(A.B);
    long long n_seg = 0, n_pts = 0;
    for (int b = lo; b < hi; ++b) {
        const int q0 = A.in_off[b], n = A.n_in[b];
        int status = kPathsDeferred, n_out = 0, run = 0, decided = 0;
        long long pts = 0;
        if (!A.pre[b]) {
            const int32_t* st1 = W.status1 + q0;
            const int32_t* ro = W.retry_of + q0;
            const int32_t* st2 = W.status2;
            auto second = [ro, st2](int k) { return ro[k] >= 0 ? st2[ro[k]] : 2; };
            status = path_walk(n, W.seg + 2 * (size_t)q0, [st1](int k) { return st1[k]; }, second, W.mseg + 2 * (size_t)q0, W.pick + q0, &n_out);
            for (int j = 0; j < n_out; ++j) {
                const int k = W.pick[q0 + j] & ~kPathsSecond;
                pts += ((W.pick[q0 + j] & kPathsSecond) ? W.len2[ro[k]] : W.len1[q0 + k]) + 1;
            }
            for (int k = 0; k < n; ++k) {
                ++run;
                decided += paths_search_decided(st1[k]) ? 1 : 0;
                if (ro[k] >= 0) {
                    ++run;
                    decided += paths_search_decided(st2[ro[k]]) ? 1 : 0;
                }
            }
        }
        A.tstatus[b] = status;
        A.n_out[b] = n_out;
        A.tcounts[2 * b] = run;
        A.tcounts[2 * b + 1] = decided;
        A.opt_off[b] = (int32_t)(pts > 0x7fffffffLL ? 0x7fffffffLL : pts);      // (for now: this trajectory's points)
        n_seg += n_out;
        n_pts += pts;
    }
    long long total_seg, total_pts;
    long long at_seg = scan1024(s_cnt, n_seg, &total_seg) - n_seg;
    long long at_pts = scan1024(s_cnt, n_pts, &total_pts) - n_pts;
    const bool fits = total_pts <= 0x7fffffffLL;
    for (int b = lo; b < hi && fits; ++b) {
        const long long pts = A.opt_off[b];
        A.oseg_off[b] = (int32_t)at_seg;
        A.opt_off[b] = (int32_t)at_pts;
        at_seg += A.n_out[b];
        at_pts += pts;
    }
    if (tid == 0) {
        A.result[3] = total_seg;
        A.result[4] = total_pts;
    }
}

__global__ void __launch_bounds__(64) k_ps_write(PathSearchArgs A, PathSearchWork W, int total_seg, int total_pts) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const int q0 = A.in_off[b], n_out = A.n_out[b], s0 = A.oseg_off[b];
    if (lane == 0) {
        A.out_status[b] = A.tstatus[b];
        A.out_seg_off[b] = s0;
        if (A.out_counts) {
            A.out_counts[2 * b] = A.tcounts[2 * b];
            A.out_counts[2 * b + 1] = A.tcounts[2 * b + 1];
        }
        if (b == 0) {
            A.out_seg_off[A.B] = total_seg;
            A.out_path_off[total_seg] = total_pts;
        }
    }
    const double* c = A.ctrl + (size_t)b * A.N * 3;
    const int32_t* seg = W.seg + 2 * (size_t)q0;
    int at = A.opt_off[b];
    for (int j = 0; j < n_out; ++j) {                     // (n_out, the picks and the lengths: one value for all lanes)
        const int pick = W.pick[q0 + j];
        const int k = pick & ~kPathsSecond;
        const bool second = (pick & kPathsSecond) != 0;
        const int r = second ? W.retry_of[q0 + k] : q0 + k;
        const int len = second ? W.len2[r] : W.len1[r];   // 1 .. search_path_cap points of the search
        const double* src = (second ? W.path2 : W.path1) + (size_t)r * A.search_path_cap * 3;
        const double* first = c + 3 * (size_t)seg[2 * k];
        const double* last = c + 3 * (size_t)seg[2 * (second ? k + 1 : k) + 1];
        if (lane == 0) {
            A.out_seg[2 * (size_t)(s0 + j)] = W.mseg[2 * (size_t)(q0 + j)];
            A.out_seg[2 * (size_t)(s0 + j) + 1] = W.mseg[2 * (size_t)(q0 + j) + 1];
            A.out_path_off[s0 + j] = at;
        }
        for (int i = lane; i <= len; i += 64) {
            const double* p = i == 0 ? first : i == len ? last : src + 3 * (size_t)i;
            double* o = A.out_path + 3 * (size_t)(at + i);
            o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        }
        at += len + 1;
    }
}

}  // namespace

int launch_ps_count(hipStream_t s, const PathSearchArgs& a) {
    hipLaunchKernelGGL(k_ps_count, dim3(1), dim3(1024), 0, s, a);
    return (int)hipGetLastError();
}

int launch_ps_fill(hipStream_t s, const PathSearchArgs& a, int32_t* dst_seg, double* start, double* end) {
    hipLaunchKernelGGL(k_ps_fill, dim3((a.B + 255) / 256), dim3(256), 0, s, a, dst_seg, start, end);
    return (int)hipGetLastError();
}

int launch_ps_segs_out(hipStream_t s, const PathSearchArgs& a) {
    hipLaunchKernelGGL(k_ps_segs_out, dim3((a.B + 1 + 255) / 256), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int launch_ps_retry(hipStream_t s, const PathSearchArgs& a, const PathSearchWork& w) {
    hipLaunchKernelGGL(k_ps_retry, dim3(1), dim3(1024), 0, s, a, w);
    return (int)hipGetLastError();
}

int launch_ps_decide(hipStream_t s, const PathSearchArgs& a, const PathSearchWork& w) {
    hipLaunchKernelGGL(k_ps_decide, dim3(1), dim3(1024), 0, s, a, w);
    return (int)hipGetLastError();
}

int launch_ps_write(hipStream_t s, const PathSearchArgs& a, const PathSearchWork& w, int total_seg, int total_pts) {
    hipLaunchKernelGGL(k_ps_write, dim3(a.B), dim3(64), 0, s, a, w, total_seg, total_pts);
    return (int)hipGetLastError();
}

}  // namespace vigo
