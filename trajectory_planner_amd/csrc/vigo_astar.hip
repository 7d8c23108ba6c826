// vigo_astar.hip — vigo_astar_search: Q independent A* searches of the facade's host A* (host/src/astarOcc.cpp) on the
// handle's grid snapshot, each the search of vigo_astar_core.hpp bit for bit.
//
// One wavefront (one workgroup of 64) per search; node table and open set in LDS.  An expansion is
//   lane 0      pop (libstdc++'s pop_heap on the array heap), goal test, close            -> s_cur, s_gcur, s_status
//   lanes 0-26  astar_probe of neighbour `lane`: table probe, height band, the map bit (the one global-memory read of an
//               expansion), g through the expanded node                                   -> s_cand[lane]
//   lane 0      astar_commit: the candidates in the host's neighbour order — insert + push, or rewrite
// with a workgroup barrier between the steps (one wave: it costs a wait for the LDS writes).  Results leave with plain
// vector stores from lane 0; no atomics.
//
// Two table sizes: 2048 slots (1792 nodes, 30 KiB of LDS: five searches share a CU) for every search first, then 8192
// slots (7168 nodes, 112 KiB: a CU's LDS) for the ones whose table or heap overflowed — the second kernel picks them up
// from the status array, no host round trip.  The table holds the nodes that were PUSHED; a blocked neighbour (height
// band, map) is asked again when another expansion reaches it, which is a register test or a cached map word, while the
// host's count of reached nodes is 1.5 times its count of pushed ones on the pipeline workload (profiles/README.md).
// Workgroups take the searches round-robin, so a launch runs as many at a time as the device has room for.
#include "vigo_astar_core.hpp"
#include "vigo_grid.hpp"

namespace vigo {
namespace {

constexpr int kAstarRetry = 4;   // (between the two kernels) the small table overflowed

struct AstarArgs {
    int Q;
    const double* start;
    const double* end;
    double step, min_h, max_h;
    int pool[3];
    int max_expansions, path_cap;
    int32_t* status;
    int32_t* len;
    double* path;
    int32_t* stats;
    int pass;          // 0: every search, overflow -> kAstarRetry; 1: the kAstarRetry ones, overflow -> kAstarDeferred
};

template <int CAP_LOG2, int HEAP_CAP>
constexpr size_t astar_lds_bytes() { return ((size_t)1 << CAP_LOG2) * (8 + 4 + 1) + (size_t)HEAP_CAP * 2; }

template <int CAP_LOG2, int HEAP_CAP>
__global__ void __launch_bounds__(64) k_astar(GridOcc occ, AstarArgs A) {
    constexpr int CAP = 1 << CAP_LOG2;
    extern __shared__ __align__(16) unsigned char s_lds[];
    __shared__ AstarCand s_cand[27];
    __shared__ double s_gcur;
    __shared__ int s_cur, s_status;
    const int lane = threadIdx.x;
    AstarStore<uint16_t> S;
    S.g = reinterpret_cast<double*>(s_lds);
    S.key = reinterpret_cast<int32_t*>(S.g + CAP);
    S.heap = reinterpret_cast<uint16_t*>(S.key + CAP);
    S.meta = reinterpret_cast<uint8_t*>(S.heap + HEAP_CAP);
    S.cap_log2 = CAP_LOG2;
    S.max_nodes = CAP - CAP / 8;
    S.heap_cap = HEAP_CAP;
    S.n_nodes = S.n_heap = S.heap_peak = S.pops = S.rewrites = 0;
    S.goal[0] = S.goal[1] = S.goal[2] = 0;
    for (int q = blockIdx.x; q < A.Q; q += gridDim.x) {
        if (A.pass == 1 && A.status[q] != kAstarRetry) continue;      // (the workgroup's: one value for all lanes)
        for (int i = lane; i < CAP; i += 64) S.key[i] = -1;
        double s[3], e[3];
        for (int a = 0; a < 3; ++a) { s[a] = A.start[(size_t)q * 3 + a]; e[a] = A.end[(size_t)q * 3 + a]; }
        AstarGeom G;
        astar_geom(G, s, e, A.step, A.pool, A.min_h, A.max_h);
        __syncthreads();
        int goal_slot = 0;
        if (lane == 0) {
            int si[3], ei[3];
            S.n_nodes = S.n_heap = S.heap_peak = S.pops = S.rewrites = 0;
            if (astar_adjust_ends(G, occ, s, e, si, ei)) {
                astar_begin(S, si, ei);
                s_status = kAstarRunning;
            } else {
                s_status = kAstarNotFound;
            }
        }
        for (;;) {
            if (lane == 0 && s_status == kAstarRunning) {
                int cur = 0, slot = 0;
                double g_cur = 0.0;
                s_status = astar_next(S, A.max_expansions, &cur, &g_cur, &slot);
                s_cur = cur;
                s_gcur = g_cur;
                goal_slot = slot;
            }
            __syncthreads();
            if (s_status != kAstarRunning) break;
            if (lane < 27) astar_probe(S, G, occ, s_cur, s_gcur, lane, s_cand[lane]);
            __syncthreads();
            if (lane == 0 && !astar_commit(S, s_cand)) s_status = A.pass == 0 ? kAstarRetry : kAstarDeferred;
        }
        if (lane == 0) {
            int st = s_status, len = 0;
            if (st == kAstarFound) {
                len = astar_path(S, G, goal_slot, A.path_cap, A.path + (size_t)q * A.path_cap * 3);
                if (len > A.path_cap) st = kAstarPathTooLong;
            }
            A.status[q] = st;
            A.len[q] = len;
            if (A.stats) {
                A.stats[(size_t)q * 3] = S.pops;
                A.stats[(size_t)q * 3 + 1] = S.n_nodes;
                A.stats[(size_t)q * 3 + 2] = S.heap_peak;
            }
        }
        __syncthreads();                                              // (s_status is rewritten for the next search)
    }
}

}  // namespace

int astar_max_nodes() { return 8192 - 8192 / 8; }
int astar_max_heap() { return 4096; }

int launch_astar(hipStream_t s, const GridView& g, int Q, const double* start, const double* end, double step, const int32_t pool[3],
                 double min_h, double max_h, int max_expansions, int path_cap, int32_t* out_status, int32_t* out_len, double* out_path,
                 int32_t* out_stats, LaunchState& L) {
    if (Q <= 0) return hipSuccess;
    constexpr size_t small = astar_lds_bytes<11, 2048>(), large = astar_lds_bytes<13, 4096>();
    if (!L.astar_attr_set) {     // per handle = per device (LaunchState)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_astar<13, 4096>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)large);
        if (e != hipSuccess) return (int)e;
        L.astar_attr_set = true;
    }
    const int cus = L.simd_count > 0 ? L.simd_count / 4 : 256;
    AstarArgs a{Q, start, end, step, min_h, max_h, {pool[0], pool[1], pool[2]}, max_expansions, path_cap, out_status, out_len, out_path, out_stats, 0};
    const GridOcc occ{g};
    hipLaunchKernelGGL((k_astar<11, 2048>), dim3(Q < 5 * cus ? Q : 5 * cus), dim3(64), small, s, occ, a);
    a.pass = 1;
    hipLaunchKernelGGL((k_astar<13, 4096>), dim3(Q < cus ? Q : cus), dim3(64), large, s, occ, a);
    return (int)hipGetLastError();
}

}  // namespace vigo
