// vigo_api.cpp — the C ABI of libvigo_hip.so (include/vigo.h): handle management, argument
// checks and kernel launches.  No computation happens on the host: if HIP is unusable every
// entry point fails loudly (VIGO_ERR_NO_DEVICE / VIGO_ERR_HIP) instead of falling back.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "vigo_esdf_core.hpp"
#include "vigo_exact_pow.hpp"
#include "vigo_exact_time.hpp"
#include "vigo_fit_plan.hpp"
#include "vigo_grid_update_core.hpp"
#include "vigo_handle.hpp"
#include "vigo_seed_core.hpp"
#include "vigo_solver_plan.hpp"
#include "vigo_traj_runs.hpp"
#include "vigo_validate_core.hpp"
#include "vigo_ws_layout.hpp"

#include "../../include/vigo_validate.h"

using vigo::DevBuffer;
using vigo::DevConst;
using vigo::GridView;
using vigo::SolveArgs;

namespace {

int fail(vigo_handle_t h, int code, const char* what, hipError_t e = hipSuccess) {
    if (h) {
        h->last_error = what;
        if (e != hipSuccess) {
            h->last_error += ": ";
            h->last_error += hipGetErrorString(e);
        }
    }
    return code;
}

// (the launchers report hipGetLastError(): whatever another library of the process — torch, RCCL — left
// in the thread's last-error slot is discarded first, so it is not mistaken for a failed launch of ours)
#define VIGO_HIP(h, call)                                                      \
    do {                                                                       \
        (void)hipGetLastError();                                               \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) return fail((h), VIGO_ERR_HIP, #call, e_);       \
    } while (0)
#define VIGO_TRY(call)                                                         \
    do {                                                                       \
        const int rc_ = (call);                                                \
        if (rc_ != VIGO_OK) return rc_;                                        \
    } while (0)

// Buffer `id` of the handle holds at least `need` bytes afterwards; when it has to grow, to `alloc` bytes (contents are
// not kept).  A failed allocation leaves it empty.  Callers whose cache lives in the buffer invalidate it first.
int reserve(vigo_handle_t h, vigo::BufId id, size_t need, size_t alloc) {
    static const char* const what[] = {
        "hipMalloc(grid)", "hipMalloc(esdf)", "hipMalloc(esdf_ws)", "hipMalloc(esdf_track)", "hipMalloc(fit)", "hipMalloc(fit_table)", "hipMalloc(times)", "hipMalloc(finish_ts)", "hipMalloc(finish_dt)", "hipMalloc(validate_clock)", "hipMalloc(validate_tab)", "hipMalloc(scratch)",
        "hipMalloc(paths_ws[0])", "hipMalloc(paths_ws[1])", "hipMalloc(reguide_ws[0])", "hipMalloc(reguide_ws[1])",
        "hipMalloc(reguide_ws[2])", "hipMalloc(rebound)"};
    static_assert(sizeof(what) / sizeof(what[0]) == vigo::kBufCount, "one name per BufId, in its order");
    DevBuffer& b = h->buf[id];
    if (need <= b.bytes) return VIGO_OK;
    if (b.ptr) (void)hipFree(b.ptr);
    b = DevBuffer{};
    (void)hipGetLastError();
    const hipError_t e = hipMalloc(&b.ptr, alloc);
    if (e != hipSuccess) {
        b.ptr = nullptr;
        return fail(h, VIGO_ERR_HIP, what[id], e);
    }
    b.bytes = alloc;
    return VIGO_OK;
}
// the per-call workspaces are reused at nearby sizes: a quarter of slack keeps a slowly growing batch from reallocating
int reserve_slack(vigo_handle_t h, vigo::BufId id, size_t need) { return reserve(h, id, need, need + need / 4 + 4096); }
int ensure_scratch(vigo_handle_t h, size_t bytes) { return reserve_slack(h, vigo::kBufScratch, bytes); }
// a workspace laid out by `layout` (vigo_ws_layout.hpp) in buffer `id`: measured on a null base, reserved, carved
enum Growth { kExact, kSlack };
template <class Layout>
int carve(vigo_handle_t h, vigo::BufId id, Growth g, Layout layout) {
    const size_t need = layout(nullptr);
    const int rc = g == kSlack ? reserve_slack(h, id, need) : reserve(h, id, need, need);
    if (rc == VIGO_OK) layout(h->buf[id].ptr);
    return rc;
}

// a few result words back on the host: the copy and the wait for it
int read_back(vigo_handle_t h, void* dst, const void* src, size_t bytes) {
    VIGO_HIP(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    VIGO_HIP(h, hipStreamSynchronize(h->stream));
    return VIGO_OK;
}

int check_solve_args(vigo_handle_t h, int B, int N, const void* ctrl) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && !ctrl)) return fail(h, VIGO_ERR_INVALID_ARG, "B < 0 or ctrl == NULL");
    if (N < 7 || N > VIGO_MAX_CTRL_POINTS) return fail(h, VIGO_ERR_UNSUPPORTED_N, "N outside [7, VIGO_MAX_CTRL_POINTS]");
    return VIGO_OK;
}

// the mixed-count entries: rows of Ns control points, one launch of the general kernel up to Ns = 64
int check_mixed_args(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const void* ctrl) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!ctrl || !n_pts))) return fail(h, VIGO_ERR_INVALID_ARG, "B < 0, ctrl == NULL or n_pts == NULL");
    if (Ns < 7 || Ns > vigo::kMixedMaxStride) return fail(h, VIGO_ERR_UNSUPPORTED_N, "Ns outside [7, 64]: group such trajectories by their exact count");
    return VIGO_OK;
}

// The list arguments shared by the solve entry points and the dynamic gate.  Offsets (or a shared count)
// without the list they index mean "no guides" / "no obstacles" — callers keep all-zero CSR offsets around
// when a batch happens to have none — and the kernels never dereference the missing list.
int check_list_args(vigo_handle_t h, int n_obs_shared) {
    if (n_obs_shared < 0) return fail(h, VIGO_ERR_INVALID_ARG, "n_obs_shared < 0");
    return VIGO_OK;
}

// the common fields of the solve entry points' SolveArgs
SolveArgs solve_args(int B, int N, double* ctrl, const int32_t* guide_off, const double* guide_pv, const uint8_t* guide_unk,
                     const int32_t* obs_off, const double* obs, int n_obs_shared, const double* weights) {
    SolveArgs a{};
    a.B = B; a.N = N;
    a.ctrl = ctrl;
    a.guide_off = guide_off; a.guide_pv = guide_pv; a.guide_unk = guide_unk;
    a.obs_off = obs_off; a.obs = obs; a.n_obs_shared = n_obs_shared;
    a.weights = weights;
    return a;
}
vigo::MixedSolveArgs mixed_args(const SolveArgs& a, const int32_t* n_pts) {
    vigo::MixedSolveArgs m{};
    static_cast<SolveArgs&>(m) = a;
    m.n_pts = n_pts;
    return m;
}

// the L-BFGS history of a solve workgroup fits the LDS of a CU
bool lds_fits(vigo_handle_t h, int N) { return vigo::optimize_lds_requirement(N, h->params.mem_size, h->precision) <= vigo::kLdsPerWorkgroup; }
const char* const kLdsMsg = "the L-BFGS history of N control points x mem_size does not fit the 160 KiB LDS of a CU";

// the control points a spline gate evaluates (the solver's own range starts at 7: check_solve_args)
bool gate_N_ok(int N) { return N >= 4 && N <= VIGO_MAX_CTRL_POINTS; }
const char* const kGateNMsg = "N outside [4, VIGO_MAX_CTRL_POINTS]";

// Sample times of `for (t = 0; t <= tmax; t += dt)` (BT.h:313, :347): t_k is the k-fold floating point
// accumulation, reproduced exactly by vigo::accumulated_time (closed form per binade).  The sample count T is
// found on the host by bisection over that closed form (monotone in k), the table is filled by a device kernel
// and cached in the handle per (dt, tmax): the gates run without a host round trip.  -1: more than 2^24 samples.
// (vigo_exact_time.hpp has the function: the host twin of vigo_validate_core.hpp counts with the same copy)
using vigo::count_sample_times;

int upload_sample_times(vigo_handle_t h, double tmax, double dt, int* out_T, const double** out_dev) {
    if (!(dt > 0.0)) return fail(h, VIGO_ERR_INVALID_ARG, "dt must be > 0");
    if (h->times_T >= 0 && h->times_dt == dt && h->times_tmax == tmax) {
        if (h->times_stream != h->stream) {            // filled on another stream: make sure it has landed
            VIGO_HIP(h, hipStreamSynchronize(h->times_stream));
            h->times_stream = h->stream;
        }
        *out_T = h->times_T;
        *out_dev = h->buf[vigo::kBufTimes].as<double>();
        return VIGO_OK;
    }
    const int T = count_sample_times(dt, tmax);
    if (T < 0) return fail(h, VIGO_ERR_INVALID_ARG, "too many samples");
    h->times_T = -1;                                   // no clock cached while the buffer is regrown or refilled
    VIGO_TRY(reserve(h, vigo::kBufTimes, (size_t)T * sizeof(double), ((size_t)T + 64) * sizeof(double)));
    double* times = h->buf[vigo::kBufTimes].as<double>();
    VIGO_HIP(h, (hipError_t)vigo::launch_fill_sample_times(h->stream, dt, T, times));
    h->times_dt = dt;
    h->times_tmax = tmax;
    h->times_T = T;
    h->times_stream = h->stream;
    *out_T = T;
    *out_dev = times;
    return VIGO_OK;
}

// The strict sibling: samples of `for (t = 0; t < tmax; t += dt)` (BT.cpp:1122).  -1: more than 2^24.
int count_sample_times_strict(double dt, double tmax) {
    if (!(tmax > 0.0)) return 0;
    const int64_t cap = (int64_t)1 << 24;
    if (vigo::accumulated_time(dt, cap) < tmax) return -1;
    int64_t lo = 0, hi = cap;                       // t_lo < tmax <= t_hi
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (vigo::accumulated_time(dt, mid) < tmax) lo = mid; else hi = mid;
    }
    return (int)hi;                                 // samples k = 0 .. lo
}

// vigo_traj_finish's clocks, cached per (dt, tmax) like the gates' but in slots of their own (which: 0 the strict `<`
// clock of ts in kBufFinishTs, 1 the `<=` clock of the sample step in kBufFinishDt): a plan batch between two gate
// calls does not evict the gates' table, nor the other way round
int upload_clock_slot(vigo_handle_t h, vigo_context::ClockSlot& c, vigo::BufId id, bool strict, double tmax, double dt, int* out_T,
                      const double** out_dev);
int upload_finish_clock(vigo_handle_t h, int which, double tmax, double dt, int* out_T, const double** out_dev) {
    return upload_clock_slot(h, h->finish_clock[which], which == 0 ? vigo::kBufFinishTs : vigo::kBufFinishDt, which == 0, tmax, dt, out_T, out_dev);
}
// (vigo_traj_validate's clock is the third such slot: the `<=` clock of its dt in kBufValidateClock)
int upload_clock_slot(vigo_handle_t h, vigo_context::ClockSlot& c, vigo::BufId id, bool strict, double tmax, double dt, int* out_T,
                      const double** out_dev) {
    if (c.T >= 0 && c.dt == dt && c.tmax == tmax) {
        if (c.stream != h->stream) {                   // filled on another stream: make sure it has landed
            VIGO_HIP(h, hipStreamSynchronize(c.stream));
            c.stream = h->stream;
        }
        *out_T = c.T;
        *out_dev = h->buf[id].as<double>();
        return VIGO_OK;
    }
    const int T = strict ? count_sample_times_strict(dt, tmax) : count_sample_times(dt, tmax);
    if (T < 0) return fail(h, VIGO_ERR_INVALID_ARG, "too many samples");
    c.T = -1;                                          // no clock cached while the buffer is regrown or refilled
    VIGO_TRY(reserve(h, id, (size_t)T * sizeof(double), ((size_t)T + 64) * sizeof(double)));
    double* times = h->buf[id].as<double>();
    VIGO_HIP(h, (hipError_t)vigo::launch_fill_sample_times(h->stream, dt, T, times));
    c.dt = dt;
    c.tmax = tmax;
    c.T = T;
    c.stream = h->stream;
    *out_T = T;
    *out_dev = times;
    return VIGO_OK;
}

// vigo_traj_validate's {S, C} of every count 4 .. Ns (validate_counts), cached per (dt, ts_ctrl, ratio, rule, Ns) in one of
// kValidateSlots device tables.  A new key is computed into the pinned stage of the next slot in turn and copied in
// stream order; the host waits only if that slot's previous copy, kValidateSlots keys ago, has not left the stage yet.
int upload_validate_tab(vigo_handle_t h, double dt, double ratio, int rule, int Ns, const int32_t** out_dev) {
    const size_t per = (size_t)vigo::validate_tab_entries(VIGO_MAX_CTRL_POINTS);
    const double ts_ctrl = h->params.ts_ctrl;
    VIGO_TRY(reserve(h, vigo::kBufValidateTab, vigo_context::kValidateSlots * per * sizeof(int32_t), vigo_context::kValidateSlots * per * sizeof(int32_t)));
    int32_t* dev = h->buf[vigo::kBufValidateTab].as<int32_t>();
    for (int i = 0; i < vigo_context::kValidateSlots; ++i) {
        const vigo_context::ValidateKey& k = h->validate_key[i];
        if (k.Ns == Ns && k.rule == rule && k.dt == dt && k.ts_ctrl == ts_ctrl && k.ratio == ratio) {
            *out_dev = dev + i * per;
            return VIGO_OK;
        }
    }
    if (!h->validate_stage) {
        for (int i = 0; i < vigo_context::kValidateSlots; ++i)
            if (!h->validate_event[i]) VIGO_HIP(h, hipEventCreateWithFlags(&h->validate_event[i], hipEventDisableTiming));
        VIGO_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&h->validate_stage), vigo_context::kValidateSlots * per * sizeof(int32_t)));
    }
    const int slot = h->validate_next;
    // (the longest count first: it has the most samples, and a refusal must leave the slot's key alone)
    int32_t probe[2];
    if (!vigo::validate_counts(dt, ts_ctrl, ratio, rule, Ns, &probe[0], &probe[1])) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_validate: too many samples");
    VIGO_HIP(h, hipEventSynchronize(h->validate_event[slot]));
    h->validate_key[slot].Ns = 0;                      // no table cached while the slot is refilled
    int32_t* tab = h->validate_stage + slot * per;
    for (int n = vigo::kValidateMinN; n <= Ns; ++n)
        (void)vigo::validate_counts(dt, ts_ctrl, ratio, rule, n, &tab[2 * (n - vigo::kValidateMinN)], &tab[2 * (n - vigo::kValidateMinN) + 1]);
    VIGO_HIP(h, hipMemcpyAsync(dev + slot * per, tab, (size_t)vigo::validate_tab_entries(Ns) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    VIGO_HIP(h, hipEventRecord(h->validate_event[slot], h->stream));
    h->validate_key[slot] = vigo_context::ValidateKey{dt, ts_ctrl, ratio, rule, Ns};
    h->validate_next = (slot + 1) % vigo_context::kValidateSlots;
    *out_dev = dev + slot * per;
    return VIGO_OK;
}

// The box sweep visits (box / map_res + 1) lattice points per axis for every pose: a finite box and a bounded
// lattice, or the sweep is an unbounded device loop (the cfg box is 0.4 x 0.4 x 0.2 at 0.2: 3 x 3 x 2 points).
// Negative extents are the reference's "no lattice point at all" and stay allowed.
bool sweep_box_ok(const double box[3], double map_res) {
    double pts = 1.0;
    for (int a = 0; a < 3; ++a) {
        if (!(fabs(box[a]) < 1e9)) return false;
        const double n = box[a] > 0 ? floor(box[a] / map_res) + 1.0 : 1.0;
        if (!(n <= 256.0)) return false;
        pts *= n;
    }
    return pts <= 32768.0;
}

// a finite origin and a finite positive resolution (the key offsets below are integer conversions of origin / res)
bool geometry_ok(const double origin[3], double res) {
    if (!(res > 0.0) || !(res < 1e12)) return false;
    for (int a = 0; a < 3; ++a)
        if (!(fabs(origin[a]) < 1e12) || !(fabs(origin[a] / res) < 2e9)) return false;
    return true;
}

void fill_grid_view(vigo_handle_t h, int nx, int ny, int nz, const double origin[3], double res) {
    GridView& g = h->grid;
    g.planes = h->buf[vigo::kBufGrid].as<uint32_t>();
    g.nx = nx; g.ny = ny; g.nz = nz;
    g.nzw = (nz + 31) / 32;
    g.plane_words = (size_t)nx * ny * g.nzw;
    g.res = res;
    for (int a = 0; a < 3; ++a) {
        g.origin[a] = origin[a];
        g.bmin[a] = origin[a];
        g.key0[a] = (int)floor(origin[a] / res + 0.5);
    }
    g.bmax[0] = origin[0] + nx * res;
    g.bmax[1] = origin[1] + ny * res;
    g.bmax[2] = origin[2] + nz * res;
    h->has_grid = true;
}

int ensure_grid_storage(vigo_handle_t h, int nx, int ny, int nz) {
    const size_t need = vigo_grid_packed_bytes(nx, ny, nz);
    return reserve(h, vigo::kBufGrid, need, need);
}

// the corridor checker's lattice is octomap's: keys are whole multiples of res from the origin
bool key_lattice_ok(const GridView& g) {
    for (int a = 0; a < 3; ++a) {
        double q = g.origin[a] / g.res;
        if (fabs(q - floor(q + 0.5)) > 1e-6) return false;
    }
    return true;
}
const char* const kKeyLatticeMsg = "corridor checker needs a grid origin that is a multiple of res (octomap keys)";

// the whole-trajectory checkers take the trajectories *chunk at a time: the scratch holds their workspace afterwards
int traj_scratch(vigo_handle_t h, int T, int S, int* chunk) {
    *chunk = T < VIGO_TRAJ_CHUNK ? (T > 0 ? T : 1) : VIGO_TRAJ_CHUNK;
    return ensure_scratch(h, vigo::traj_ws_bytes(S, *chunk));
}

// the arguments vigo_astar_search and the entry points that run it share; astar_pool_fits: the VIGO_ASTAR_MAX_POOL_AXIS limit
bool astar_args_ok(const int32_t pool[3], double step, int path_cap, int max_expansions) {
    return pool && pool[0] >= 3 && pool[1] >= 3 && pool[2] >= 3 && step > 0.0 && step < 1e300 && path_cap >= 2 && max_expansions >= 0;
}
bool astar_pool_fits(const int32_t pool[3]) {
    return pool[0] <= VIGO_ASTAR_MAX_POOL_AXIS && pool[1] <= VIGO_ASTAR_MAX_POOL_AXIS && pool[2] <= VIGO_ASTAR_MAX_POOL_AXIS;
}

// the lattice (row-major float[nx][ny][nz], device) becomes the handle's ESDF: one 128-B line per cell group
int install_esdf(vigo_handle_t h, int nx, int ny, int nz, const double origin[3], double res, const float* dist_dev) {
    size_t bytes = vigo::esdf_bricked_floats(nx, ny, nz) * sizeof(float);   // 3.56x the lattice (one line per cell group)
    if (bytes > h->buf[vigo::kBufEsdf].bytes) {
        h->has_esdf = false;                 // the earlier field goes with its buffer: if the allocation fails, queries say so
        h->esdf_view.dist = nullptr;
    }
    VIGO_TRY(reserve(h, vigo::kBufEsdf, bytes, bytes));
    float* esdf = h->buf[vigo::kBufEsdf].as<float>();
    VIGO_HIP(h, (hipError_t)vigo::launch_esdf_brick(h->stream, nx, ny, nz, dist_dev, esdf));   // row-major -> one line per cell group
    h->esdf_view.dist = esdf;
    h->esdf_view.nx = nx; h->esdf_view.ny = ny; h->esdf_view.nz = nz;
    h->esdf_view.nby = vigo::esdf_bricks_along(ny); h->esdf_view.nbz = vigo::esdf_bricks_along(nz);
    h->esdf_view.res = res;
    for (int a = 0; a < 3; ++a) h->esdf_view.origin[a] = origin[a];
    h->has_esdf = true;
    return VIGO_OK;
}

// the checks vigo_build_esdf and vigo_build_esdf_tracked share
int check_esdf_build(vigo_handle_t h, const char* who, int plane) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, (std::string(who) + " before vigo_set_grid").c_str());
    const GridView& g = h->grid;
    if ((plane != 0 && plane != 2) || g.nx < 2 || g.ny < 2 || g.nz < 2)
        return fail(h, VIGO_ERR_INVALID_ARG, (std::string(who) + ": plane is not 0 or 2, or a grid axis < 2").c_str());
    if (vigo::esdf_empty_d2(g.nx, g.ny, g.nz) == 0)
        return fail(h, VIGO_ERR_UNSUPPORTED, (std::string(who) + ": nx^2 + ny^2 + nz^2 > 2^30 or more than 2^33 voxels").c_str());
    return VIGO_OK;
}

// tracking ends where the snapshot or the field stops being what vigo_build_esdf_tracked left and the updates kept
void end_esdf_tracking(vigo_handle_t h) {
    h->esdf_tracking = false;
    for (int a = 0; a < 3; ++a) h->esdf_pending_lo[a] = h->esdf_pending_n[a] = 0;
}

// a region update's box [lo, e) joins the pending box: the bounding box of both
void add_pending_box(vigo_handle_t h, const int lo[3], const int e[3]) {
    int32_t* plo = h->esdf_pending_lo;
    int32_t* pn = h->esdf_pending_n;
    const bool empty = pn[0] == 0;
    for (int a = 0; a < 3; ++a) {
        const int a0 = empty || lo[a] < plo[a] ? lo[a] : plo[a];
        const int e0 = empty || e[a] > plo[a] + pn[a] ? e[a] : plo[a] + pn[a];
        plo[a] = a0;
        pn[a] = e0 - a0;
    }
}

}  // namespace

extern "C" {

int vigo_abi_version(void) { return 4; }
double vigo_accumulated_time(double delT, int64_t k) { return vigo::accumulated_time(delT, k); }
double vigo_clock_table_time(double delT, int64_t k_last, int64_t k) {
    if (k_last < 0 || k < 0 || k > k_last || k_last > (int64_t)1 << 30) return NAN;
    vigo::ClockTable C;
    const double t_last = vigo::build_clock_table(delT, (int)k_last, C);
    if (C.n <= 0) return NAN;
    if (k == k_last && vigo::clock_at(C, (int)k) != t_last) return NAN;     // (the builder's own last value)
    return vigo::clock_at(C, (int)k);
}
int vigo_traj_sample_runs(int K, const double* knots, double delT, int32_t* run_first, int32_t* run_len, int32_t* n_total) {
    if (K < 0 || !knots || !n_total || (K > 0 && (!run_first || !run_len))) return VIGO_ERR_INVALID_ARG;
    *n_total = 0;
    int st = vigo::traj_knots_status(K, knots);
    int64_t n = 0;
    if (st == vigo::kTrajOk) st = vigo::traj_sample_count(knots[K], delT, &n);
    if (st != vigo::kTrajOk) return st;
    vigo::ClockTable C;                                  // the table k_traj_runs builds, and its searches
    (void)vigo::build_clock_table(delT, (int)n, C);
    int32_t lead, end_seg;
    vigo::traj_runs(K, knots, delT, n, &C, &lead, run_first, run_len, 1, &end_seg);
    *n_total = (int32_t)(n + 1);
    return VIGO_OK;
}
double vigo_exact_pow_dd(double t, int d, int* ambiguous) {
    // the first tier as the sampler kernels run it: t^0 = 1, t^1 = t, then the running double-double product
    bool amb = false;
    double hi = d <= 0 ? 1.0 : t, lo = 0.0;
    for (int i = 2; i <= d && i <= 15; ++i) amb |= vigo::pow_step(hi, lo, t);
    if (ambiguous) *ambiguous = amb ? 1 : 0;
    return hi;
}
double vigo_exact_pow(double t, int d) {
    if (d < 0 || d > 15) return NAN;
    if (t == 0.0) return vigo::pow_exact(t, d);   // (the first tier does not track the sign of a zero result)
    int amb = 0;
    const double v = vigo_exact_pow_dd(t, d, &amb);
    return amb ? vigo::pow_exact(t, d) : v;
}
double vigo_exact_pow_integer(double t, int d) { return (d < 0 || d > 15) ? NAN : vigo::pow_exact(t, d); }
const char* vigo_build_arch(void) { return "gfx950"; }

void vigo_default_params(vigo_params_t* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    // cfg/bspline_interactive/bspline_planner_param.yaml:4-19, BT.h:46-47
    p->dthresh = 0.5;
    p->dist_thresh_dynamic = 0.5;
    p->ts_ctrl = 0.2;
    p->ts = 0.1;
    p->pred_horizon = 2.0;
    p->uncertain_factor = 1.0;
    p->w_distance = 1.0;
    p->w_smoothness = 1.0;
    p->w_feasibility = 1.0;
    p->w_dynamic = 1.0;
    p->min_height = 0.7;
    p->max_height = 1.3;
    p->plan_in_z = 0;
    // BT.cpp:695-699 over LB:942-954
    p->mem_size = 16;
    p->max_iterations = 200;
    p->max_linesearch = 40;
    p->past = 0;
    p->g_epsilon = 0.01;
    p->delta = 1e-5;
    p->min_step = 1e-20;
    p->max_step = 1e20;
    p->f_dec_coeff = 1e-4;
    p->s_curv_coeff = 0.9;
    p->xtol = 1.0e-16;
}

int vigo_create(vigo_handle_t* out, int device_ordinal) {
    if (!out) return VIGO_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return VIGO_ERR_NO_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= count) return VIGO_ERR_INVALID_ARG;
    if (hipSetDevice(device_ordinal) != hipSuccess) return VIGO_ERR_NO_DEVICE;
    vigo_context* h = new vigo_context();
    h->device = device_ordinal;
    vigo_default_params(&h->params);
    h->dc = vigo::make_dev_const(h->params);
    bool ok = hipMalloc(reinterpret_cast<void**>(&h->dc_dev), sizeof(vigo::DevConst)) == hipSuccess &&
              hipMemcpy(h->dc_dev, &h->dc, sizeof(vigo::DevConst), hipMemcpyHostToDevice) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&h->dc_stage), vigo_context::kDcSlots * sizeof(vigo::DevConst)) == hipSuccess;
    for (int i = 0; ok && i < vigo_context::kDcSlots; ++i)
        ok = hipEventCreateWithFlags(&h->dc_event[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)vigo_destroy(h);
        return VIGO_ERR_HIP;
    }
    // launch geometry of this handle's device (plan_optimize decides one or two waves per SIMD from it)
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cus > 0)
        h->launch.simd_count = 4 * cus;
    *out = h;
    return VIGO_OK;
}

int vigo_destroy(vigo_handle_t h) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    for (const DevBuffer& b : h->buf)
        if (b.ptr) (void)hipFree(b.ptr);
    if (h->dc_dev) (void)hipFree(h->dc_dev);
    for (int i = 0; i < vigo_context::kDcSlots; ++i)
        if (h->dc_event[i]) (void)hipEventDestroy(h->dc_event[i]);
    if (h->dc_stage) (void)hipHostFree(h->dc_stage);
    for (int i = 0; i < vigo_context::kValidateSlots; ++i)
        if (h->validate_event[i]) (void)hipEventDestroy(h->validate_event[i]);
    if (h->validate_stage) (void)hipHostFree(h->validate_stage);
    delete h;
    return VIGO_OK;
}

int vigo_set_stream(vigo_handle_t h, void* hip_stream) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (s != h->stream) {
        // the handle's device-side state (solver constants, cached tables) is updated in stream order on the bound
        // stream: work still queued on the old stream must not see updates issued on the new one
        VIGO_HIP(h, hipStreamSynchronize(h->stream));
        h->stream = s;
    }
    return VIGO_OK;
}

int vigo_set_params(vigo_handle_t h, const vigo_params_t* p) {
    if (!h || !p) return VIGO_ERR_INVALID_ARG;
    if (p->mem_size <= 0 || p->mem_size > VIGO_MAX_MEM_SIZE) return fail(h, VIGO_ERR_UNSUPPORTED, "mem_size outside [1, VIGO_MAX_MEM_SIZE]");
    if (p->past != 0) return fail(h, VIGO_ERR_UNSUPPORTED, "past != 0 (delta test) is not implemented; the reference runs past = 0");
    // lbfgs.hpp treats max_iterations == 0 as "until convergence or error" (LB:127-131); a device kernel
    // must have a bound every wave reaches, so the unbounded setting is refused (the reference runs 200)
    if (p->max_iterations == 0) return fail(h, VIGO_ERR_UNSUPPORTED, "max_iterations == 0 (unbounded) is not supported on the device");
    // (finite: an infinite knot spacing makes the span search of the spline evaluation spin on NaN knots)
    if (!(p->ts > 0) || !(p->ts_ctrl > 0) || !(p->ts < 1e9) || !(p->ts_ctrl < 1e9)) return fail(h, VIGO_ERR_INVALID_ARG, "ts and ts_ctrl must be finite and > 0");
    // every device loop needs a bound a wave reaches in reasonable time (the reference runs 200 / 40)
    if (p->max_iterations > 1000000 || p->max_linesearch > 100000)
        return fail(h, VIGO_ERR_UNSUPPORTED, "max_iterations > 1e6 or max_linesearch > 1e5");
    // predictionNum = int(predHorizon / ts) divides n in the dynamic-obstacle term (BT.cpp:1006, :1020): 0 is a
    // division by zero in the reference; a huge value is an unbounded device loop
    if (!(p->pred_horizon / p->ts >= 1.0) || !(p->pred_horizon / p->ts <= 100000.0))
        return fail(h, VIGO_ERR_INVALID_ARG, "pred_horizon / ts must lie in [1, 1e5]");
    // the argument checks of lbfgs_optimize (LB:1060-1104): refuse here rather than per trajectory
    if (p->g_epsilon < 0. || p->delta < 0. || p->min_step < 0. || p->max_step < p->min_step ||
        p->f_dec_coeff < 0. || p->s_curv_coeff <= p->f_dec_coeff || 1. <= p->s_curv_coeff ||
        p->xtol < 0. || p->max_linesearch <= 0 || p->max_iterations < 0)
        return fail(h, VIGO_ERR_INVALID_ARG, "invalid L-BFGS parameter (see lbfgs.hpp:1060-1104)");
    if (memcmp(&h->params, p, sizeof(*p)) == 0) return VIGO_OK;   // unchanged (callers re-send them per round): no copy, no sync
    // The kernels read the constants through dc_dev for the whole solve, and launches are asynchronous: the
    // refresh is therefore ordered WITH the bound stream (an async copy from a pinned staging slot), after every
    // solve already queued there and before every later one — a blocking copy on the null stream would change
    // max_iterations, the weights, ... under a solve still running on a non-blocking stream.
    const int slot = h->dc_next;
    VIGO_HIP(h, hipEventSynchronize(h->dc_event[slot]));          // the slot's previous copy (4 refreshes ago) has left it
    h->dc_stage[slot] = vigo::make_dev_const(*p);
    VIGO_HIP(h, hipMemcpyAsync(h->dc_dev, &h->dc_stage[slot], sizeof(vigo::DevConst), hipMemcpyHostToDevice, h->stream));
    VIGO_HIP(h, hipEventRecord(h->dc_event[slot], h->stream));
    h->dc_next = (slot + 1) % vigo_context::kDcSlots;
    h->params = *p;
    h->dc = h->dc_stage[slot];
    return VIGO_OK;
}

int vigo_get_params(vigo_handle_t h, vigo_params_t* p) {
    if (!h || !p) return VIGO_ERR_INVALID_ARG;
    *p = h->params;
    return VIGO_OK;
}

int vigo_set_precision(vigo_handle_t h, int precision) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (precision != VIGO_PREC_F64 && precision != VIGO_PREC_F32 && precision != VIGO_PREC_F64_FAST) return fail(h, VIGO_ERR_INVALID_ARG, "unknown precision");
    h->precision = precision;
    return VIGO_OK;
}

const char* vigo_last_error(vigo_handle_t h) { return h ? h->last_error.c_str() : "null handle"; }

/* ---- voxel map ---------------------------------------------------------------------- */

size_t vigo_grid_packed_bytes(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
    return (size_t)3 * nx * ny * ((nz + 31) / 32) * sizeof(uint32_t);
}

int vigo_pack_grid(vigo_handle_t h, int nx, int ny, int nz, const uint8_t* voxels_dev, uint32_t* packed_dev) {
    if (!h || !voxels_dev || !packed_dev || nx <= 0 || ny <= 0 || nz <= 0) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_pack_grid: bad argument");
    VIGO_HIP(h, (hipError_t)vigo::launch_pack_grid(h->stream, nx, ny, nz, voxels_dev, packed_dev));
    return VIGO_OK;
}

int vigo_inflate_grid(vigo_handle_t h, int nx, int ny, int nz, uint8_t* voxels_dev, int rx, int ry, int rz) {
    if (!h || !voxels_dev || nx <= 0 || ny <= 0 || nz <= 0 || rx < 0 || ry < 0 || rz < 0 || (size_t)nx * ny * nz > ((size_t)1 << 31))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_inflate_grid: bad argument");
    if (rz > 31) return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_inflate_grid: rz > 31 voxels");
    const size_t nw = (size_t)nx * ny * ((nz + 31) / 32);
    uint32_t *planeA, *planeB;
    VIGO_TRY(carve(h, vigo::kBufScratch, kSlack, [&](void* p) { return vigo::ws_pair(p, nw, planeA, planeB); }));
    VIGO_HIP(h, (hipError_t)vigo::launch_inflate(h->stream, nx, ny, nz, voxels_dev, planeA, planeB, rx, ry, rz));
    return VIGO_OK;
}

int vigo_set_grid(vigo_handle_t h, int nx, int ny, int nz, const double origin[3], double res, const uint8_t* voxels_dev) {
    if (!h || !voxels_dev || !origin || nx <= 0 || ny <= 0 || nz <= 0 || !geometry_ok(origin, res)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_set_grid: bad argument");
    end_esdf_tracking(h);
    VIGO_TRY(ensure_grid_storage(h, nx, ny, nz));
    VIGO_HIP(h, (hipError_t)vigo::launch_pack_grid(h->stream, nx, ny, nz, voxels_dev, h->buf[vigo::kBufGrid].as<uint32_t>()));
    fill_grid_view(h, nx, ny, nz, origin, res);
    return VIGO_OK;
}

int vigo_set_grid_host(vigo_handle_t h, int nx, int ny, int nz, const double origin[3], double res, const uint8_t* voxels_host) {
    if (!h || !voxels_host || !origin || nx <= 0 || ny <= 0 || nz <= 0 || !geometry_ok(origin, res)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_set_grid_host: bad argument");
    size_t bytes = (size_t)nx * ny * nz;
    VIGO_TRY(ensure_scratch(h, bytes));
    uint8_t* staged = h->buf[vigo::kBufScratch].as<uint8_t>();
    VIGO_HIP(h, hipMemcpyAsync(staged, voxels_host, bytes, hipMemcpyHostToDevice, h->stream));
    VIGO_TRY(vigo_set_grid(h, nx, ny, nz, origin, res, staged));
    VIGO_HIP(h, hipStreamSynchronize(h->stream));
    return VIGO_OK;
}

int vigo_set_grid_packed(vigo_handle_t h, int nx, int ny, int nz, const double origin[3], double res, const uint32_t* packed_dev) {
    if (!h || !packed_dev || !origin || nx <= 0 || ny <= 0 || nz <= 0 || !geometry_ok(origin, res)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_set_grid_packed: bad argument");
    end_esdf_tracking(h);
    VIGO_TRY(ensure_grid_storage(h, nx, ny, nz));
    VIGO_HIP(h, hipMemcpyAsync(h->buf[vigo::kBufGrid].ptr, packed_dev, vigo_grid_packed_bytes(nx, ny, nz), hipMemcpyDeviceToDevice, h->stream));
    fill_grid_view(h, nx, ny, nz, origin, res);
    return VIGO_OK;
}

}  // extern "C"
namespace {
int region_code(vigo::RegionCheck c) {
    return c == vigo::kRegionInvalid ? VIGO_ERR_INVALID_ARG : c == vigo::kRegionUnsupported ? VIGO_ERR_UNSUPPORTED : VIGO_OK;
}
// both forms of vigo_update_grid_region: every refusal comes before the first copy or launch.  Grid dims, origin, res, the
// metric bounds, the ESDF and the cached clocks are not touched.
int update_grid_region(vigo_handle_t h, const char* who, const int32_t lo[3], const int32_t n[3], const uint8_t* vox, bool on_host,
                       const int32_t* r) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (!lo || !n || !vox) return fail(h, VIGO_ERR_INVALID_ARG, (std::string(who) + ": NULL argument").c_str());
    for (int a = 0; a < 3; ++a)
        if (lo[a] < 0 || n[a] < 0 || (r && r[a] < 0)) return fail(h, VIGO_ERR_INVALID_ARG, (std::string(who) + ": negative lo, n or radius").c_str());
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, (std::string(who) + " before vigo_set_grid").c_str());
    const GridView& g = h->grid;
    const vigo::RegionCheck rc = vigo::region_check(g.nx, g.ny, g.nz, lo, n, r);
    if (rc == vigo::kRegionInvalid) return fail(h, VIGO_ERR_INVALID_ARG, (std::string(who) + ": lo + n beyond the grid").c_str());
    if (rc == vigo::kRegionUnsupported) return fail(h, VIGO_ERR_UNSUPPORTED, (std::string(who) + ": rz > 31 voxels").c_str());
    if (rc == vigo::kRegionEmpty) return VIGO_OK;
    const vigo::RegionPlan p = vigo::region_plan(g.nx, g.ny, g.nz, lo, n, r);
    if (h->esdf_tracking) {                   // host bookkeeping for vigo_update_esdf: every plane this call may change
        const int box_e[3] = {lo[0] + n[0], lo[1] + n[1], lo[2] + n[2]};
        add_pending_box(h, r ? p.a1 : p.lo, r ? p.e1 : box_e);
    }
    const size_t bytes = (size_t)n[0] * n[1] * n[2];
    uint8_t* staged;
    uint32_t *planeA, *planeB;
    VIGO_TRY(carve(h, vigo::kBufScratch, kSlack,
                   [&](void* b) { return vigo::ws_grid_update(b, on_host ? bytes : 0, vigo::region_window_words(p), staged, planeA, planeB); }));
    if (on_host) VIGO_HIP(h, hipMemcpyAsync(staged, vox, bytes, hipMemcpyHostToDevice, h->stream));
    VIGO_HIP(h, (hipError_t)vigo::launch_grid_region(h->stream, p, on_host ? staged : vox, h->buf[vigo::kBufGrid].as<uint32_t>(), g.plane_words,
                                                     planeA, planeB));
    if (on_host) VIGO_HIP(h, hipStreamSynchronize(h->stream));
    return VIGO_OK;
}
}  // namespace
extern "C" {

int vigo_update_grid_region(vigo_handle_t h, const int32_t lo[3], const int32_t n[3], const uint8_t* voxels_dev, const int32_t inflate_r[3]) {
    return update_grid_region(h, "vigo_update_grid_region", lo, n, voxels_dev, false, inflate_r);
}

int vigo_update_grid_region_host(vigo_handle_t h, const int32_t lo[3], const int32_t n[3], const uint8_t* voxels_host, const int32_t inflate_r[3]) {
    return update_grid_region(h, "vigo_update_grid_region_host", lo, n, voxels_host, true, inflate_r);
}

int vigo_get_grid_packed(vigo_handle_t h, uint32_t* packed_dev) {
    if (!h || !packed_dev) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_get_grid_packed: bad argument");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_get_grid_packed before vigo_set_grid");
    VIGO_HIP(h, hipMemcpyAsync(packed_dev, h->buf[vigo::kBufGrid].ptr, vigo_grid_packed_bytes(h->grid.nx, h->grid.ny, h->grid.nz), hipMemcpyDeviceToDevice, h->stream));
    return VIGO_OK;
}

int vigo_grid_region_apply_host(int nx, int ny, int nz, uint8_t* voxels_host_inout, const int32_t lo[3], const int32_t n[3],
                                const uint8_t* region_voxels_host, const int32_t inflate_r[3]) {
    if (nx <= 0 || ny <= 0 || nz <= 0 || !voxels_host_inout || !lo || !n || !region_voxels_host) return VIGO_ERR_INVALID_ARG;
    return region_code(vigo::grid_region_apply(nx, ny, nz, voxels_host_inout, lo, n, region_voxels_host, inflate_r));
}

int vigo_set_metric_bounds(vigo_handle_t h, const double bmin[3], const double bmax[3]) {
    if (!h || !bmin || !bmax) return VIGO_ERR_INVALID_ARG;
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_set_metric_bounds before vigo_set_grid");
    for (int a = 0; a < 3; ++a) { h->grid.bmin[a] = bmin[a]; h->grid.bmax[a] = bmax[a]; }
    return VIGO_OK;
}

int vigo_query_points(vigo_handle_t h, int which, int64_t Q, const double* pts, uint8_t* out) {
    if (!h || Q < 0 || (Q > 0 && (!pts || !out)) || which < 0 || which > 1) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_query_points: bad argument");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_query_points before vigo_set_grid");
    VIGO_HIP(h, (hipError_t)vigo::launch_query_points(h->stream, h->grid, which, Q, pts, 3, out));
    return VIGO_OK;
}

int vigo_guides_unknown(vigo_handle_t h, int64_t G, const double* guide_pv, uint8_t* out_unk) {
    if (!h || G < 0 || (G > 0 && (!guide_pv || !out_unk))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_guides_unknown: bad argument");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_guides_unknown before vigo_set_grid");
    VIGO_HIP(h, (hipError_t)vigo::launch_query_points(h->stream, h->grid, 1, G, guide_pv, 6, out_unk));
    return VIGO_OK;
}

int vigo_check_lists(vigo_handle_t h, int B, int N, const int32_t* guide_off, int64_t G, const int32_t* obs_off, int64_t O) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || N < 1 || G < 0 || O < 0) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_check_lists: bad argument");
    if (B == 0 || (!guide_off && !obs_off)) return 0;
    VIGO_TRY(ensure_scratch(h, 64));
    int* bad = h->buf[vigo::kBufScratch].as<int>();
    VIGO_HIP(h, (hipError_t)vigo::launch_check_lists(h->stream, B, N, guide_off, G, obs_off, O, bad));
    int host_bad = 0;
    VIGO_TRY(read_back(h, &host_bad, bad, sizeof(int)));
    return host_bad;
}

/* ---- ViGO cost / gradient / solve ----------------------------------------------------- */

int vigo_cost_grad(vigo_handle_t h, int B, int N, const double* ctrl, const int32_t* guide_off,
                   const double* guide_pv, const uint8_t* guide_unk, const int32_t* obs_off,
                   const double* obs, int n_obs_shared, const double* weights, double* out_cost,
                   double* out_grad, double* out_terms) {
    VIGO_TRY(check_solve_args(h, B, N, ctrl));
    VIGO_TRY(check_list_args(h, n_obs_shared));
    SolveArgs a = solve_args(B, N, const_cast<double*>(ctrl), guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights);
    a.out_cost = out_cost; a.out_grad = out_grad; a.out_terms = out_terms;
    VIGO_HIP(h, (hipError_t)vigo::launch_cost_grad(h->stream, a, h->dc, h->dc_dev, h->precision));
    return VIGO_OK;
}

int vigo_optimize(vigo_handle_t h, int B, int N, double* ctrl, const int32_t* guide_off,
                  const double* guide_pv, const uint8_t* guide_unk, const int32_t* obs_off,
                  const double* obs, int n_obs_shared, const double* weights, double* out_x,
                  int32_t* out_status, double* out_fx, int32_t* out_iters, int32_t* out_evals) {
    VIGO_TRY(check_solve_args(h, B, N, ctrl));
    VIGO_TRY(check_list_args(h, n_obs_shared));
    SolveArgs a = solve_args(B, N, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights);
    a.out_x = out_x; a.out_status = out_status; a.out_fx = out_fx;
    a.out_iters = out_iters; a.out_evals = out_evals;
    if (!lds_fits(h, N)) return fail(h, VIGO_ERR_UNSUPPORTED_N, kLdsMsg);
    VIGO_HIP(h, (hipError_t)vigo::launch_optimize(h->stream, a, h->dc, h->dc_dev, h->precision, h->launch));
    return VIGO_OK;
}

int vigo_cost_grad_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const int32_t* guide_off,
                         const double* guide_pv, const uint8_t* guide_unk, const int32_t* obs_off, const double* obs,
                         int n_obs_shared, const double* weights, double* out_cost, double* out_grad, double* out_terms) {
    VIGO_TRY(check_mixed_args(h, B, Ns, n_pts, ctrl));
    VIGO_TRY(check_list_args(h, n_obs_shared));
    SolveArgs a = solve_args(B, Ns, const_cast<double*>(ctrl), guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights);
    a.out_cost = out_cost; a.out_grad = out_grad; a.out_terms = out_terms;
    VIGO_HIP(h, (hipError_t)vigo::launch_cost_grad_mixed(h->stream, mixed_args(a, n_pts), h->dc_dev, h->precision));
    return VIGO_OK;
}

int vigo_optimize_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, double* ctrl, const int32_t* guide_off,
                        const double* guide_pv, const uint8_t* guide_unk, const int32_t* obs_off, const double* obs,
                        int n_obs_shared, const double* weights, double* out_x, int32_t* out_status, double* out_fx,
                        int32_t* out_iters, int32_t* out_evals) {
    VIGO_TRY(check_mixed_args(h, B, Ns, n_pts, ctrl));
    VIGO_TRY(check_list_args(h, n_obs_shared));
    SolveArgs a = solve_args(B, Ns, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights);
    a.out_x = out_x; a.out_status = out_status; a.out_fx = out_fx;
    a.out_iters = out_iters; a.out_evals = out_evals;
    VIGO_HIP(h, (hipError_t)vigo::launch_optimize_mixed(h->stream, mixed_args(a, n_pts), h->dc, h->dc_dev, h->precision, h->launch));
    return VIGO_OK;
}

}  // extern "C"

namespace {
// vigo_rebound_rounds (n_pts == NULL: B trajectories of N control points) and vigo_rebound_rounds_mixed (rows of N, counts
// n_pts): the same queue of launches, the solves by launch_optimize / launch_optimize_mixed
int rebound_rounds(vigo_handle_t h, int B, int N, const int32_t* n_pts, double* ctrl, const int32_t* guide_off, const double* guide_pv,
                   const uint8_t* guide_unk, const int32_t* obs_off, const double* obs, int n_obs_shared, double* weights,
                   double gate_dt, double not_check_ratio, int max_rounds, vigo_rebound_state_t* state) {
    VIGO_TRY(check_list_args(h, n_obs_shared));
    if (B > 0 && (!weights || !state)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_rebound_rounds: weights and state are required");
    if (max_rounds < 0 || max_rounds > 64 || !(not_check_ratio >= 0.0 && not_check_ratio < 1.0))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_rebound_rounds: max_rounds outside [0, 64] or not_check_ratio outside [0, 1)");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_rebound_rounds before vigo_set_grid");
    if (!lds_fits(h, N)) return fail(h, VIGO_ERR_UNSUPPORTED_N, kLdsMsg);
    if (B == 0) return VIGO_OK;
    int T = 0;
    const double* times = nullptr;
    // (mixed: the sample clock depends on gate_dt and k only, so the table of the longest duration serves every count)
    VIGO_TRY(upload_sample_times(h, (N - 3) * h->params.ts_ctrl, gate_dt, &T, &times));
    auto static_samples = [&](int n, int all) {   // see T_static below
        const int t = count_sample_times(gate_dt, (1.0 - not_check_ratio) * ((n - 3) * h->params.ts_ctrl));
        return t < 0 || t > all ? all : t;
    };
    // compacted active set: count = flags[0]; flags[1], flags[2]: "a trajectory waits for the host"
    int32_t *count, *idx, *count_tab = nullptr;
    if (n_pts) {
        VIGO_TRY(carve(h, vigo::kBufRebound, kExact, [&](void* p) { return vigo::ws_rebound_mixed(p, B, N, count, idx, count_tab); }));
        // {T, T_static} of every count 7 .. N, by the host function that counts the uniform entry's samples
        int32_t tab[2 * (vigo::kMixedMaxStride - 6)];
        for (int n = 7; n <= N; ++n) {
            int t = count_sample_times(gate_dt, (n - 3) * h->params.ts_ctrl);
            if (t < 0 || t > T) t = T;
            tab[2 * (n - 7)] = t;
            tab[2 * (n - 7) + 1] = static_samples(n, t);
        }
        VIGO_HIP(h, hipMemcpyAsync(count_tab, tab, 2 * (size_t)(N - 6) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        VIGO_HIP(h, hipStreamSynchronize(h->stream));   // tab is on this stack frame
        VIGO_HIP(h, (hipError_t)vigo::launch_rebound_check_counts(h->stream, B, N, n_pts, state));
    } else {
        VIGO_TRY(carve(h, vigo::kBufRebound, kExact, [&](void* p) { return vigo::ws_rebound(p, B, count, idx); }));
    }
    VIGO_HIP(h, hipMemsetAsync(count, 0, 16 * sizeof(int32_t), h->stream));
    SolveArgs a = solve_args(B, N, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights);
    a.active_idx = idx; a.active_count = count;
    a.out_status = &state[0].lbfgs_status;
    a.status_stride = (int)(sizeof(vigo_rebound_state_t) / sizeof(int32_t));
    vigo::ReboundArgs r{};
    r.B = B; r.N = N; r.ctrl = ctrl;
    r.guide_off = guide_off; r.guide_pv = guide_pv;
    r.obs_off = obs_off; r.obs = obs; r.n_obs_shared = n_obs_shared;
    r.weights = weights; r.state = state;
    r.ts_ctrl = h->params.ts_ctrl; r.T = T; r.times = times;
    // the static gate stops at (1 - notCheckRatio_) * duration (BT.h:313); the dynamic one samples the whole
    // trajectory (evalTraj(), BT.h:345) — a prefix of the same clock
    r.T_static = static_samples(N, T);
    r.dthresh = h->params.dthresh; r.not_check_ratio = not_check_ratio;
    r.flags = count;
    r.n_pts = n_pts; r.count_tab = count_tab;
    const vigo::MixedSolveArgs am = mixed_args(a, n_pts);
    auto solve = [&]() {
        return (hipError_t)(n_pts ? vigo::launch_optimize_mixed(h->stream, am, h->dc, h->dc_dev, h->precision, h->launch)
                                  : vigo::launch_optimize(h->stream, a, h->dc, h->dc_dev, h->precision, h->launch));
    };
    // the optimize() a trajectory still owes (BT.cpp:612 / after a host-side re-guide) ...
    VIGO_HIP(h, (hipError_t)vigo::launch_rebound_compact(h->stream, B, state, 0, idx, count));
    VIGO_HIP(h, solve());
    // ... then the rounds: gates + decision, compaction of the still-active set, optimize
    for (int round = 0; round < max_rounds; ++round) {
        VIGO_HIP(h, (hipError_t)vigo::launch_rebound_decide(h->stream, h->grid, r));
        VIGO_HIP(h, (hipError_t)vigo::launch_rebound_compact(h->stream, B, state, 1, idx, count));
        VIGO_HIP(h, solve());
    }
    return VIGO_OK;
}
}  // namespace

extern "C" {

int vigo_rebound_rounds(vigo_handle_t h, int B, int N, double* ctrl, const int32_t* guide_off, const double* guide_pv,
                        const uint8_t* guide_unk, const int32_t* obs_off, const double* obs, int n_obs_shared, double* weights,
                        double gate_dt, double not_check_ratio, int max_rounds, vigo_rebound_state_t* state) {
    VIGO_TRY(check_solve_args(h, B, N, ctrl));
    return rebound_rounds(h, B, N, nullptr, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights, gate_dt,
                          not_check_ratio, max_rounds, state);
}

int vigo_rebound_rounds_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, double* ctrl, const int32_t* guide_off,
                              const double* guide_pv, const uint8_t* guide_unk, const int32_t* obs_off, const double* obs,
                              int n_obs_shared, double* weights, double gate_dt, double not_check_ratio, int max_rounds,
                              vigo_rebound_state_t* state) {
    VIGO_TRY(check_mixed_args(h, B, Ns, n_pts, ctrl));
    return rebound_rounds(h, B, Ns, n_pts, ctrl, guide_off, guide_pv, guide_unk, obs_off, obs, n_obs_shared, weights, gate_dt,
                          not_check_ratio, max_rounds, state);
}

/* ---- B-spline fit, evaluation and gates ------------------------------------------------- */

int vigo_bspline_fit(vigo_handle_t h, int B, int K, double ts, const double* points, const double* conds, double* ctrl_out) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || !(ts > 0) || (B > 0 && (!points || !ctrl_out))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_bspline_fit: bad argument");
    // bspline.cpp:83-87 needs at least 4 points; K + 2 control points must fit the solver's range
    if (K < 4 || K + 2 > VIGO_MAX_CTRL_POINTS) return fail(h, VIGO_ERR_UNSUPPORTED_N, "K outside [4, VIGO_MAX_CTRL_POINTS - 2]");
    if (h->fit_K != K || h->fit_ts != ts) {
        // one-off per (K, ts): factorise A on the device, keep the least-squares operator
        const size_t need = vigo::fit_pinv_doubles(K) * sizeof(double);
        h->fit_K = 0;                                   // no operator cached while the buffer is regrown or refilled
        VIGO_TRY(reserve(h, vigo::kBufFit, need, need));
        VIGO_TRY(ensure_scratch(h, vigo::fit_work_doubles(K) * sizeof(double)));
        VIGO_HIP(h, (hipError_t)vigo::launch_fit_setup(h->stream, K, ts, h->buf[vigo::kBufScratch].as<double>(), h->buf[vigo::kBufFit].as<double>()));
        h->fit_K = K;
        h->fit_ts = ts;
    }
    VIGO_HIP(h, (hipError_t)vigo::launch_bspline_fit(h->stream, B, K, h->buf[vigo::kBufFit].as<double>(), points, conds, ctrl_out));
    return VIGO_OK;
}

int vigo_bspline_fit_mixed(vigo_handle_t h, int T, int Ns, double ts, const int32_t* n_fit, const int32_t* status,
                           const double* points, int point_stride, const double* conds, double* ctrl_out, int32_t* out_n_pts) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (T < 0 || !(ts > 0) || !isfinite(ts) || point_stride < 1 || (T > 0 && (!n_fit || !points || !ctrl_out || !out_n_pts)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_bspline_fit_mixed: bad argument");
    if (Ns < vigo::kFitMixedMinStride || Ns > vigo::kFitMixedMaxStride)
        return fail(h, VIGO_ERR_UNSUPPORTED_N, "vigo_bspline_fit_mixed: Ns outside [7, 64]");
    if (T == 0) return VIGO_OK;
    // one-off per ts: the operator of EVERY count, each by k_fit_setup's arithmetic — the host never learns which occur
    const bool build = h->fit_table_ts != ts;
    if (build) {
        h->fit_table_ts = 0.0;                          // no table cached while the buffer is made or refilled
        const size_t need = vigo::fit_table_doubles() * sizeof(double);
        VIGO_TRY(reserve(h, vigo::kBufFitTable, need, need));
    }
    int32_t *perm, *tab;
    double* work;
    VIGO_TRY(carve(h, vigo::kBufScratch, kSlack, [&](void* p) {
        return vigo::ws_fit_mixed(p, (size_t)T, 2 * (vigo::kFitBins + 1), build ? vigo::fit_table_work_doubles() : 0, perm, tab, work);
    }));
    double* table = h->buf[vigo::kBufFitTable].as<double>();
    if (build) {
        VIGO_HIP(h, (hipError_t)vigo::launch_fit_setup_table(h->stream, ts, work, table));
        h->fit_table_ts = ts;
    }
    VIGO_HIP(h, (hipError_t)vigo::launch_bspline_fit_mixed(h->stream, T, Ns, point_stride, table, n_fit, status, points, conds, perm,
                                                           tab, ctrl_out, out_n_pts));
    return VIGO_OK;
}

int vigo_bspline_eval(vigo_handle_t h, int B, int N, const double* ctrl, int deriv, int T,
                      const double* times, double* out) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || T < 0 || deriv < 0 || deriv > 2 || ((B > 0 && T > 0) && (!ctrl || !times || !out)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_bspline_eval: bad argument");
    if (!gate_N_ok(N)) return fail(h, VIGO_ERR_UNSUPPORTED_N, kGateNMsg);
    VIGO_HIP(h, (hipError_t)vigo::launch_bspline_eval(h->stream, B, N, ctrl, h->params.ts_ctrl, deriv, T, times, out));
    return VIGO_OK;
}

int vigo_traj_collision(vigo_handle_t h, int B, int N, const double* ctrl, double dt,
                        uint8_t* out_flag, int32_t* out_first) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!ctrl || !out_flag))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_collision: bad argument");
    if (!gate_N_ok(N)) return fail(h, VIGO_ERR_UNSUPPORTED_N, kGateNMsg);
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_traj_collision before vigo_set_grid");
    int T = 0;
    const double* times = nullptr;
    double duration = (N - 3) * h->params.ts_ctrl;  // knots(N), BS.cpp:27
    VIGO_TRY(upload_sample_times(h, (1.0 - 0.0) * duration, dt, &T, &times));
    VIGO_HIP(h, (hipError_t)vigo::launch_traj_collision(h->stream, h->grid, B, N, ctrl, h->params.ts_ctrl, T, times, out_flag, out_first));
    return VIGO_OK;
}

int vigo_traj_dynamic_collision(vigo_handle_t h, int B, int N, const double* ctrl, double dt,
                                const int32_t* obs_off, const double* obs, int n_obs_shared,
                                uint8_t* out_flag) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!ctrl || !out_flag)) || n_obs_shared < 0) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_dynamic_collision: bad argument");
    if (!gate_N_ok(N)) return fail(h, VIGO_ERR_UNSUPPORTED_N, kGateNMsg);
    VIGO_TRY(check_list_args(h, n_obs_shared));
    int T = 0;
    const double* times = nullptr;
    double duration = (N - 3) * h->params.ts_ctrl;
    VIGO_TRY(upload_sample_times(h, duration, dt, &T, &times));
    VIGO_HIP(h, (hipError_t)vigo::launch_traj_dynamic_collision(h->stream, B, N, ctrl, h->params.ts_ctrl, T, times, obs_off, obs, n_obs_shared, out_flag));
    return VIGO_OK;
}

int vigo_traj_finish(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const double* limits, double sample_dt,
                     int S_cap, double* out_factor, double* out_max, int32_t* out_n, double* out_pos, double* out_vel, int32_t* out_status) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    const double ts = h->params.ts, ts_ctrl = h->params.ts_ctrl;
    if (B < 0 || S_cap < 1 || !(sample_dt > 0.0) || !isfinite(sample_dt) || !(ts > 0.0) || !isfinite(ts) || !(ts_ctrl > 0.0) || !isfinite(ts_ctrl) ||
        (B > 0 && (!ctrl || !limits || !out_factor || !out_n || !out_pos || !out_status)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_finish: bad argument");
    if (Ns < 7 || Ns > VIGO_MAX_CTRL_POINTS) return fail(h, VIGO_ERR_UNSUPPORTED_N, "Ns outside [7, VIGO_MAX_CTRL_POINTS]");
    if (B == 0) return VIGO_OK;
    vigo::FinishArgs a{};
    a.B = B; a.Ns = Ns; a.n_pts = n_pts; a.ctrl = ctrl; a.limits = limits;
    a.ts_ctrl = ts_ctrl; a.sample_dt = sample_dt; a.S_cap = S_cap;
    // (the clocks depend on the step and k only: the tables of the longest duration serve every count)
    const double longest = (Ns - 3) * ts_ctrl;
    VIGO_TRY(upload_finish_clock(h, 0, longest, ts, &a.T_ts, &a.times_ts));
    VIGO_TRY(upload_finish_clock(h, 1, longest, sample_dt, &a.T_dt, &a.times_dt));
    a.out_factor = out_factor; a.out_max = out_max; a.out_n = out_n; a.out_pos = out_pos; a.out_vel = out_vel; a.out_status = out_status;
    VIGO_HIP(h, (hipError_t)vigo::launch_traj_finish(h->stream, a));
    return VIGO_OK;
}

int vigo_traj_validate(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, double dt, double not_check_ratio, int rule,
                       const int32_t* obs_off, const double* obs, int n_obs_shared, int32_t* out_status, int32_t* out_first, double* out_pos,
                       int32_t* out_dyn_first, int32_t* out_invalid, int32_t* out_n_invalid) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    const double ts_ctrl = h->params.ts_ctrl;
    if (B < 0 || !vigo::finish_step_ok(dt) || !vigo::finish_step_ok(ts_ctrl) || !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0) ||
        (rule != VIGO_VALIDATE_BY_TIME && rule != VIGO_VALIDATE_BY_INDEX) || n_obs_shared < 0 || (B > 0 && (!ctrl || !out_status || !out_first)) ||
        (!out_invalid != !out_n_invalid))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_validate: bad argument");
    if (Ns < vigo::kValidateMinN || Ns > VIGO_MAX_CTRL_POINTS) return fail(h, VIGO_ERR_UNSUPPORTED_N, kGateNMsg);
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_traj_validate before vigo_set_grid");
    if (B == 0) return VIGO_OK;
    vigo::ValidateArgs a{};
    a.B = B; a.Ns = Ns; a.n_pts = n_pts; a.ctrl = ctrl; a.ts_ctrl = ts_ctrl;
    VIGO_TRY(upload_validate_tab(h, dt, not_check_ratio, rule, Ns, &a.count_tab));
    // (the clock depends on dt and k only: the table of the longest duration serves every count)
    VIGO_TRY(upload_clock_slot(h, h->validate_clock, vigo::kBufValidateClock, false, (Ns - 3) * ts_ctrl, dt, &a.T, &a.times));
    a.obs_off = obs_off; a.obs = obs; a.n_obs_shared = n_obs_shared;
    a.out_status = out_status; a.out_first = out_first; a.out_pos = out_pos; a.out_dyn_first = out_dyn_first;
    a.out_invalid = out_invalid; a.out_n_invalid = out_n_invalid;
    VIGO_HIP(h, (hipError_t)vigo::launch_traj_validate(h->stream, h->grid, a));
    return VIGO_OK;
}

int vigo_ctrl_occupancy(vigo_handle_t h, int B, int N, const double* ctrl, uint8_t* out_pt, uint8_t* out_line) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || N < 1 || (B > 0 && (!ctrl || !out_pt || !out_line))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_ctrl_occupancy: bad argument");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_ctrl_occupancy before vigo_set_grid");
    VIGO_HIP(h, (hipError_t)vigo::launch_ctrl_occupancy(h->stream, h->grid, B, N, ctrl, out_pt, out_line));
    return VIGO_OK;
}

/* ---- min-snap QP and corridor checker ---------------------------------------------------- */

int vigo_minsnap_supported(int W, int deg, int diff, int cont) { return vigo::minsnap_supported(W, deg, diff, cont) ? 1 : 0; }

int vigo_minsnap(vigo_handle_t h, int T, int W, int deg, int diff, int cont, double desired_vel, double corridor_res,
                 const double* waypoints, const double* corridor, const double* conds, double* out_coeffs,
                 double* out_knots, int32_t* out_status) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (T < 0 || !(desired_vel > 0) || (corridor && !(corridor_res > 0)) || (T > 0 && (!waypoints || !out_coeffs || !out_knots || !out_status)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_minsnap: bad argument");
    if (deg != 7 || diff < 1 || diff > deg) return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_minsnap: degree 7 polynomials only (polynomial_degree of cfg/planner*.yaml)");
    if (W < 2 || W > vigo::minsnap_max_waypoints()) return fail(h, VIGO_ERR_UNSUPPORTED_N, "vigo_minsnap: 2..11 waypoints per path on the device");
    if (!vigo_minsnap_supported(W, deg, diff, cont))
        return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_minsnap: continuity degree outside what one wavefront / 160 KiB of LDS holds");
    VIGO_HIP(h, (hipError_t)vigo::launch_minsnap(h->stream, T, W, deg, diff, cont, desired_vel, corridor_res, waypoints, corridor, conds,
                                                 out_coeffs, out_knots, out_status, h->launch));
    return VIGO_OK;
}


int vigo_corridor_check(vigo_handle_t h, int S, int deg, const double* coeffs, const int32_t* n_samp,
                        const double* delT, const double box[3], double map_res, uint8_t* out_flag,
                        int32_t* out_first, int32_t* out_count) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (S < 0 || deg < 0 || deg > 15 || !box || !(map_res > 0) || (S > 0 && (!coeffs || !n_samp || !delT || !out_flag)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_corridor_check: bad argument");
    if (!sweep_box_ok(box, map_res)) return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_corridor_check: collision box not finite or more than 32768 lattice points per pose");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_corridor_check before vigo_set_grid");
    if (!key_lattice_ok(h->grid)) return fail(h, VIGO_ERR_UNSUPPORTED, kKeyLatticeMsg);
    if (S == 0) return VIGO_OK;
    // scratch: the first pass' work list for the second, then (up to 16384 segments: 42 MB) the segments' clock tables
    const size_t clock_bytes = S <= 16384 ? vigo::corridor_clock_ws_bytes(S) : 0;
    int* todo;
    void* clock_ws;
    VIGO_TRY(carve(h, vigo::kBufScratch, kSlack, [&](void* p) { return vigo::ws_corridor(p, S, clock_bytes, todo, clock_ws); }));
    VIGO_HIP(h, (hipError_t)vigo::launch_corridor_check2(h->stream, h->grid, S, deg, coeffs, n_samp, delT, box, map_res, out_flag,
                                                         out_first, out_count, todo, clock_ws));
    return VIGO_OK;
}

int vigo_traj_corridor_check(vigo_handle_t h, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                             const double* knots, const double* delT, const double* endpoint, const double box[3], double map_res,
                             int flags, int32_t* out_status, int32_t* out_n, uint8_t* out_flag, int32_t* out_first,
                             int32_t* out_count, uint8_t* out_seg) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (T < 0 || S < 0 || deg < 0 || deg > 15 || !box || !(map_res > 0) || (flags & ~VIGO_TRAJ_NONFINITE_COLLIDES) ||
        (T > 0 && (!seg_off || !knots || !delT || !endpoint || !out_status || !out_n || !out_flag || !out_first)) ||
        (S > 0 && (!coeffs || !out_seg)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_corridor_check: bad argument");
    if (!sweep_box_ok(box, map_res)) return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_traj_corridor_check: collision box not finite or more than 32768 lattice points per pose");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_traj_corridor_check before vigo_set_grid");
    if (!key_lattice_ok(h->grid)) return fail(h, VIGO_ERR_UNSUPPORTED, kKeyLatticeMsg);
    if (T == 0 && S == 0) return VIGO_OK;
    int chunk;
    VIGO_TRY(traj_scratch(h, T, S, &chunk));
    VIGO_HIP(h, (hipError_t)vigo::launch_traj_corridor(h->stream, h->grid, T, S, deg, seg_off, coeffs, knots, delT, endpoint, box,
                                                       map_res, (flags & VIGO_TRAJ_NONFINITE_COLLIDES) ? 1 : 0, out_status, out_n,
                                                       out_flag, out_first, out_count, out_seg, h->buf[vigo::kBufScratch].ptr, chunk));
    return VIGO_OK;
}

int vigo_traj_point_check(vigo_handle_t h, int T, int S, int deg, const int32_t* seg_off, const double* coeffs,
                          const double* knots, const double* delT, const double* endpoint, int32_t* out_status, int32_t* out_n,
                          uint8_t* out_flag, int32_t* out_first, int32_t* out_count, uint8_t* out_seg) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (T < 0 || S < 0 || deg < 0 || deg > 15 ||
        (T > 0 && (!seg_off || !knots || !delT || !endpoint || !out_status || !out_n || !out_flag || !out_first)) ||
        (S > 0 && (!coeffs || !out_seg)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_traj_point_check: bad argument");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_traj_point_check before vigo_set_grid");
    if (T == 0 && S == 0) return VIGO_OK;
    int chunk;
    VIGO_TRY(traj_scratch(h, T, S, &chunk));
    VIGO_HIP(h, (hipError_t)vigo::launch_traj_point(h->stream, h->grid, T, S, deg, seg_off, coeffs, knots, delT, endpoint, out_status,
                                                    out_n, out_flag, out_first, out_count, out_seg, h->buf[vigo::kBufScratch].ptr, chunk));
    return VIGO_OK;
}

/* ---- seed paths (vigo_seed_core.hpp) ------------------------------------------------------ */

namespace {
bool seed_args_ok(int T, int S, int deg, const int32_t* seg_off, const double* coeffs, const double* knots, const double* duration,
                  const double* dt0, const double* cpd, const double* max_len, const double* prev_seed, const double* prev_fit,
                  int max_tries, int point_cap, const int32_t* out_status, const int32_t* out_tries, const double* out_dt,
                  const double* out_final_time, const int32_t* out_seed_n, const double* out_seed, const int32_t* out_fit_n,
                  const double* out_fit, const double* out_prev_seed, const double* out_prev_fit) {
    if (T < 0 || S < 0 || deg < 0 || deg > vigo::kSeedMaxDeg || max_tries < 1 || point_cap < 0) return false;
    if (T > 0 && (!seg_off || !knots || !duration || !dt0 || !cpd || !max_len || !prev_seed || !prev_fit || !out_status || !out_tries ||
                  !out_dt || !out_final_time || !out_seed_n || !out_fit_n || !out_prev_seed || !out_prev_fit))
        return false;
    if (T > 0 && point_cap > 0 && (!out_seed || !out_fit)) return false;
    return !(T > 0 && S > 0 && !coeffs);
}
}  // namespace

int vigo_seed_capacity(int32_t* max_samples) {
    if (!max_samples) return VIGO_ERR_INVALID_ARG;
    *max_samples = vigo::kSeedCapacity;
    return VIGO_OK;
}

int vigo_seed_paths(vigo_handle_t h, int T, int S, int deg, const int32_t* seg_off, const double* coeffs, const double* knots,
                    const double* duration, const double* dt0, const double* control_point_distance,
                    const double* max_path_length, const double* prev_in_seed, const double* prev_in_fit, int max_tries,
                    int point_cap, int32_t* out_status, int32_t* out_tries, double* out_dt, double* out_final_time,
                    int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit, double* out_prev_seed,
                    double* out_prev_fit) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (!seed_args_ok(T, S, deg, seg_off, coeffs, knots, duration, dt0, control_point_distance, max_path_length, prev_in_seed, prev_in_fit,
                      max_tries, point_cap, out_status, out_tries, out_dt, out_final_time, out_seed_n, out_seed, out_fit_n, out_fit,
                      out_prev_seed, out_prev_fit))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_seed_paths: bad argument");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_seed_paths before vigo_set_grid");
    if (T == 0) return VIGO_OK;
    VIGO_HIP(h, (hipError_t)vigo::launch_seed_paths(h->stream, h->grid, T, S, deg, seg_off, coeffs, knots, duration, dt0,
                                                    control_point_distance, max_path_length, prev_in_seed, prev_in_fit, max_tries,
                                                    point_cap, out_status, out_tries, out_dt, out_final_time, out_seed_n, out_seed,
                                                    out_fit_n, out_fit, out_prev_seed, out_prev_fit));
    return VIGO_OK;
}

int vigo_seed_paths_host(int nx, int ny, int nz, const double origin[3], double res, const uint8_t* voxels_host, int pow_mode,
                         int cap, int T, int S, int deg, const int32_t* seg_off, const double* coeffs, const double* knots,
                         const double* duration, const double* dt0, const double* control_point_distance,
                         const double* max_path_length, const double* prev_in_seed, const double* prev_in_fit, int max_tries,
                         int point_cap, int32_t* out_status, int32_t* out_tries, double* out_dt, double* out_final_time,
                         int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit, double* out_prev_seed,
                         double* out_prev_fit) {
    if (nx < 1 || ny < 1 || nz < 1 || !origin || !voxels_host || !(res > 0) || !vigo::seed_finite(res) || (pow_mode != 0 && pow_mode != 1) ||
        !seed_args_ok(T, S, deg, seg_off, coeffs, knots, duration, dt0, control_point_distance, max_path_length, prev_in_seed, prev_in_fit,
                      max_tries, point_cap, out_status, out_tries, out_dt, out_final_time, out_seed_n, out_seed, out_fit_n, out_fit,
                      out_prev_seed, out_prev_fit))
        return VIGO_ERR_INVALID_ARG;
    if (cap <= 0) cap = vigo::kSeedCapacity;
    const vigo::SeedByteGrid occ{voxels_host, nx, ny, nz, {origin[0], origin[1], origin[2]}, res};
    std::vector<double> pts(3 * ((size_t)cap + 1)), step((size_t)cap), dist((size_t)cap), seed(3 * (size_t)point_cap + 3), fit(3 * (size_t)point_cap + 3);
    std::vector<uint8_t> line((size_t)cap);
    for (int t = 0; t < T; ++t) {
        const int a = seg_off[t], b = seg_off[t + 1];
        if (a < 0 || b < a || b > S) {
            out_status[t] = vigo::kSeedBadInput;
            out_tries[t] = 0; out_dt[t] = dt0[t]; out_final_time[t] = 0.0; out_seed_n[t] = 0; out_fit_n[t] = 0;
            out_prev_seed[t] = prev_in_seed[t]; out_prev_fit[t] = prev_in_fit[t];
            continue;
        }
        vigo::SeedIn in;
        in.K = b - a; in.deg = deg;
        in.knots = knots + (size_t)a + t;
        in.coeffs = coeffs + (size_t)a * 3 * (deg + 1);
        in.duration = duration[t]; in.dt0 = dt0[t];
        in.control_point_distance = control_point_distance[t]; in.max_path_length = max_path_length[t];
        in.prev_seed = prev_in_seed[t]; in.prev_fit = prev_in_fit[t];
        in.max_tries = max_tries; in.point_cap = point_cap;
        vigo::SeedOut o;
        if (pow_mode == 0) vigo::seed_one(in, occ, res, vigo::SeedPowExact{}, cap, pts.data(), step.data(), dist.data(), line.data(), &o, seed.data(), fit.data());
        else vigo::seed_one(in, occ, res, vigo::SeedPowLibm{}, cap, pts.data(), step.data(), dist.data(), line.data(), &o, seed.data(), fit.data());
        out_status[t] = o.status;
        if (o.status == vigo::kSeedDeferred) continue;
        out_tries[t] = o.tries; out_dt[t] = o.dt; out_final_time[t] = o.final_time;
        out_seed_n[t] = o.seed_n; out_fit_n[t] = o.fit_n;
        out_prev_seed[t] = o.prev_seed; out_prev_fit[t] = o.prev_fit;
        if (o.seed_n > 0) memcpy(out_seed + (size_t)t * point_cap * 3, seed.data(), sizeof(double) * 3 * (size_t)o.seed_n);
        if (o.fit_n > 0) memcpy(out_fit + (size_t)t * point_cap * 3, fit.data(), sizeof(double) * 3 * (size_t)o.fit_n);
    }
    return VIGO_OK;
}

int vigo_poly_sample(vigo_handle_t h, int S, int deg, const double* coeffs, const int32_t* n_samp, const double* delT,
                     int stride, double* out_pos, float* out_pos_f32) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (S < 0 || deg < 0 || deg > 15 || stride < 0 || (S > 0 && stride > 0 && (!coeffs || !n_samp || !delT || (!out_pos && !out_pos_f32))))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_poly_sample: bad argument");
    VIGO_HIP(h, (hipError_t)vigo::launch_poly_sample(h->stream, S, deg, coeffs, n_samp, delT, stride, out_pos, out_pos_f32));
    return VIGO_OK;
}

int vigo_box_collision_points(vigo_handle_t h, int64_t M, const double* pts, const double box[3], double map_res, uint8_t* out) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (M < 0 || !box || !(map_res > 0) || (M > 0 && (!pts || !out))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_box_collision_points: bad argument");
    if (!sweep_box_ok(box, map_res)) return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_box_collision_points: collision box not finite or more than 32768 lattice points per pose");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_box_collision_points before vigo_set_grid");
    if (!key_lattice_ok(h->grid)) return fail(h, VIGO_ERR_UNSUPPORTED, kKeyLatticeMsg);
    VIGO_HIP(h, (hipError_t)vigo::launch_box_points(h->stream, h->grid, M, pts, box, map_res, out));
    return VIGO_OK;
}

int vigo_astar_search(vigo_handle_t h, int Q, const double* start, const double* end, double step, const int32_t pool[3],
                      double min_height, double max_height, int max_expansions, int path_cap, int32_t* out_status, int32_t* out_len,
                      double* out_path, int32_t* out_stats) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (Q < 0 || !astar_args_ok(pool, step, path_cap, max_expansions) ||
        (Q > 0 && (!start || !end || !out_status || !out_len || !out_path)))
        return fail(h, VIGO_ERR_INVALID_ARG, "vigo_astar_search: bad argument");
    if (!astar_pool_fits(pool))
        return fail(h, VIGO_ERR_UNSUPPORTED, "vigo_astar_search: more than VIGO_ASTAR_MAX_POOL_AXIS nodes along a pool axis");
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, "vigo_astar_search before vigo_set_grid");
    if (Q == 0) return VIGO_OK;
    VIGO_HIP(h, (hipError_t)vigo::launch_astar(h->stream, h->grid, Q, start, end, step, pool, min_height, max_height, max_expansions, path_cap,
                                               out_status, out_len, out_path, out_stats, h->launch));
    return VIGO_OK;
}
int vigo_astar_capacity(int32_t* max_nodes, int32_t* max_heap) {
    if (max_nodes) *max_nodes = vigo::astar_max_nodes();
    if (max_heap) *max_heap = vigo::astar_max_heap();
    return VIGO_OK;
}

}  // extern "C"

namespace {

// what a *_mixed prologue entry checks before its uniform body: the handle, the counts' pointer, the row stride
int check_mixed_rows(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const char* who) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B > 0 && !n_pts) return fail(h, VIGO_ERR_INVALID_ARG, (std::string(who) + ": n_pts == NULL").c_str());
    if (Ns < 7 || Ns > VIGO_MAX_CTRL_POINTS) return fail(h, VIGO_ERR_UNSUPPORTED_N, (std::string(who) + ": Ns outside [7, VIGO_MAX_CTRL_POINTS]").c_str());
    return VIGO_OK;
}

// vigo_guide_assign (n_pts == NULL) and vigo_guide_assign_mixed (rows of N control points, n_pts[b] of them the trajectory's)
int guide_assign(vigo_handle_t h, const std::string& who, int B, int N, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off,
                 const int32_t* seg, const int32_t* path_off, const double* path, int64_t pair_cap, int32_t* out_guide_off, double* out_guide_pv,
                 uint8_t* out_guide_unk, int32_t* out_status) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || N < 1 || pair_cap < 0 ||
        (B > 0 && (!ctrl || !seg_off || !seg || !path_off || !path || !out_guide_off || !out_guide_pv || !out_status)))
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": bad argument").c_str());
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, (who + " before vigo_set_grid").c_str());
    if (B == 0) return VIGO_OK;
    VIGO_TRY(ensure_scratch(h, 64));
    long long* result = h->buf[vigo::kBufScratch].as<long long>();
    VIGO_HIP(h, (hipError_t)vigo::launch_guide_offsets(h->stream, B, N, n_pts, seg_off, seg, path_off, (long long)pair_cap, out_guide_off,
                                                       out_status, result));
    long long host_result[2] = {0, 0};
    VIGO_TRY(read_back(h, host_result, result, sizeof(host_result)));
    if (host_result[1] != 0) return fail(h, VIGO_ERR_INVALID_ARG, (who + ": offsets that decrease, a path without a point or a segment out of range").c_str());
    if (host_result[0] > (long long)pair_cap || host_result[0] > 0x7fffffffLL)
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": the pairs do not fit pair_cap").c_str());
    VIGO_HIP(h, (hipError_t)vigo::launch_guide_assign(h->stream, h->grid, B, N, n_pts, ctrl, seg_off, seg, path_off, path, out_guide_off,
                                                      out_guide_pv, out_guide_unk, out_status));
    return VIGO_OK;
}

}  // namespace

extern "C" {

int vigo_guide_assign(vigo_handle_t h, int B, int N, const double* ctrl, const int32_t* seg_off, const int32_t* seg, const int32_t* path_off,
                      const double* path, int64_t pair_cap, int32_t* out_guide_off, double* out_guide_pv, uint8_t* out_guide_unk,
                      int32_t* out_status) {
    return guide_assign(h, "vigo_guide_assign", B, N, nullptr, ctrl, seg_off, seg, path_off, path, pair_cap, out_guide_off, out_guide_pv,
                        out_guide_unk, out_status);
}
int vigo_guide_assign_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off, const int32_t* seg,
                            const int32_t* path_off, const double* path, int64_t pair_cap, int32_t* out_guide_off, double* out_guide_pv,
                            uint8_t* out_guide_unk, int32_t* out_status) {
    VIGO_TRY(check_mixed_rows(h, B, Ns, n_pts, "vigo_guide_assign_mixed"));
    return guide_assign(h, "vigo_guide_assign_mixed", B, Ns, n_pts, ctrl, seg_off, seg, path_off, path, pair_cap, out_guide_off, out_guide_pv,
                        out_guide_unk, out_status);
}
int vigo_guide_capacity(int32_t* max_path_points) {
    if (max_path_points) *max_path_points = vigo::guide_path_capacity();
    return VIGO_OK;
}

}  // extern "C"

namespace {

// the per-trajectory scratch of vigo_collision_segs / vigo_path_search, carved out of the scratch buffer
int path_search_scratch(vigo_handle_t h, int B, int N, bool flags, vigo::PathSearchArgs& a) {
    return carve(h, vigo::kBufScratch, kSlack, [&](void* p) { return vigo::ws_path_search_scratch(p, B, N, flags, a); });
}

// flags and segment counts of the call, read back: result[0] segments, result[1] a bad list
int path_search_count(vigo_handle_t h, vigo::PathSearchArgs& a, long long result[2], const char* bad_list) {
    if (!a.seg_in)
        VIGO_HIP(h, (hipError_t)vigo::launch_ctrl_occupancy(h->stream, h->grid, a.B, a.N, a.ctrl, const_cast<uint8_t*>(a.pt), const_cast<uint8_t*>(a.ln)));
    VIGO_HIP(h, (hipError_t)vigo::launch_ps_count(h->stream, a));
    VIGO_TRY(read_back(h, result, a.result, 2 * sizeof(long long)));
    if (result[1] != 0) return fail(h, VIGO_ERR_INVALID_ARG, bad_list);
    return VIGO_OK;
}

// the searches of a call whose lists are counted (path_search_count): first choices, the retries the failures ask for,
// the walk; result[2..4] read back
int path_search_searches(vigo_handle_t h, vigo::PathSearchArgs& a, vigo::PathSearchWork& w, double step, const int32_t pool[3], double min_height,
                         double max_height, int max_expansions, long long result[5]) {
    const int search_path_cap = a.search_path_cap;
    const size_t S = (size_t)result[0];
    if (S > 0) {
        VIGO_TRY(carve(h, vigo::kBufPaths0, kSlack, [&](void* p) { return vigo::ws_first_searches(p, S, search_path_cap, w); }));
        VIGO_HIP(h, (hipError_t)vigo::launch_ps_fill(h->stream, a, w.seg, w.start1, w.end1));
        VIGO_HIP(h, (hipError_t)vigo::launch_astar(h->stream, h->grid, (int)S, w.start1, w.end1, step, pool, min_height, max_height, max_expansions,
                                                   search_path_cap, w.status1, w.len1, w.path1, nullptr, h->launch));
        VIGO_HIP(h, (hipError_t)vigo::launch_ps_retry(h->stream, a, w));
        VIGO_TRY(read_back(h, result + 2, a.result + 2, sizeof(long long)));
        const size_t Q2 = (size_t)result[2];
        if (Q2 > 0) {
            VIGO_TRY(carve(h, vigo::kBufPaths1, kSlack, [&](void* p) { return vigo::ws_second_searches(p, Q2, search_path_cap, w); }));
            VIGO_HIP(h, (hipError_t)vigo::launch_astar(h->stream, h->grid, (int)Q2, w.start2, w.end2, step, pool, min_height, max_height,
                                                       max_expansions, search_path_cap, w.status2, w.len2, w.path2, nullptr, h->launch));
        }
    }
    VIGO_HIP(h, (hipError_t)vigo::launch_ps_decide(h->stream, a, w));
    return read_back(h, result + 3, a.result + 3, 2 * sizeof(long long));
}

// the bodies of the uniform entries (n_pts == NULL) and of their _mixed forms (rows of N control points, n_pts[b] of them
// the trajectory's; check_mixed_rows has passed): the same checks, the same kernels, the same read-backs
int collision_segs(vigo_handle_t h, const std::string& who, int B, int N, const int32_t* n_pts, const double* ctrl, double not_check_ratio,
                   int32_t* out_seg_off, int32_t* out_seg, int64_t seg_cap, int32_t* out_status) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (B < 0 || N < 7 || seg_cap < 0 || !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0) ||
        (B > 0 && (!ctrl || !out_seg_off || !out_seg || !out_status)))
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": bad argument").c_str());
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, (who + " before vigo_set_grid").c_str());
    if (B == 0) return VIGO_OK;
    vigo::PathSearchArgs a{};
    a.B = B; a.N = N; a.n_pts = n_pts; a.ctrl = ctrl; a.not_check_ratio = not_check_ratio;
    VIGO_TRY(path_search_scratch(h, B, N, true, a));
    long long result[2] = {0, 0};
    VIGO_TRY(path_search_count(h, a, result, (who + ": bad list").c_str()));
    if (result[0] > (long long)seg_cap) return fail(h, VIGO_ERR_INVALID_ARG, (who + ": the segments do not fit seg_cap").c_str());
    a.out_seg_off = out_seg_off; a.out_status = out_status;
    VIGO_HIP(h, (hipError_t)vigo::launch_ps_fill(h->stream, a, out_seg, nullptr, nullptr));
    VIGO_HIP(h, (hipError_t)vigo::launch_ps_segs_out(h->stream, a));
    return VIGO_OK;
}

int path_search(vigo_handle_t h, const std::string& who, int B, int N, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off,
                const int32_t* seg, double not_check_ratio, double step, const int32_t pool[3], double min_height, double max_height,
                int max_expansions, int search_path_cap, int64_t seg_cap, int64_t point_cap, int32_t* out_status, int32_t* out_seg_off,
                int32_t* out_seg, int32_t* out_path_off, double* out_path, int32_t* out_counts) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    const bool scan = !seg_off && !seg;
    if (B < 0 || N < 7 || seg_cap < 0 || point_cap < 0 || (!scan && (!seg_off || !seg)) ||
        (scan && !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0)) || !astar_args_ok(pool, step, search_path_cap, max_expansions) ||
        (B > 0 && (!ctrl || !out_status || !out_seg_off || !out_seg || !out_path_off || !out_path)))
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": bad argument").c_str());
    if (!astar_pool_fits(pool))
        return fail(h, VIGO_ERR_UNSUPPORTED, (who + ": more than VIGO_ASTAR_MAX_POOL_AXIS nodes along a pool axis").c_str());
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, (who + " before vigo_set_grid").c_str());
    if (B == 0) return VIGO_OK;
    vigo::PathSearchArgs a{};
    a.B = B; a.N = N; a.n_pts = n_pts; a.ctrl = ctrl; a.not_check_ratio = not_check_ratio; a.seg_off_in = seg_off; a.seg_in = seg;
    a.search_path_cap = search_path_cap;
    VIGO_TRY(path_search_scratch(h, B, N, scan, a));
    long long result[5] = {0, 0, 0, 0, 0};
    VIGO_TRY(path_search_count(h, a, result, (who + ": offsets that decrease or start below 0, or a segment end outside [0, N)").c_str()));
    vigo::PathSearchWork w{};
    VIGO_TRY(path_search_searches(h, a, w, step, pool, min_height, max_height, max_expansions, result));
    if (result[3] > (long long)seg_cap || result[3] >= 0x7fffffffLL)
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": the segments do not fit seg_cap").c_str());
    if (result[4] > (long long)point_cap || result[4] > 0x7fffffffLL)
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": the path points do not fit point_cap").c_str());
    a.out_status = out_status; a.out_seg_off = out_seg_off; a.out_seg = out_seg; a.out_path_off = out_path_off; a.out_path = out_path;
    a.out_counts = out_counts;
    VIGO_HIP(h, (hipError_t)vigo::launch_ps_write(h->stream, a, w, (int)result[3], (int)result[4]));
    return VIGO_OK;
}

int rebound_reguide(vigo_handle_t h, const std::string& who, int B, int N, const int32_t* n_pts, const double* ctrl, const int32_t* guide_off,
                    const double* guide_pv, const uint8_t* guide_unk, double* weights, double not_check_ratio, double step, const int32_t pool[3],
                    double min_height, double max_height, int max_expansions, int search_path_cap, vigo_rebound_state_t* state,
                    int64_t pair_cap, int32_t* out_guide_off, double* out_guide_pv, uint8_t* out_guide_unk, int64_t seg_cap,
                    int64_t point_cap, int32_t* out_path_seg_off, int32_t* out_path_off, double* out_path, int32_t* out_status) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    const bool no_guides = !guide_off && !guide_pv && !guide_unk;
    const bool no_paths = !out_path_seg_off && !out_path_off && !out_path;
    if (B < 0 || N < 7 || pair_cap < 0 || seg_cap < 0 || point_cap < 0 || !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0) ||
        (!no_guides && (!guide_off || !guide_pv)) || (!no_paths && (!out_path_seg_off || !out_path_off || !out_path)) ||
        !astar_args_ok(pool, step, search_path_cap, max_expansions) ||
        (B > 0 && (!ctrl || !weights || !state || !out_guide_off || !out_guide_pv || !out_status)))
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": bad argument").c_str());
    if (N > VIGO_MAX_CTRL_POINTS) return fail(h, VIGO_ERR_UNSUPPORTED_N, "N outside [7, VIGO_MAX_CTRL_POINTS]");
    if (!astar_pool_fits(pool))
        return fail(h, VIGO_ERR_UNSUPPORTED, (who + ": more than VIGO_ASTAR_MAX_POOL_AXIS nodes along a pool axis").c_str());
    if (B > (1 << 20)) return fail(h, VIGO_ERR_UNSUPPORTED, (who + ": more than 2^20 trajectories in a call").c_str());
    if (!h->has_grid) return fail(h, VIGO_ERR_NO_GRID, (who + " before vigo_set_grid").c_str());
    if (B == 0) return VIGO_OK;
    constexpr int kSegs = VIGO_MAX_COLLISION_SEGS;
    vigo::ReguideArgs r{};
    vigo::ReguideStage st{};
    VIGO_TRY(carve(h, vigo::kBufReguide0, kSlack, [&](void* p) { return vigo::ws_reguide(p, B, N, kSegs, r, st); }));
    r.B = B; r.N = N; r.n_pts = n_pts; r.ctrl = ctrl; r.guide_off = guide_off; r.guide_pv = guide_pv; r.guide_unk = guide_unk; r.weights = weights; r.state = state;
    r.dthresh = h->params.dthresh; r.not_check_ratio = not_check_ratio;
    // vigo_path_search's chain on the lists (a trajectory that is not worked on has an empty one)
    vigo::PathSearchArgs a{};
    a.B = B; a.N = N; a.n_pts = n_pts; a.ctrl = ctrl; a.not_check_ratio = not_check_ratio; a.seg_in = r.list; a.seg_cnt_in = r.n_list; a.seg_stride_in = kSegs;
    a.search_path_cap = search_path_cap;
    VIGO_TRY(path_search_scratch(h, B, N, false, a));
    VIGO_HIP(h, hipMemsetAsync(r.result, 0, 64, h->stream));
    VIGO_HIP(h, (hipError_t)vigo::launch_reguide_list(h->stream, h->grid, r));
    long long bad_off = 0;
    VIGO_HIP(h, hipMemcpyAsync(&bad_off, r.result, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    long long result[5] = {0, 0, 0, 0, 0};
    const int rc = path_search_count(h, a, result, (who + ": a re-guide list out of range").c_str());
    if (rc == VIGO_ERR_HIP) (void)hipStreamSynchronize(h->stream);   // (it may have failed before its own wait: bad_off's copy must have landed)
    if (rc) return rc;
    if (bad_off != 0) return fail(h, VIGO_ERR_INVALID_ARG, (who + ": guide offsets that decrease or start below 0").c_str());
    vigo::PathSearchWork w{};
    VIGO_TRY(path_search_searches(h, a, w, step, pool, min_height, max_height, max_expansions, result));
    const long long total_seg = result[3], total_pts = result[4];
    if (total_pts > 0x7fffffffLL) return fail(h, VIGO_ERR_INVALID_ARG, (who + ": more than 2^31 path points").c_str());
    if (!no_paths && (total_seg > (long long)seg_cap || total_pts > (long long)point_cap))
        return fail(h, VIGO_ERR_INVALID_ARG, (who + ": the paths do not fit seg_cap / point_cap").c_str());
    VIGO_TRY(carve(h, vigo::kBufReguide1, kSlack, [&](void* p) { return vigo::ws_reguide_paths(p, total_seg, total_pts, a); }));
    a.out_status = st.ps_status; a.out_seg_off = st.ps_seg_off; a.out_counts = st.ps_counts;
    VIGO_HIP(h, (hipError_t)vigo::launch_ps_write(h->stream, a, w, (int)total_seg, (int)total_pts));
    // vigo_guide_assign's pair on that output: the pairs THIS step appends
    long long* g_result = r.result + 2;
    VIGO_HIP(h, (hipError_t)vigo::launch_guide_offsets(h->stream, B, N, n_pts, st.ps_seg_off, a.out_seg, a.out_path_off, 0x7fffffffLL, st.g_off, st.g_status, g_result));
    long long g_host[2] = {0, 0};
    VIGO_TRY(read_back(h, g_host, g_result, sizeof(g_host)));
    if (g_host[1] != 0 || g_host[0] > 0x7fffffffLL) return fail(h, VIGO_ERR_HIP, (who + ": the path search's output is no input of the guide step").c_str());
    const size_t P = (size_t)g_host[0];
    double* g_pv;
    uint8_t* g_unk;
    VIGO_TRY(carve(h, vigo::kBufReguide2, kSlack, [&](void* p) { return vigo::ws_reguide_pairs(p, P, g_pv, g_unk); }));
    VIGO_HIP(h, (hipError_t)vigo::launch_guide_assign(h->stream, h->grid, B, N, n_pts, ctrl, st.ps_seg_off, a.out_seg, a.out_path_off, a.out_path, st.g_off, g_pv, g_unk, st.g_status));
    r.ps_status = st.ps_status; r.ps_seg_off = st.ps_seg_off; r.ps_counts = st.ps_counts; r.g_status = st.g_status; r.g_off = st.g_off; r.g_pv = g_pv; r.g_unk = g_unk;
    r.pair_cap = (long long)pair_cap;
    r.out_guide_off = out_guide_off; r.out_guide_pv = out_guide_pv; r.out_guide_unk = out_guide_unk; r.out_status = out_status;
    VIGO_HIP(h, (hipError_t)vigo::launch_guide_merge_offsets(h->stream, r));
    long long merged = 0;
    VIGO_TRY(read_back(h, &merged, r.result + 1, sizeof(long long)));
    if (merged > (long long)pair_cap || merged > 0x7fffffffLL) return fail(h, VIGO_ERR_INVALID_ARG, (who + ": the merged pairs do not fit pair_cap").c_str());
    VIGO_HIP(h, (hipError_t)vigo::launch_guide_merge(h->stream, h->grid, r));
    if (!no_paths) {
        VIGO_HIP(h, hipMemcpyAsync(out_path_seg_off, st.ps_seg_off, ((size_t)B + 1) * 4, hipMemcpyDeviceToDevice, h->stream));
        VIGO_HIP(h, hipMemcpyAsync(out_path_off, a.out_path_off, ((size_t)total_seg + 1) * 4, hipMemcpyDeviceToDevice, h->stream));
        if (total_pts > 0) VIGO_HIP(h, hipMemcpyAsync(out_path, a.out_path, (size_t)total_pts * 24, hipMemcpyDeviceToDevice, h->stream));
    }
    VIGO_HIP(h, (hipError_t)vigo::launch_reguide_commit(h->stream, r));
    return VIGO_OK;
}

}  // namespace

extern "C" {

int vigo_collision_segs(vigo_handle_t h, int B, int N, const double* ctrl, double not_check_ratio, int32_t* out_seg_off, int32_t* out_seg,
                        int64_t seg_cap, int32_t* out_status) {
    return collision_segs(h, "vigo_collision_segs", B, N, nullptr, ctrl, not_check_ratio, out_seg_off, out_seg, seg_cap, out_status);
}
int vigo_collision_segs_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, double not_check_ratio,
                              int32_t* out_seg_off, int32_t* out_seg, int64_t seg_cap, int32_t* out_status) {
    VIGO_TRY(check_mixed_rows(h, B, Ns, n_pts, "vigo_collision_segs_mixed"));
    return collision_segs(h, "vigo_collision_segs_mixed", B, Ns, n_pts, ctrl, not_check_ratio, out_seg_off, out_seg, seg_cap, out_status);
}

int vigo_path_search(vigo_handle_t h, int B, int N, const double* ctrl, const int32_t* seg_off, const int32_t* seg, double not_check_ratio,
                     double step, const int32_t pool[3], double min_height, double max_height, int max_expansions, int search_path_cap,
                     int64_t seg_cap, int64_t point_cap, int32_t* out_status, int32_t* out_seg_off, int32_t* out_seg, int32_t* out_path_off,
                     double* out_path, int32_t* out_counts) {
    return path_search(h, "vigo_path_search", B, N, nullptr, ctrl, seg_off, seg, not_check_ratio, step, pool, min_height, max_height,
                       max_expansions, search_path_cap, seg_cap, point_cap, out_status, out_seg_off, out_seg, out_path_off, out_path, out_counts);
}
int vigo_path_search_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const int32_t* seg_off, const int32_t* seg,
                           double not_check_ratio, double step, const int32_t pool[3], double min_height, double max_height, int max_expansions,
                           int search_path_cap, int64_t seg_cap, int64_t point_cap, int32_t* out_status, int32_t* out_seg_off, int32_t* out_seg,
                           int32_t* out_path_off, double* out_path, int32_t* out_counts) {
    VIGO_TRY(check_mixed_rows(h, B, Ns, n_pts, "vigo_path_search_mixed"));
    return path_search(h, "vigo_path_search_mixed", B, Ns, n_pts, ctrl, seg_off, seg, not_check_ratio, step, pool, min_height, max_height,
                       max_expansions, search_path_cap, seg_cap, point_cap, out_status, out_seg_off, out_seg, out_path_off, out_path, out_counts);
}

int vigo_rebound_reguide(vigo_handle_t h, int B, int N, const double* ctrl, const int32_t* guide_off, const double* guide_pv,
                         const uint8_t* guide_unk, double* weights, double not_check_ratio, double step, const int32_t pool[3],
                         double min_height, double max_height, int max_expansions, int search_path_cap, vigo_rebound_state_t* state,
                         int64_t pair_cap, int32_t* out_guide_off, double* out_guide_pv, uint8_t* out_guide_unk, int64_t seg_cap,
                         int64_t point_cap, int32_t* out_path_seg_off, int32_t* out_path_off, double* out_path, int32_t* out_status) {
    return rebound_reguide(h, "vigo_rebound_reguide", B, N, nullptr, ctrl, guide_off, guide_pv, guide_unk, weights, not_check_ratio, step, pool,
                           min_height, max_height, max_expansions, search_path_cap, state, pair_cap, out_guide_off, out_guide_pv, out_guide_unk,
                           seg_cap, point_cap, out_path_seg_off, out_path_off, out_path, out_status);
}
int vigo_rebound_reguide_mixed(vigo_handle_t h, int B, int Ns, const int32_t* n_pts, const double* ctrl, const int32_t* guide_off,
                               const double* guide_pv, const uint8_t* guide_unk, double* weights, double not_check_ratio, double step,
                               const int32_t pool[3], double min_height, double max_height, int max_expansions, int search_path_cap,
                               vigo_rebound_state_t* state, int64_t pair_cap, int32_t* out_guide_off, double* out_guide_pv,
                               uint8_t* out_guide_unk, int64_t seg_cap, int64_t point_cap, int32_t* out_path_seg_off, int32_t* out_path_off,
                               double* out_path, int32_t* out_status) {
    VIGO_TRY(check_mixed_rows(h, B, Ns, n_pts, "vigo_rebound_reguide_mixed"));
    return rebound_reguide(h, "vigo_rebound_reguide_mixed", B, Ns, n_pts, ctrl, guide_off, guide_pv, guide_unk, weights, not_check_ratio, step,
                           pool, min_height, max_height, max_expansions, search_path_cap, state, pair_cap, out_guide_off, out_guide_pv,
                           out_guide_unk, seg_cap, point_cap, out_path_seg_off, out_path_off, out_path, out_status);
}

/* ---- ESDF ----------------------------------------------------------------------------------- */

int vigo_set_esdf(vigo_handle_t h, int nx, int ny, int nz, const double origin[3], double res, const float* dist_dev) {
    if (!h || !dist_dev || !origin || nx < 2 || ny < 2 || nz < 2 || !geometry_ok(origin, res)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_set_esdf: bad argument");
    if ((long long)nx * ny * nz > (1LL << 33)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_set_esdf: lattice too large");
    end_esdf_tracking(h);
    return install_esdf(h, nx, ny, nz, origin, res, dist_dev);
}

int vigo_build_esdf(vigo_handle_t h, int plane, int unknown_is_site, float* out_lattice_dev) {
    VIGO_TRY(check_esdf_build(h, "vigo_build_esdf", plane));
    end_esdf_tracking(h);
    const GridView& g = h->grid;
    const size_t voxels = (size_t)g.nx * g.ny * g.nz;
    int32_t *a, *b;
    VIGO_TRY(carve(h, vigo::kBufEsdfWs, kExact, [&](void* p) { return vigo::ws_pair(p, voxels, a, b); }));   // = esdf_build_ws_bytes(): 1 GiB at 512^3
    float* lattice = out_lattice_dev ? out_lattice_dev : reinterpret_cast<float*>(a);
    VIGO_HIP(h, (hipError_t)vigo::launch_esdf_build(h->stream, g, plane, unknown_is_site != 0, a, b, lattice));
    return install_esdf(h, g.nx, g.ny, g.nz, g.origin, g.res, lattice);
}

int vigo_build_esdf_tracked(vigo_handle_t h, int plane, int unknown_is_site, float* out_lattice_dev) {
    VIGO_TRY(check_esdf_build(h, "vigo_build_esdf_tracked", plane));
    end_esdf_tracking(h);                                         // until everything below is in place
    const GridView& g = h->grid;
    const size_t voxels = (size_t)g.nx * g.ny * g.nz;
    vigo::EsdfTrackWs& w = h->esdf_track;
    VIGO_TRY(carve(h, vigo::kBufEsdfTrack, kExact,
                   [&](void* p) { return vigo::ws_esdf_track(p, voxels, (size_t)g.nx * g.nz, (size_t)g.ny * g.nz, w); }));
    VIGO_HIP(h, (hipError_t)vigo::launch_esdf_build(h->stream, g, plane, unknown_is_site != 0, w.a, w.b, w.lattice));
    if (out_lattice_dev) VIGO_HIP(h, hipMemcpyAsync(out_lattice_dev, w.lattice, voxels * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    VIGO_TRY(install_esdf(h, g.nx, g.ny, g.nz, g.origin, g.res, w.lattice));
    h->esdf_tracking = true;
    h->esdf_track_plane = plane;
    h->esdf_track_unknown = unknown_is_site != 0;
    return VIGO_OK;
}

int vigo_update_esdf(vigo_handle_t h, float* out_lattice_dev, vigo_esdf_update_stats_t* stats) {
    if (!h) return VIGO_ERR_INVALID_ARG;
    if (!h->esdf_tracking) return fail(h, VIGO_ERR_NO_GRID, "vigo_update_esdf: the handle is not tracking (no vigo_build_esdf_tracked since the last whole-snapshot call, vigo_build_esdf or vigo_set_esdf)");
    const GridView& g = h->grid;
    const vigo::EsdfTrackWs& w = h->esdf_track;
    if (stats) *stats = vigo_esdf_update_stats_t{};
    const bool pending = h->esdf_pending_n[0] != 0;
    if (pending) {
        if (stats)
            for (int a = 0; a < 3; ++a) { stats->box_lo[a] = h->esdf_pending_lo[a]; stats->box_n[a] = h->esdf_pending_n[a]; }
        VIGO_HIP(h, (hipError_t)vigo::launch_esdf_region_update(h->stream, g, h->esdf_pending_lo, h->esdf_pending_n, h->esdf_track_plane,
                                                                h->esdf_track_unknown, w, h->buf[vigo::kBufEsdf].as<float>(), stats != nullptr));
        for (int a = 0; a < 3; ++a) h->esdf_pending_lo[a] = h->esdf_pending_n[a] = 0;
    }
    if (out_lattice_dev)
        VIGO_HIP(h, hipMemcpyAsync(out_lattice_dev, w.lattice, (size_t)g.nx * g.ny * g.nz * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (stats && pending) {
        unsigned long long counts[2];
        VIGO_TRY(read_back(h, counts, w.counters, sizeof counts));
        stats->y_lines = (int64_t)counts[0];
        stats->x_lines = (int64_t)counts[1];
    }
    return VIGO_OK;
}

int vigo_esdf_from_voxels_host(int nx, int ny, int nz, const uint8_t* voxels_host, int plane, int unknown_is_site, double res,
                               float* out_lattice_host) {
    return vigo::esdf_from_voxels(nx, ny, nz, voxels_host, plane, unknown_is_site, res, out_lattice_host);
}

int vigo_esdf_from_voxels_host_tracked(int nx, int ny, int nz, const uint8_t* voxels_host, int plane, int unknown_is_site, double res,
                                       int32_t* a_out, int32_t* b_out, float* out_lattice_host) {
    return vigo::esdf_from_voxels_tracked(nx, ny, nz, voxels_host, plane, unknown_is_site, res, a_out, b_out, out_lattice_host);
}

int vigo_esdf_update_host(int nx, int ny, int nz, const uint8_t* new_voxels_host, int plane, int unknown_is_site, double res,
                          const int32_t lo[3], const int32_t n[3], int32_t* a_inout, int32_t* b_inout, float* lattice_inout,
                          vigo_esdf_update_stats_t* stats) {
    int64_t y_lines = 0, x_lines = 0;
    const int rc = vigo::esdf_update(nx, ny, nz, new_voxels_host, plane, unknown_is_site, res, lo, n, a_inout, b_inout, lattice_inout,
                                     &y_lines, &x_lines);
    if (rc != 0 || !stats) return rc;
    *stats = vigo_esdf_update_stats_t{};
    if (n[0] != 0 && n[1] != 0 && n[2] != 0) {
        for (int a = 0; a < 3; ++a) { stats->box_lo[a] = lo[a]; stats->box_n[a] = n[a]; }
        stats->y_lines = y_lines;
        stats->x_lines = x_lines;
    }
    return rc;
}

int vigo_esdf_query(vigo_handle_t h, int64_t Q, const double* pts, double* out_dist, double* out_grad) {
    if (!h || Q < 0 || (Q > 0 && (!pts || !out_dist || !out_grad))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_esdf_query: bad argument");
    if (!h->has_esdf) return fail(h, VIGO_ERR_NO_GRID, "vigo_esdf_query before vigo_set_esdf");
    VIGO_HIP(h, (hipError_t)vigo::launch_esdf_query(h->stream, h->esdf_view, Q, pts, out_dist, out_grad));
    return VIGO_OK;
}

int vigo_esdf_query_f32(vigo_handle_t h, int64_t Q, const float* pts, float* out_dist_grad) {
    if (!h || Q < 0 || (Q > 0 && (!pts || !out_dist_grad))) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_esdf_query_f32: bad argument");
    if (Q > 0 && (reinterpret_cast<uintptr_t>(out_dist_grad) & 15u)) return fail(h, VIGO_ERR_INVALID_ARG, "vigo_esdf_query_f32: out must be 16-byte aligned");
    if (!h->has_esdf) return fail(h, VIGO_ERR_NO_GRID, "vigo_esdf_query_f32 before vigo_set_esdf");
    VIGO_HIP(h, (hipError_t)vigo::launch_esdf_query_f32(h->stream, h->esdf_view, Q, pts, out_dist_grad));
    return VIGO_OK;
}

}  // extern "C"
