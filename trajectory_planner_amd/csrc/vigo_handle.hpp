// vigo_handle.hpp — what a vigo_handle_t points to.  Only vigo_api.cpp includes this: the handle is opaque to the kernel
// files and to everything above the ABI.
#pragma once

#include <string>

#include "vigo_esdf_core.hpp"
#include "vigo_internal.hpp"

namespace vigo {

// A grow-only device allocation.  reserve() (vigo_api.cpp) is the only code that allocates one, vigo_destroy's loop over
// vigo_context::buf the only code that frees one for good.
struct DevBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
};

// The handle's buffers, with what they grow to (reserve()'s callers) and what a growth invalidates:
enum BufId {
    kBufGrid,        // the packed voxel snapshot: exact size
    kBufEsdf,        // the bricked ESDF: exact size; growing drops has_esdf and esdf_view.dist until the new field is in
    kBufEsdfWs,      // vigo_build_esdf's two int32 buffers (vigo_esdf_build.hip): exact size (1 GiB at 512^3)
    kBufEsdfTrack,   // vigo_build_esdf_tracked's A, B, lattice, counts and flags (ws_esdf_track): exact size, 12 bytes per voxel
                     //   and the flags (1.5 GiB at 512^3); a failed growth ends the tracking
    kBufFit,         // least-squares operator of the B-spline fit, transposed (vigo_fit.hip): exact size; growing clears fit_K
    kBufFitTable,    // the operators of K = 4 .. 62 at one ts for vigo_bspline_fit_mixed (vigo_fit_plan.hpp): exact size, 0.7 MB;
                     //   a slot of its own, so filling it leaves kBufFit's operator and every other cache alone
    kBufTimes,       // the gates' sample clock: T + 64 doubles; growing clears times_T
    kBufFinishTs,    // vigo_traj_finish's two clocks (the `t += ts` one and the `t += sample_dt` one), slots of their own so
    kBufFinishDt,    //   the gates' table stays cached: T + 64 doubles; growing clears the slot's finish_clock[].T
    kBufValidateClock,  // vigo_traj_validate's clock, a slot of its own like the two above: T + 64 doubles; growing clears
                        //   validate_clock.T
    kBufValidateTab, // vigo_traj_validate's per-count tables: kValidateSlots * validate_tab_entries(VIGO_MAX_CTRL_POINTS) int32, fixed
    kBufScratch,     // per-call scratch of most entry points and staging of the *_host calls: need + 25 % + 4 KiB
    kBufPaths0,      // vigo_path_search: sized by the call's first-choice and (kBufPaths1) second-choice searches,
    kBufPaths1,      //   need + 25 % + 4 KiB
    kBufReguide0,    // vigo_rebound_reguide: per trajectory and control point, (1) the searches' segments and paths,
    kBufReguide1,    //   (2) the new pairs; need + 25 % + 4 KiB
    kBufReguide2,
    kBufRebound,     // vigo_rebound_rounds: flags + compacted indices, B + 16 int32 + 64 bytes (its own allocation: the
                     //   scratch buffer serves other entry points between the rounds' launches)
    kBufCount
};

}  // namespace vigo

// Everything an entry point keeps between calls.  Device memory is either fixed-size and made by vigo_create (dc_dev,
// dc_stage, the events) or one of buf[]; the caches below (grid, esdf_view, fit_*, times_*) describe what a buffer holds.
struct vigo_context {
    int device = 0;
    hipStream_t stream = nullptr;
    vigo_params_t params;
    vigo::DevConst dc;
    vigo::DevConst* dc_dev = nullptr;  // device copy, refreshed by vigo_set_params IN STREAM ORDER (see there)
    // pinned staging ring for those refreshes: slot i may be rewritten once dc_event[i] (its last copy) is done
    static constexpr int kDcSlots = 4;
    vigo::DevConst* dc_stage = nullptr;   // hipHostMalloc'ed [kDcSlots]
    hipEvent_t dc_event[kDcSlots] = {};
    int dc_next = 0;
    int precision = VIGO_PREC_F64;
    vigo::LaunchState launch;
    std::string last_error;
    vigo::DevBuffer buf[vigo::kBufCount];
    // voxel snapshot (kBufGrid)
    vigo::GridView grid{};
    bool has_grid = false;
    // esdf (kBufEsdf)
    vigo::EsdfView esdf_view{};
    bool has_esdf = false;
    // tracking (kBufEsdfTrack): from vigo_build_esdf_tracked until a whole-snapshot call, vigo_build_esdf or vigo_set_esdf.
    // esdf_track points into the buffer; the pending box is the bounding box of the region updates since the last
    // vigo_update_esdf, host integers, empty while an esdf_pending_n is 0
    bool esdf_tracking = false;
    int esdf_track_plane = 0, esdf_track_unknown = 0;
    vigo::EsdfTrackWs esdf_track{};
    int32_t esdf_pending_lo[3] = {}, esdf_pending_n[3] = {};
    // kBufFit holds the operator for (fit_K, fit_ts); fit_K == 0: none
    int fit_K = 0;
    double fit_ts = 0.0;
    // kBufFitTable holds the operators of every K at fit_table_ts; 0: none
    double fit_table_ts = 0.0;
    // kBufTimes holds the clock of (times_dt, times_tmax), filled on times_stream; times_T < 0: none
    double times_dt = -1.0, times_tmax = -1.0;
    int times_T = -1;
    hipStream_t times_stream = nullptr;
    // kBufFinishTs / kBufFinishDt hold the clock of (dt, tmax) — [0]: samples t < tmax, [1]: samples t <= tmax; T < 0: none
    struct ClockSlot {
        double dt = -1.0, tmax = -1.0;
        int T = -1;
        hipStream_t stream = nullptr;
    } finish_clock[2];
    // kBufValidateClock holds vigo_traj_validate's clock (samples t <= tmax)
    ClockSlot validate_clock;
    // vigo_traj_validate's {S, C} tables, one per key (dt, ts_ctrl, ratio, rule, Ns): slot i of kBufValidateTab is filled in
    // stream order from slot i of the pinned validate_stage, which may be rewritten once validate_event[i] (its copy) is done
    static constexpr int kValidateSlots = 4;
    struct ValidateKey {
        double dt = -1.0, ts_ctrl = -1.0, ratio = -1.0;
        int rule = -1, Ns = 0;                   // Ns == 0: the slot is empty
    } validate_key[kValidateSlots];
    int32_t* validate_stage = nullptr;           // hipHostMalloc'ed on first use, [kValidateSlots][validate_tab_entries(256)]
    hipEvent_t validate_event[kValidateSlots] = {};
    int validate_next = 0;
};
