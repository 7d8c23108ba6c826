// bsplineTrajBatch.cpp — trajPlanner::bsplineTraj::makePlanBatch: the split into pipelined parts, the prologue
// (BT.cpp:333-385, steps 1-3) and the rebound loops (BT.cpp:611-685) of many planners in lock-step, and the device stages
// they are made of, each one launch per group of planners through the C ABI of include/vigo.h.
#include <trajectory_planner/bsplineTraj.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../../csrc/vigo_guide_core.hpp"
#include "../../csrc/vigo_pathsearch_core.hpp"
#include "bsplineTrajBatch.h"

using std::cout;
using std::endl;

namespace trajPlanner {

namespace {
using vigo_host::Companion;
constexpr int kAstarPathCap = 128;   // path points a device search returns (a longer path is searched again by the host)

// ---- the process default and the process totals (bsplineTraj.h): all there is of process-wide state of the batch calls.
// The calls below touch it at their two ends only: the overloads without options copy the default, every call adds its
// stats when it returns.
std::mutex g_batchMutex;
bsplineTraj::BatchOptions g_batchDefaults;   // (g_batchMutex) kept normalized
bsplineTraj::BatchStats g_batchTotals;       // (g_batchMutex)

template <class Edit>
void editDefaults(Edit edit) {
    std::lock_guard<std::mutex> lock(g_batchMutex);
    edit(g_batchDefaults);
    g_batchDefaults = g_batchDefaults.normalized();
}
template <class T>
void put(T* out, T v) {
    if (out) *out = v;
}
}  // namespace

bsplineTraj::BatchOptions bsplineTraj::defaultBatchOptions() {
    std::lock_guard<std::mutex> lock(g_batchMutex);
    return g_batchDefaults;
}
bsplineTraj::BatchStats bsplineTraj::batchTotals() {
    std::lock_guard<std::mutex> lock(g_batchMutex);
    return g_batchTotals;
}
void reportBatchStats(const bsplineTraj::BatchStats& st, bsplineTraj::BatchStats* out) {
    put(out, st);
    std::lock_guard<std::mutex> lock(g_batchMutex);
    g_batchTotals += st;
}

void bsplineTraj::setDeviceAstar(bool on) { editDefaults([=](BatchOptions& o) { o.deviceAstar = on; }); }
void bsplineTraj::setDeviceAstarBudget(int maxExpansions) { editDefaults([=](BatchOptions& o) { o.deviceAstarBudget = maxExpansions; }); }
void bsplineTraj::setDeviceGuides(int mode) { editDefaults([=](BatchOptions& o) { o.deviceGuides = mode; }); }
void bsplineTraj::setDevicePrologue(bool on) { editDefaults([=](BatchOptions& o) { o.devicePrologue = on; }); }
void bsplineTraj::setDeviceReguide(int mode) { editDefaults([=](BatchOptions& o) { o.deviceReguide = mode; }); }
void bsplineTraj::setReguideStepLog(std::vector<ReguideStepRecord>* log) { editDefaults([=](BatchOptions& o) { o.reguideStepLog = log; }); }
void bsplineTraj::setDeviceResidentRebound(bool on) { editDefaults([=](BatchOptions& o) { o.deviceResidentRebound = on; }); }
void bsplineTraj::setMixedBatches(bool on) { editDefaults([=](BatchOptions& o) { o.mixedBatches = on; }); }
void bsplineTraj::setMixedPrologue(bool on) { editDefaults([=](BatchOptions& o) { o.mixedPrologue = on; }); }
void bsplineTraj::setDeviceEpilogue(bool on) { editDefaults([=](BatchOptions& o) { o.deviceEpilogue = on; }); }
void bsplineTraj::setBatchPipelineThreshold(size_t planners) { editDefaults([=](BatchOptions& o) { o.pipelineThreshold = planners; }); }
void bsplineTraj::setDeviceSeed(bool on) { editDefaults([=](BatchOptions& o) { o.deviceSeed = on; }); }
void bsplineTraj::setMixedFit(bool on) { editDefaults([=](BatchOptions& o) { o.mixedFit = on; }); }
void bsplineTraj::setSeedMaxTries(int n) { editDefaults([=](BatchOptions& o) { o.seedMaxTries = n; }); }
bool bsplineTraj::deviceAstar() { return defaultBatchOptions().deviceAstar; }
int bsplineTraj::deviceGuides() { return defaultBatchOptions().deviceGuides; }
bool bsplineTraj::devicePrologue() { return defaultBatchOptions().devicePrologue; }
int bsplineTraj::deviceReguide() { return defaultBatchOptions().deviceReguide; }
bool bsplineTraj::deviceResidentRebound() { return defaultBatchOptions().deviceResidentRebound; }
bool bsplineTraj::mixedBatches() { return defaultBatchOptions().mixedBatches; }
bool bsplineTraj::mixedPrologue() { return defaultBatchOptions().mixedPrologue; }
bool bsplineTraj::deviceEpilogue() { return defaultBatchOptions().deviceEpilogue; }
bool bsplineTraj::deviceSeed() { return defaultBatchOptions().deviceSeed; }
bool bsplineTraj::mixedFit() { return defaultBatchOptions().mixedFit; }
int bsplineTraj::seedMaxTries() { return defaultBatchOptions().seedMaxTries; }

void bsplineTraj::deviceAstarTotals(long long* deviceDecided, long long* hostRun, double* prologueSeconds) {
    const BatchStats t = batchTotals();
    put(deviceDecided, t.astarDecided), put(hostRun, t.astarHost), put(prologueSeconds, t.prologueSeconds);
}
void bsplineTraj::deviceGuideTotals(long long* deviceDecided, long long* hostRun) {
    const BatchStats t = batchTotals();
    put(deviceDecided, t.guidesDecided), put(hostRun, t.guidesHost);
}
void bsplineTraj::devicePrologueTotals(long long* deviceDecided, long long* hostRun, double* chainSeconds) {
    const BatchStats t = batchTotals();
    put(deviceDecided, t.prologueDecided), put(hostRun, t.prologueHost), put(chainSeconds, t.chainSeconds);
}
void bsplineTraj::deviceReguideTotals(long long* deviceDecided, long long* hostRun) {
    const BatchStats t = batchTotals();
    put(deviceDecided, t.reguideDecided), put(hostRun, t.reguideHost);
}
void bsplineTraj::deviceEpilogueTotals(long long* deviceDecided, long long* hostRun, long long* deviceGroups) {
    const BatchStats t = batchTotals();
    put(deviceDecided, t.epilogueDecided), put(hostRun, t.epilogueHost), put(deviceGroups, t.epilogueGroups);
}
void bsplineTraj::mixedBatchTotals(long long* deviceBatches, long long* planners) {
    const BatchStats t = batchTotals();
    put(deviceBatches, t.solveBatches), put(planners, t.solvePlanners);
}
void bsplineTraj::deviceSeedTotals(long long* deviceDecided, long long* hostRun) {
    const BatchStats t = batchTotals();
    put(deviceDecided, t.seedDecided), put(hostRun, t.seedHost);
}

// ---- device calls ---------------------------------------------------------------------

BatchStage& batchStage() {
    static thread_local BatchStage st;
    return st;
}

// hb into the calling thread's staging buffers, then map_->isUnknown(guidePoint) (BT.cpp:841) for its guides, hoisted
// out of the solve.  The buffers live across calls (hipMalloc/hipFree per rebound round cost more than the round's
// kernels): the thread's next upload overwrites them, so what a call reads back is read back before that.
bool uploadBatch(vigo_handle_t h, const HostBatch& hb, DeviceBatch& d) {
    BatchStage& st = batchStage();
    const size_t G = hb.guides();
    if (!st.ctrl.upload(hb.ctrl) || !st.goff.upload(hb.goff) || !st.gpv.upload(hb.gpv) || !st.gunk.alloc(G) || !st.ooff.upload(hb.ooff) ||
        !st.obs.upload(hb.obs) || !st.weights.upload(hb.weights))
        return false;
    if (G && vigo_guides_unknown(h, (int64_t)G, st.gpv.get(), st.gunk.get()) != VIGO_OK) return false;
    const bool mixed = !hb.uniform();
    if (mixed && !st.npts.upload(hb.npts)) return false;
    d = {st.ctrl.get(), st.goff.get(), G ? st.gpv.get() : nullptr, G ? st.gunk.get() : nullptr, st.ooff.get(),
         hb.obs.empty() ? nullptr : st.obs.get(), st.weights.get(), mixed ? st.npts.get() : nullptr};
    return true;
}

void bsplineTraj::solveBatch(const std::vector<bsplineTraj*>& ps, const BatchOptions& o, BatchStats& stats) {
    // groups of equal N share a launch (vigo_optimize takes one N per call); under mixedBatches the counts of one shape
    // class do (vigo_optimize_mixed), in rows of the group's largest count
    auto same = [&](size_t a, size_t b) { return ps[a]->sameSolveGroup(*ps[b], o.mixedBatches); };
    vigo_host::forEachGroup(ps.size(), same, [&](const std::vector<size_t>& grp) {
        bsplineTraj* lead = ps[grp[0]];
        int N = 0;        // the row stride: the group's one count, or its largest
        for (size_t k : grp) N = std::max(N, (int)ps[k]->optData_.controlPoints.cols());
        for (size_t k : grp) ps[k]->lastStatus_ = VIGO_ERR_HIP;
        if (lead->optData_.controlPoints.cols() < 7 || N > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return;
        stats.solveBatches += 1;
        stats.solvePlanners += (long long)grp.size();
        HostBatch hb(N);
        for (size_t k : grp) {
            const bsplineTraj* p = ps[k];
            hb.add(p->optData_.controlPoints.data(), (int)p->optData_.controlPoints.cols(), p->optData_,
                   {p->weightDistance_, p->weightSmoothness_, p->weightFeasibility_, p->weightDynamicObstacle_});
        }
        static thread_local Staged<int32_t> dStatus;
        vigo_handle_t h = lead->link_.handle();
        std::vector<int32_t> status(hb.B);
        DeviceBatch d;
        if (!uploadBatch(h, hb, d) || !dStatus.alloc(status.size())) return;
        // (a group of one count: the uniform entry, exactly as without the switch)
        if (d.npts ? !deviceCallOk(vigo_optimize_mixed(h, hb.B, N, d.npts, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, nullptr,
                                                       dStatus.get(), nullptr, nullptr, nullptr),
                                   "vigo_optimize_mixed", h)
                   : !deviceCallOk(vigo_optimize(h, hb.B, N, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, nullptr, dStatus.get(), nullptr,
                                                 nullptr, nullptr),
                                   "vigo_optimize", h))
            return;
        if (!vigo_host::threadSync() || !batchStage().ctrl.download(hb.ctrl) || !dStatus.download(status)) return;
        for (int b = 0; b < hb.B; ++b) {
            // optData_.controlPoints = the last evaluated point, as costFunction leaves it (BT.cpp:803)
            std::memcpy(ps[grp[b]]->optData_.controlPoints.data(), hb.row(b), sizeof(double) * 3 * hb.npts[b]);
            ps[grp[b]]->lastStatus_ = status[b];
        }
    });
}

namespace {
struct GateStage {
    Staged<double> ctrl, obs;
    Staged<int32_t> ooff;
    Staged<uint8_t> flag, dyn;   // [B] each
};
}  // namespace

void bsplineTraj::gateBatch(const std::vector<bsplineTraj*>& ps, std::vector<uint8_t>& col, std::vector<uint8_t>& dyn) {
    col.assign(ps.size(), 1);
    dyn.assign(ps.size(), 0);
    auto same = [&](size_t a, size_t b) { return ps[a]->sameBatchKey(*ps[b]); };
    vigo_host::forEachGroup(ps.size(), same, [&](const std::vector<size_t>& idx) {
        bsplineTraj* lead = ps[idx[0]];
        const int N = lead->optData_.controlPoints.cols();
        if (N < 4 || N > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return;
        std::vector<double> ctrl, obs;
        std::vector<int32_t> ooff{0};
        for (size_t b : idx) {
            vigo_host::appendCtrl(ps[b]->optData_.controlPoints, ctrl);
            vigo_host::appendObstacles(ps[b]->optData_, obs);
            ooff.push_back((int32_t)(obs.size() / 9));
        }
        const int B = (int)idx.size();
        static thread_local GateStage st;
        std::vector<uint8_t> f(B), d(B, 0);
        if (!st.ctrl.upload(ctrl) || !st.flag.alloc(f.size()) || !st.dyn.alloc(d.size()) || !st.ooff.upload(ooff) || !st.obs.upload(obs)) return;
        const double dt = lead->link_.map()->getRes() / lead->maxVel_ / 2.0;  // BT.h:312
        if (vigo_traj_collision(lead->link_.handle(), B, N, st.ctrl.get(), dt, st.flag.get(), nullptr) != VIGO_OK) return;
        if (!obs.empty()) {
            if (vigo_traj_dynamic_collision(lead->link_.handle(), B, N, st.ctrl.get(), dt, st.ooff.get(), st.obs.get(), 0, st.dyn.get()) != VIGO_OK)
                return;
        }
        if (!vigo_host::threadSync() || !st.flag.download(f)) return;
        if (!obs.empty() && !st.dyn.download(d)) return;
        for (int b = 0; b < B; ++b) {
            col[idx[b]] = f[b];
            // BT.cpp:621-626: the dynamic gate only runs when the planner has obstacles
            dyn[idx[b]] = ps[idx[b]]->optData_.dynamicObstaclesPos.empty() ? 0 : d[b];
        }
    });
}

// BT.cpp:611-685 between two A* calls, on the device, for one group of planners (one batch): upload the planners'
// state, queue the rounds (vigo_rebound_rounds), bring back what the host part of the loop needs.
bool bsplineTraj::deviceRounds(const std::vector<bsplineTraj*>& grp, const std::vector<Rebound*>& rb, int maxRounds, const BatchOptions& o,
                               BatchStats& stats) {
    bsplineTraj* lead = grp[0];
    int N = 0;            // the row stride: the group's one count, or (mixedBatches) its largest
    for (const bsplineTraj* p : grp) N = std::max(N, (int)p->optData_.controlPoints.cols());
    std::vector<int> prevStatus(grp.size());
    for (size_t k = 0; k < grp.size(); ++k) { prevStatus[k] = grp[k]->lastStatus_; grp[k]->lastStatus_ = VIGO_ERR_HIP; }
    if (lead->optData_.controlPoints.cols() < 7 || N > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return false;
    stats.solveBatches += 1;
    stats.solvePlanners += (long long)grp.size();
    HostBatch hb(N);
    std::vector<vigo_rebound_state_t> state(grp.size());
    for (size_t k = 0; k < grp.size(); ++k) {
        bsplineTraj* p = grp[k];
        hb.add(p->optData_.controlPoints.data(), (int)p->optData_.controlPoints.cols(), p->optData_,
               {p->weightDistance_, p->weightSmoothness_, p->weightFeasibility_, p->weightDynamicObstacle_});
        vigo_rebound_state_t& st = state[k];
        std::memset(&st, 0, sizeof(st));
        st.status = VIGO_RB_ACTIVE;
        st.lbfgs_status = prevStatus[k];      // kept when this call makes no optimize() for the planner
        st.solve_first = rb[k]->needOptimize ? 1 : 0;
        st.fail_count = rb[k]->failCount;
        st.n_seg = (int32_t)p->collisionSeg_.size();
        if (st.n_seg > VIGO_MAX_COLLISION_SEGS) {
            // more previous segments than the device state holds: this planner's rounds stay with the host (one gate,
            // then reboundStep) — a trajectory of VIGO_MAX_CTRL_POINTS control points can get there, a 7 m path cannot
            st.status = VIGO_RB_NEEDS_HOST;
            st.n_seg = 0;
        } else {
            for (int q = 0; q < st.n_seg; ++q) { st.seg[2 * q] = p->collisionSeg_[q].first; st.seg[2 * q + 1] = p->collisionSeg_[q].second; }
        }
    }
    static thread_local Staged<vigo_rebound_state_t> dState;
    DeviceBatch d;
    if (!uploadBatch(lead->link_.handle(), hb, d) || !dState.upload(state)) return false;
    vigo_handle_t h = lead->link_.handle();
    const double dt = lead->link_.map()->getRes() / lead->maxVel_ / 2.0;  // BT.h:312
    if (d.npts ? !deviceCallOk(vigo_rebound_rounds_mixed(h, hb.B, N, d.npts, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, dt,
                                                         lead->notCheckRatio_, maxRounds, dState.get()),
                               "vigo_rebound_rounds_mixed", h)
               : !deviceCallOk(vigo_rebound_rounds(h, hb.B, N, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, dt, lead->notCheckRatio_,
                                                   maxRounds, dState.get()),
                               "vigo_rebound_rounds", h))
        return false;
    // everything is read back here: the solveBatch of the overflow planners below reuses the staging buffers
    if (!vigo_host::threadSync() || !batchStage().ctrl.download(hb.ctrl) || !batchStage().weights.download(hb.weights) || !dState.download(state))
        return false;
    std::vector<size_t> overflow;
    for (size_t k = 0; k < grp.size(); ++k) {
        bsplineTraj* p = grp[k];
        const vigo_rebound_state_t& st = state[k];
        if (st.rounds == 0 && st.status == VIGO_RB_NEEDS_HOST) { overflow.push_back(k); continue; }
        // optData_.controlPoints = the last evaluated point, as costFunction leaves it (BT.cpp:803)
        std::memcpy(p->optData_.controlPoints.data(), hb.row((int)k), sizeof(double) * 3 * hb.npts[k]);
        p->weightDistance_ = hb.weights[4 * k + 0];
        p->weightDynamicObstacle_ = hb.weights[4 * k + 3];
        p->lastStatus_ = st.lbfgs_status;
        p->collisionSeg_.clear();
        for (int q = 0; q < st.n_seg; ++q) p->collisionSeg_.push_back({st.seg[2 * q], st.seg[2 * q + 1]});
        rb[k]->failCount = st.fail_count;
        rb[k]->needOptimize = st.solve_first != 0;     // an optimize() the device deferred to the next call
        rb[k]->devStatus = st.status;
        rb[k]->gateStatic = st.gate_static != 0;
        rb[k]->gateDynamic = st.gate_dynamic != 0;
    }
    // planners the device state cannot represent: one host-driven round (solve if owed, gate; the caller steps)
    for (size_t k : overflow) {
        std::vector<bsplineTraj*> one{grp[k]};
        Rebound& r = *rb[k];
        if (r.needOptimize) solveBatch(one, o, stats);
        std::vector<uint8_t> col, dyn;
        gateBatch(one, col, dyn);
        r.gateStatic = col[0] != 0;
        r.gateDynamic = dyn[0] != 0;
        r.devStatus = (!r.gateStatic && !r.gateDynamic) ? VIGO_RB_DONE : VIGO_RB_NEEDS_HOST;
    }
    return true;
}

// BT.cpp:333-385 for many planners at once: host prologue per planner, then the rebound loops in
// lock-step so each optimize() round is one launch over all still-active planners.
std::vector<bool> bsplineTraj::makePlanBatch(const std::vector<bsplineTraj*>& planners, const BatchOptions& options, BatchStats* stats) {
    BatchStats st;
    std::vector<bool> result = planBatch(planners, nullptr, true, options.normalized(), st);
    reportBatchStats(st, stats);
    return result;
}

std::vector<bool> bsplineTraj::makePlanBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>& trajectories, bool yaw,
                                             const BatchOptions& options, BatchStats* stats) {
    trajectories.assign(planners.size(), nav_msgs::Path());
    BatchStats st;
    std::vector<bool> result = planBatch(planners, trajectories.data(), yaw, options.normalized(), st);
    reportBatchStats(st, stats);
    return result;
}

std::vector<bool> bsplineTraj::makePlanBatch(const std::vector<bsplineTraj*>& planners) { return makePlanBatch(planners, defaultBatchOptions()); }

std::vector<bool> bsplineTraj::makePlanBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>& trajectories, bool yaw) {
    return makePlanBatch(planners, trajectories, yaw, defaultBatchOptions());
}

std::vector<bool> bsplineTraj::planBatch(const std::vector<bsplineTraj*>& planners, nav_msgs::Path* paths, bool yaw, const BatchOptions& o,
                                         BatchStats& stats) {
    const size_t P = planners.size();
    if (o.pipelineThreshold > 0 && P >= o.pipelineThreshold && P >= 2) return makePlanPipelined(planners, paths, yaw, o, stats);
    return planPart(planners, paths, yaw, o, stats);
}

// one unsplit batch: a whole call, or one part of a pipelined one
std::vector<bool> bsplineTraj::planPart(const std::vector<bsplineTraj*>& planners, nav_msgs::Path* paths, bool yaw, const BatchOptions& o,
                                        BatchStats& stats) {
    const size_t P = planners.size();
    PlanBatch pb(P, o);
    const bool timing = getenv("VIGO_FACADE_TIMING") != nullptr;
    const double tp0 = wallSeconds();
    planPrologue(planners, pb);
    const double tp1 = wallSeconds();
    pb.stats.prologueSeconds += tp1 - tp0;
    // step 4: rebound loops.  The 30 ms budget of BT.cpp:633 is per makePlan() call in the
    // reference; a batch keeps it per round so one slow planner cannot starve the others.
    if (o.deviceResidentRebound) reboundOnDevice(pb, timing);
    else reboundFromHost(pb, timing);
    const double tp2 = wallSeconds();
    planEpilogue(planners, pb.result, paths, yaw, o, pb.stats);
    if (timing) {
        cout << "[BsplineTraj]: prologue CPU time summed over the workers: findCollisionSeg " << pb.nsSeg.load() * 1e-6 << " ms, A* "
             << pb.nsAstar.load() * 1e-6 << " ms, guide assignment " << pb.nsGuide.load() * 1e-6 << " ms; device chains (wall) "
             << pb.nsChain.load() * 1e-6 << " ms" << endl;
        cout << "[BsplineTraj]: makePlanBatch of " << P << ": prologue " << (tp1 - tp0) * 1e3 << " ms, rebound loop " << (tp2 - tp1) * 1e3
             << " ms, epilogue " << (wallSeconds() - tp2) * 1e3 << " ms" << endl;
    }
    stats += pb.stats;
    return pb.result;
}

// A large batch runs as two to four pipelined parts of >= threshold / 2 planners, all but the first on companion
// host threads with their own handles and HIP streams: while one part waits for its device rounds (a chain of
// single-wave solves, ~10 ms per 1024 planners) the others' host work (A*, guide assignment) and device rounds
// proceed — what a caller otherwise gets only by planning from several threads of its own.  Planners are independent
// (per-trajectory results do not depend on which batch carries them), so the plans are those of the unsplit call.
// Every part runs under the call's options — with a step log of its own, appended to the call's in part order — and
// counts into stats of its own, summed when all have ended.
std::vector<bool> bsplineTraj::makePlanPipelined(const std::vector<bsplineTraj*>& planners, nav_msgs::Path* paths, bool yaw, const BatchOptions& o,
                                                 BatchStats& stats) {
    constexpr size_t kMaxParts = 4;
    static thread_local Companion companions[kMaxParts - 1];
    const size_t P = planners.size();
    const size_t per = o.pipelineThreshold / 2 > 0 ? o.pipelineThreshold / 2 : 1;
    const size_t parts = std::min(kMaxParts, std::max<size_t>(2, P / per));
    std::vector<std::vector<bsplineTraj*>> piece(parts);
    std::vector<std::vector<bool>> res(parts);
    std::vector<nav_msgs::Path*> out(parts, nullptr);      // a part's paths: its stretch of the call's
    std::vector<BatchOptions> opt(parts, o);
    std::vector<BatchStats> partStats(parts);
    std::vector<std::vector<ReguideStepRecord>> log(parts);
    for (size_t k = 0; k < parts; ++k) {
        const size_t lo = P * k / parts, hi = P * (k + 1) / parts;
        piece[k].assign(planners.begin() + lo, planners.begin() + hi);
        res[k].assign(hi - lo, false);
        if (paths) out[k] = paths + lo;
        if (o.reguideStepLog) opt[k].reguideStepLog = &log[k];
    }
    for (size_t k = 1; k < parts; ++k)
        companions[k - 1].start([&piece, &res, &out, &opt, &partStats, yaw, k]() { res[k] = bsplineTraj::planPart(piece[k], out[k], yaw, opt[k], partStats[k]); });
    // the jobs hold piece and res: every part has ended before an exception leaves (the first one in part order)
    std::exception_ptr err;
    try { res[0] = bsplineTraj::planPart(piece[0], out[0], yaw, opt[0], partStats[0]); } catch (...) { err = std::current_exception(); }
    for (size_t k = 1; k < parts; ++k)
        try { companions[k - 1].wait(); } catch (...) { if (!err) err = std::current_exception(); }
    if (err) std::rethrow_exception(err);
    std::vector<bool> all;
    for (size_t k = 0; k < parts; ++k) {
        all.insert(all.end(), res[k].begin(), res[k].end());
        stats += partStats[k];
        if (o.reguideStepLog) o.reguideStepLog->insert(o.reguideStepLog->end(), log[k].begin(), log[k].end());
    }
    return all;
}

// steps 1-3 (collision segments, A*, guide assignment) touch only the planner's own state and the read-only map: the
// planners are spread over the host cores.  Those that get through enter the rebound loop.
void bsplineTraj::planPrologue(const std::vector<bsplineTraj*>& planners, PlanBatch& pb) {
    const size_t P = planners.size();
    std::vector<uint8_t> prepared(P, 0), hasPaths(P, 0);
    const int guides = pb.o.devicePrologue ? 0 : pb.o.deviceGuides;
    if (pb.o.devicePrologue) {
        // the three steps as one device chain per group; what the device does not decide runs the host steps there too
        std::vector<uint8_t> outcome(P, 0);
        prologueOnDevice(planners, pb, outcome);
        for (size_t i = 0; i < P; ++i) prepared[i] = outcome[i] == 1;
    } else {
        // The host steps, per planner on the workers, all three in one pass.  deviceAstar gathers step 2 over the
        // planners (pathSearchBatch: the searches of all of them on the device): steps 1 and 3 are then a pass each
        // around it.  deviceGuides gathers step 3 (below).
        const bool gathered = pb.o.deviceAstar;
        std::vector<uint8_t> ready(P, 0);
        auto assignGuides = [&](size_t i) {
            const double t2 = wallSeconds();
            planners[i]->assignGuidePointsSemiCircle(planners[i]->astarPaths_, planners[i]->collisionSeg_);   // step 3
            pb.nsGuide += (long long)((wallSeconds() - t2) * 1e9);
            prepared[i] = 1;
        };
        parallelFor(P, [&](size_t i) {
            bsplineTraj* p = planners[i];
            if (!p->init_ || !p->link_.map() || !pb.hostSteps(p, !gathered)) return;
            if (gathered) ready[i] = 1;
            else if (guides != 0) hasPaths[i] = 1;
            else assignGuides(i);
        });
        if (gathered) {
            const double t1 = wallSeconds();
            pathSearchBatch(planners, pb, ready, hasPaths);                                 // step 2
            pb.nsAstar += (long long)((wallSeconds() - t1) * 1e9);
            if (guides == 0)
                parallelFor(P, [&](size_t i) {
                    if (hasPaths[i]) assignGuides(i);
                });
        }
    }
    if (guides != 0) {
        // step 3 gathered over the planners (deviceGuides): the device, or its twin on the workers
        const double t2 = wallSeconds();
        assignGuidesBatch(planners, pb, hasPaths);
        pb.nsGuide += (long long)((wallSeconds() - t2) * 1e9);
        prepared = hasPaths;
    }
    for (size_t i = 0; i < P; ++i) {
        bsplineTraj* p = planners[i];
        if (!p->init_ || !p->link_.map()) continue;
        if (!prepared[i]) {
            cout << "[BsplineTraj]: Fail because of A* failure." << endl;
            continue;
        }
        p->reboundBegin(pb.rb[i]);
        pb.active.push_back(p);
        pb.activeIdx.push_back(i);
    }
}

namespace {
struct AstarStage {
    Staged<double> start, end, path;   // [Q][3] up; [Q][kAstarPathCap][3] back
    Staged<int32_t> status, len;       // [Q]
};
}  // namespace

// The jobs' searches: one vigo_astar_search per group of planners that share a snapshot, a node pool and a height band;
// what the device does not decide (deferred, path too long, no device or snapshot) is searched by the planner's own
// host A* on the workers.
void bsplineTraj::runAstarJobs(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, std::vector<AstarJob>& jobs) {
    if (jobs.empty()) return;
    const size_t P = planners.size();
    std::vector<uint8_t> decided(jobs.size(), 0);
    std::vector<std::vector<size_t>> jobsOf(P);
    for (size_t j = 0; j < jobs.size(); ++j) jobsOf[jobs[j].planner].push_back(j);
    std::vector<size_t> owners;                       // the planners with jobs, in call order
    for (size_t i = 0; i < P; ++i)
        if (!jobsOf[i].empty()) owners.push_back(i);
    // (the searches have no control-point count: under mixedPrologue the planners of a shape class share the launch)
    SearchGroup::forEach(planners, owners, false, pb.o.mixedPrologue, [&](bsplineTraj* lead, const SearchGroup& g, const std::vector<size_t>& who) {
        std::vector<size_t> idx;
        std::vector<double> start, end;
        for (size_t i : who)
            for (size_t j : jobsOf[i]) {
                // a search whose node pool (around the midpoint of its ends) is not in reach stays with the host
                const double mid[3] = {(jobs[j].s(0) + jobs[j].e(0)) / 2, (jobs[j].s(1) + jobs[j].e(1)) / 2, (jobs[j].s(2) + jobs[j].e(2)) / 2};
                if (!g.inReach(*planners[i], mid, 1)) continue;
                idx.push_back(j);
                for (int k = 0; k < 3; ++k) { start.push_back(jobs[j].s(k)); end.push_back(jobs[j].e(k)); }
            }
        const int Q = (int)idx.size();
        if (Q == 0) return;
        static thread_local AstarStage st;
        vigo_handle_t h = lead->link_.handle();
        std::vector<int32_t> status(Q), len(Q);
        std::vector<double> path((size_t)Q * kAstarPathCap * 3);
        if (!st.start.upload(start) || !st.end.upload(end) || !st.status.alloc(status.size()) || !st.len.alloc(len.size()) || !st.path.alloc(path.size()))
            return;
        pb.stats.prologueGroups += 1;
        if (!deviceCallOk(vigo_astar_search(h, Q, st.start.get(), st.end.get(), g.res, g.pool, lead->minHeight_, lead->maxHeight_,
                                            pb.o.deviceAstarBudget, kAstarPathCap, st.status.get(), st.len.get(), st.path.get(), nullptr),
                          "vigo_astar_search", h))
            return;
        if (!vigo_host::threadSync() || !st.status.download(status) || !st.len.download(len) || !st.path.download(path)) return;
        for (int q = 0; q < Q; ++q) {
            AstarJob& J = jobs[idx[q]];
            if (status[q] == VIGO_ASTAR_NOT_FOUND) {
                decided[idx[q]] = 1;
            } else if (status[q] == VIGO_ASTAR_FOUND && len[q] >= 1 && len[q] <= kAstarPathCap) {
                const double* src = path.data() + (size_t)q * kAstarPathCap * 3;
                J.path.resize(len[q]);
                for (int i = 0; i < len[q]; ++i) J.path[i] = Eigen::Vector3d(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
                J.ok = true;
                decided[idx[q]] = 1;
            }
        }
    });
    long long nDecided = 0;
    for (uint8_t d : decided) nDecided += d;
    pb.stats.astarDecided += nDecided;
    pb.stats.astarHost += (long long)jobs.size() - nDecided;
    parallelFor(owners.size(), [&](size_t o) {
        bsplineTraj* p = planners[owners[o]];
        for (size_t j : jobsOf[owners[o]]) {
            if (decided[j]) continue;
            AstarJob& J = jobs[j];
            J.ok = p->pathSearch_->AstarSearch(p->link_.map()->getRes(), J.s, J.e);
            if (J.ok) J.path = p->pathSearch_->getPath();
        }
    });
}

// pathSearch (BT.cpp:447-514) for all planners at once.  Which searches a planner's loop makes depends on their outcomes
// only through the merge rule: on a failure, pStart to the NEXT segment's end when the gap is <= 2, then that segment is
// skipped.  A search is a function of its two ends alone, so the first-choice search of every segment goes into one
// launch, the merged retries the failures ask for into a second one (taking every retry to succeed when looking for
// the next: a retry that fails ends the planner's loop, and what was searched beyond it is not used), and the loop is
// then replayed per planner on the results.  The price: the first launch also searches the segments the merge rule goes
// on to skip and those behind a failure that ends a planner's loop — searches the host's loop never makes, long ones by
// construction (a skipped segment's own search is one that may well fail), and worker time when the device defers
// them.  It buys one launch instead of a launch per segment index; weigh it when the timings are taken.
void bsplineTraj::pathSearchBatch(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, const std::vector<uint8_t>& ready,
                                  std::vector<uint8_t>& found) {
    const size_t P = planners.size();
    std::vector<AstarJob> first, retry;
    std::vector<size_t> firstOf(P, 0);
    for (size_t i = 0; i < P; ++i) {
        if (!ready[i]) continue;
        const bsplineTraj* p = planners[i];
        firstOf[i] = first.size();
        for (int k = 0; k < (int)p->collisionSeg_.size(); ++k) {
            AstarJob J;
            J.planner = i; J.seg = k; J.endSeg = k;
            J.s = p->optData_.controlPoints.col(p->collisionSeg_[k].first);
            J.e = p->optData_.controlPoints.col(p->collisionSeg_[k].second);
            first.push_back(J);
        }
    }
    runAstarJobs(planners, pb, first);
    std::vector<std::vector<size_t>> retryOf(P);
    for (size_t i = 0; i < P; ++i) {
        if (!ready[i]) continue;
        const bsplineTraj* p = planners[i];
        const int n = (int)p->collisionSeg_.size();
        for (int k = 0; k < n; ++k) {
            if (first[firstOf[i] + k].ok) continue;
            if (k + 1 >= n || p->collisionSeg_[k + 1].first - p->collisionSeg_[k].second > 2) break;
            AstarJob J;
            J.planner = i; J.seg = k; J.endSeg = k + 1;
            J.s = first[firstOf[i] + k].s;
            J.e = p->optData_.controlPoints.col(p->collisionSeg_[k + 1].second);
            retryOf[i].push_back(retry.size());
            retry.push_back(J);
            ++k;
        }
    }
    runAstarJobs(planners, pb, retry);
    parallelFor(P, [&](size_t i) {
        if (!ready[i]) return;
        bsplineTraj* p = planners[i];
        std::vector<std::pair<int, int>>& collisionSeg = p->collisionSeg_;
        std::vector<std::vector<Eigen::Vector3d>>& paths = p->astarPaths_;
        paths.clear();
        std::vector<int> mergeIndices;
        const int n = (int)collisionSeg.size();
        size_t nextRetry = 0;
        for (int k = 0; k < n; ++k) {
            const AstarJob* J = &first[firstOf[i] + k];
            if (!J->ok) {
                J = nullptr;
                if (k + 1 < n && collisionSeg[k + 1].first - collisionSeg[k].second <= 2) {
                    const AstarJob& R = retry[retryOf[i][nextRetry++]];
                    if (R.ok) {
                        J = &R;
                        mergeIndices.push_back(k);
                    }
                }
                if (!J) {
                    cout << "[BsplineTraj]: Path Search Error. Force return." << endl;
                    return;
                }
            }
            std::vector<Eigen::Vector3d> searchedPath = J->path;
            searchedPath[0] = J->s;
            searchedPath.push_back(J->e);
            paths.push_back(searchedPath);
            if (J->endSeg != k) ++k;
        }
        applyMerges(collisionSeg, mergeIndices);
        found[i] = 1;
    });
}

namespace {
// The tail of a stage's downloads, once its S segments and nPairs guide pairs are known to fit their buffers: the S + 1
// path offsets (S > 0; else the one offset is 0), checked against pointCap, then the path points and the pairs there are.
bool downloadPathsAndPairs(int S, long long pointCap, long long nPairs, const Staged<int32_t>& dPathOff, const Staged<double>& dPath,
                           const Staged<double>& dPv, std::vector<int32_t>& pathOff, std::vector<double>& path, std::vector<double>& pv) {
    pathOff.assign((size_t)S + 1, 0);
    if (S > 0 && !dPathOff.download(pathOff)) return false;
    if (pathOff[S] < 0 || pathOff[S] > pointCap) return false;
    path.resize((size_t)pathOff[S] * 3);
    pv.resize((size_t)nPairs * 6);
    return (path.empty() || dPath.download(path)) && (pv.empty() || dPv.download(pv));
}

// what prologueOnDevice stages per group: vigo_path_search's outputs are vigo_guide_assign's inputs, in place
struct PrologueStage {
    Staged<double> ctrl, path, pv;                                   // [B][N][3]; [pointCap][3]; [pairCap][6]
    Staged<int32_t> status, segOff, seg, pathOff, counts, off, gstatus, npts;   // npts [B]: a group of mixed counts only
};
// ... assignGuidesBatch, which uploads the lists the planners hold
struct GuideStage {
    Staged<double> ctrl, path, pv;
    Staged<int32_t> segOff, seg, pathOff, off, status, npts;
};
// ... and reguideOnDevice on top of uploadBatch's set
struct ReguideStage {
    Staged<vigo_rebound_state_t> state;
    Staged<double> pv, path;
    Staged<int32_t> off, pathSegOff, pathOff, status;
};
}  // namespace

// Steps 1-3 for all planners under devicePrologue.  Per group of planners that share a batch key and a node
// pool (mixedPrologue: whatever their counts inside a shape class — rows padded to the group's largest count, the _mixed
// entries; a group of one count calls the uniform ones): control points up, vigo_path_search on the scanned segments, vigo_guide_assign on its output (device pointers,
// nothing repacked), then one round of downloads and the results installed per planner.  What is left (see the header)
// runs findCollisionSeg -> pathSearch -> assignGuidesCore on the workers.
// Buffer sizes: segCap = B * VIGO_MAX_COLLISION_SEGS is the entry's own bound.  pointCap = B * 2 * (kAstarPathCap + 1) and
// pairCap = B * N * 4 are budgets, not bounds (the bounds, 48 full-length paths per planner and every path point a pair,
// would be ~150 MB per 1024 planners): two full-length paths and four pairs per control point on AVERAGE over the
// group, against 17 path points and 4.4 pairs per PLANNER on the pipeline batches.  A group over pointCap gets
// VIGO_ERR_INVALID_ARG from vigo_path_search (nothing written, the message is printed) and runs the host steps as a
// whole; a group over pairCap keeps the device's segments and paths and has the twin assign its guides.  Both are
// correct and slow, and both show in the stats' prologueHost.
void bsplineTraj::prologueOnDevice(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, std::vector<uint8_t>& outcome) {
    const size_t P = planners.size();
    std::vector<uint8_t> needGuides(P, 0);            // segments and paths are installed, the pairs are not
    std::vector<uint8_t> failedOnDevice(P, 0);        // the device's walk failed: the host's replay leaves the lists
    std::vector<size_t> owners;
    for (size_t i = 0; i < P; ++i)
        if (planners[i]->init_ && planners[i]->link_.map()) owners.push_back(i);
    const double tc0 = wallSeconds();
    SearchGroup::forEach(planners, owners, true, pb.o.mixedPrologue, [&](bsplineTraj* lead, const SearchGroup& g, const std::vector<size_t>& who) {
        const int N = g.N, B = (int)who.size();
        HostBatch rows(N);
        for (size_t i : who) rows.addRow(planners[i]->optData_.controlPoints.data(), (int)planners[i]->optData_.controlPoints.cols());
        const std::vector<double>& ctrl = rows.ctrl;
        const long long segCap = (long long)B * VIGO_MAX_COLLISION_SEGS, pointCap = (long long)B * 2 * (kAstarPathCap + 1),
                        pairCap = (long long)B * N * 4;
        static thread_local PrologueStage st;
        vigo_handle_t h = lead->link_.handle();
        std::vector<int32_t> status(B), segOff(B + 1), counts((size_t)B * 2), off((size_t)B * N + 1, 0), gstatus(B, VIGO_GUIDE_DEFERRED);
        if (!st.ctrl.upload(ctrl) || !st.status.alloc(status.size()) || !st.segOff.alloc(segOff.size()) || !st.seg.alloc((size_t)segCap * 2) ||
            !st.pathOff.alloc((size_t)segCap + 1) || !st.path.alloc((size_t)pointCap * 3) || !st.counts.alloc(counts.size()) ||
            !st.off.alloc(off.size()) || !st.pv.alloc((size_t)pairCap * 6) || !st.gstatus.alloc(gstatus.size()) ||
            (!g.uniform && !st.npts.upload(rows.npts)))
            return;
        pb.stats.prologueGroups += 1;
        if (g.uniform ? !deviceCallOk(vigo_path_search(h, B, N, st.ctrl.get(), nullptr, nullptr, lead->notCheckRatio_, g.res, g.pool, lead->minHeight_,
                                                       lead->maxHeight_, pb.o.deviceAstarBudget, kAstarPathCap, segCap, pointCap, st.status.get(),
                                                       st.segOff.get(), st.seg.get(), st.pathOff.get(), st.path.get(), st.counts.get()),
                                      "vigo_path_search", h)
                      : !deviceCallOk(vigo_path_search_mixed(h, B, N, st.npts.get(), st.ctrl.get(), nullptr, nullptr, lead->notCheckRatio_, g.res, g.pool,
                                                             lead->minHeight_, lead->maxHeight_, pb.o.deviceAstarBudget, kAstarPathCap, segCap, pointCap,
                                                             st.status.get(), st.segOff.get(), st.seg.get(), st.pathOff.get(), st.path.get(),
                                                             st.counts.get()),
                                      "vigo_path_search_mixed", h))
            return;
        // (not VIGO_OK: the pairs do not fit — the twin assigns them)
        const bool guided = (g.uniform ? vigo_guide_assign(h, B, N, st.ctrl.get(), st.segOff.get(), st.seg.get(), st.pathOff.get(), st.path.get(), pairCap,
                                                           st.off.get(), st.pv.get(), nullptr, st.gstatus.get())
                                       : vigo_guide_assign_mixed(h, B, N, st.npts.get(), st.ctrl.get(), st.segOff.get(), st.seg.get(), st.pathOff.get(),
                                                                 st.path.get(), pairCap, st.off.get(), st.pv.get(), nullptr, st.gstatus.get())) == VIGO_OK;
        if (!vigo_host::threadSync() || !st.status.download(status) || !st.segOff.download(segOff) || !st.counts.download(counts)) return;
        if (guided && (!st.off.download(off) || !st.gstatus.download(gstatus))) return;
        const int S = segOff[B];
        if (S < 0 || S > segCap || off.back() < 0 || off.back() > pairCap) return;
        std::vector<int32_t> seg((size_t)S * 2), pathOff;
        std::vector<double> path, pv;
        if (S > 0 && !st.seg.download(seg)) return;
        if (!downloadPathsAndPairs(S, pointCap, off.back(), st.pathOff, st.path, st.pv, pathOff, path, pv)) return;
        for (int b = 0; b < B; ++b) {
            bsplineTraj* p = planners[who[b]];
            // A failed walk owns nothing on the device, but the host steps leave the scanned segments and the paths found
            // before the failure in collisionSeg_ / astarPaths_: the planner replays steps 1-2 on the workers below.
            if (status[b] == VIGO_PATHS_FAILED) { failedOnDevice[who[b]] = 1; continue; }
            const int nOut = segOff[b + 1] - segOff[b];
            // the device returns the bounded lists only: a planner whose astarPaths_ is longer runs the host steps
            if (status[b] != VIGO_PATHS_OK || vigo::paths_cut_by_bound(counts[2 * (size_t)b], nOut)) continue;
            p->collisionSeg_.clear();
            for (int k = segOff[b]; k < segOff[b + 1]; ++k) p->collisionSeg_.push_back({seg[2 * (size_t)k], seg[2 * (size_t)k + 1]});
            vigo_host::installPaths(p->astarPaths_, segOff[b], segOff[b + 1], pathOff.data(), path.data());
            if (gstatus[b] != VIGO_GUIDE_OK) { needGuides[who[b]] = 1; continue; }
            vigo_host::installGuides(p->optData_, rows.npts[b], off.data() + (size_t)b * N, pv.data());
            outcome[who[b]] = 1;
        }
    });
    const long long chainNs = (long long)((wallSeconds() - tc0) * 1e9);
    pb.nsChain += chainNs;
    pb.stats.chainSeconds += chainNs * 1e-9;
    long long nDecided = 0;
    for (size_t i : owners) nDecided += (outcome[i] != 0 && !needGuides[i]) || failedOnDevice[i];
    pb.stats.prologueDecided += nDecided;
    pb.stats.prologueHost += (long long)owners.size() - nDecided;
    parallelFor(owners.size(), [&](size_t o) {
        const size_t i = owners[o];
        bsplineTraj* p = planners[i];
        if (outcome[i] != 0) return;
        if (!needGuides[i] && !pb.hostSteps(p, true)) { outcome[i] = 2; return; }       // steps 1-2
        const double t2 = wallSeconds();
        p->assignGuidesCore();                                                          // step 3, the device's code
        pb.nsGuide += (long long)((wallSeconds() - t2) * 1e9);
        outcome[i] = 1;
    });
}

// segments and paths as vigo_guide_assign takes them: the first min(collisionSeg.size(), paths.size()) of both
// (BT.cpp:523), paths as CSR
static void packGuideLists(const std::vector<std::pair<int, int>>& collisionSeg, const std::vector<std::vector<Eigen::Vector3d>>& paths,
                           std::vector<int32_t>& seg, std::vector<int32_t>& pathOff, std::vector<double>& path) {
    const size_t n = std::min(collisionSeg.size(), paths.size());
    for (size_t k = 0; k < n; ++k) {
        seg.push_back(collisionSeg[k].first);
        seg.push_back(collisionSeg[k].second);
        for (const Eigen::Vector3d& v : paths[k])
            for (int a = 0; a < 3; ++a) path.push_back(v(a));
        pathOff.push_back((int32_t)(path.size() / 3));
    }
}

// the planner's own
void bsplineTraj::packGuideInput(std::vector<int32_t>& seg, std::vector<int32_t>& pathOff, std::vector<double>& path) const {
    packGuideLists(this->collisionSeg_, this->astarPaths_, seg, pathOff, path);
}

// assignGuidePointsSemiCircle by the device's code (csrc/vigo_guide_core.hpp with vigo_atan2) on the planner's own map
void bsplineTraj::assignGuidesCore() { this->assignGuidesCoreOn(this->collisionSeg_, this->astarPaths_); }

void bsplineTraj::assignGuidesCoreOn(const std::vector<std::pair<int, int>>& collisionSeg, const std::vector<std::vector<Eigen::Vector3d>>& paths) {
    std::vector<int32_t> seg, pathOff{0};
    std::vector<double> path;
    packGuideLists(collisionSeg, paths, seg, pathOff, path);
    const int N = this->optData_.controlPoints.cols();
    std::vector<double> ctrl;
    vigo_host::appendCtrl(this->optData_.controlPoints, ctrl);
    size_t longest = 1;
    for (size_t k = 0; k + 1 < pathOff.size(); ++k) {
        if (pathOff[k + 1] - pathOff[k] < 1) return;     // (pathSearch leaves at least the two ends)
        longest = std::max(longest, (size_t)(pathOff[k + 1] - pathOff[k]));
    }
    std::vector<vigo::G3> sc(longest);
    auto* map = link_.map().get();
    auto occ = [map](double x, double y, double z) { return map->isInflatedOccupied(Eigen::Vector3d(x, y, z)); };
    vigo::guide_assign(occ, vigo::GuideAtan2{}, this->link_.map()->getRes(), N, ctrl.data(), (int)(seg.size() / 2), seg.data(), pathOff.data(),
                       path.data(), sc.data(), [this](int idx, const vigo::G3& p, const vigo::G3& d, const int32_t*) {
                           this->optData_.guidePoints[idx].push_back(Eigen::Vector3d(p.v[0], p.v[1], p.v[2]));
                           this->optData_.guideDirections[idx].push_back(Eigen::Vector3d(d.v[0], d.v[1], d.v[2]));
                       });
}

// Step 3 for the planners with found[i].  Setting 1: one vigo_guide_assign per group of planners that share a snapshot
// and a control-point count; the pairs come back as CSR per control point in push order and are appended to the planners'
// lists.  Whatever the device did not produce (deferred, no device, a failed call), and everything under setting 2, is
// computed by assignGuidesCore on the workers: the same code, the same pairs.
void bsplineTraj::assignGuidesBatch(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, const std::vector<uint8_t>& found) {
    const size_t P = planners.size();
    std::vector<uint8_t> done(P, 0);
    if (pb.o.deviceGuides == 1) {
        std::vector<size_t> owners;
        for (size_t i = 0; i < P; ++i)
            if (found[i]) owners.push_back(i);
        auto same = [&](size_t a, size_t b) {
            const bsplineTraj* x = planners[owners[a]];
            const bsplineTraj* y = planners[owners[b]];
            return x->sameSolveGroup(*y, pb.o.mixedPrologue);      // (one count per group, or with mixedPrologue a shape class)
        };
        vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
            bsplineTraj* lead = planners[owners[members[0]]];
            if (!lead->syncDevice()) return;
            int N = 0;                                    // the row stride: the group's one count, or its largest
            for (size_t m : members) N = std::max(N, (int)planners[owners[m]]->optData_.controlPoints.cols());
            HostBatch rows(N);
            std::vector<size_t> who;
            std::vector<double> path;
            std::vector<int32_t> segOff{0}, seg, pathOff{0};
            long long pairs = 0;
            for (size_t m : members) {
                const bsplineTraj* p = planners[owners[m]];
                const size_t seg0 = seg.size() / 2;
                p->packGuideInput(seg, pathOff, path);
#ifdef VIGO_WITH_ROS
                // the line checks stay inside the box of the path points: a planner with a path point outside the region
                // keeps to its own map (the twin), and what was packed of it is taken back
                const size_t pt0 = (size_t)pathOff[seg0];
                const double none[3] = {0.0, 0.0, 0.0};
                if (!boxInRegion(p->link_.region(), path.data() + pt0 * 3, path.size() / 3 - pt0, none)) {
                    seg.resize(seg0 * 2);
                    path.resize(pt0 * 3);
                    pathOff.resize(seg0 + 1);
                    continue;
                }
#endif
                const int n = (int)p->optData_.controlPoints.cols();
                for (size_t k = seg0; k < seg.size() / 2; ++k) pairs += vigo::guide_pushes_total(n, seg[2 * k], seg[2 * k + 1]);
                segOff.push_back((int32_t)(seg.size() / 2));
                rows.addRow(p->optData_.controlPoints.data(), n);
                who.push_back(owners[m]);
            }
            const int B = (int)who.size();
            if (B == 0) return;
            if (seg.empty()) {                       // no segments anywhere: nothing to assign
                for (size_t i : who) done[i] = 1;
                return;
            }
            const long long cap = std::max<long long>(pairs, 1);
            static thread_local GuideStage st;
            vigo_handle_t h = lead->link_.handle();
            std::vector<int32_t> off((size_t)B * N + 1), status(B);
            const bool uniform = rows.uniform();
            if (!st.ctrl.upload(rows.ctrl) || !st.segOff.upload(segOff) || !st.seg.upload(seg) || !st.pathOff.upload(pathOff) || !st.path.upload(path) ||
                !st.off.alloc(off.size()) || !st.pv.alloc((size_t)cap * 6) || !st.status.alloc(status.size()) || (!uniform && !st.npts.upload(rows.npts)))
                return;
            pb.stats.prologueGroups += 1;
            if (uniform ? !deviceCallOk(vigo_guide_assign(h, B, N, st.ctrl.get(), st.segOff.get(), st.seg.get(), st.pathOff.get(), st.path.get(), cap,
                                                          st.off.get(), st.pv.get(), nullptr, st.status.get()),
                                        "vigo_guide_assign", h)
                        : !deviceCallOk(vigo_guide_assign_mixed(h, B, N, st.npts.get(), st.ctrl.get(), st.segOff.get(), st.seg.get(), st.pathOff.get(),
                                                                st.path.get(), cap, st.off.get(), st.pv.get(), nullptr, st.status.get()),
                                        "vigo_guide_assign_mixed", h))
                return;
            if (!vigo_host::threadSync() || !st.off.download(off) || !st.status.download(status)) return;
            std::vector<double> pv((size_t)off.back() * 6);
            if (off.back() < 0 || off.back() > cap || (!pv.empty() && !st.pv.download(pv))) return;
            for (int b = 0; b < B; ++b) {
                if (status[b] != VIGO_GUIDE_OK) continue;
                vigo_host::installGuides(planners[who[b]]->optData_, rows.npts[b], off.data() + (size_t)b * N, pv.data());
                done[who[b]] = 1;
            }
        });
    }
    long long nDone = 0, nFound = 0;
    for (size_t i = 0; i < P; ++i) { nDone += done[i]; nFound += found[i] ? 1 : 0; }
    pb.stats.guidesDecided += nDone;
    pb.stats.guidesHost += nFound - nDone;
    parallelFor(P, [&](size_t i) {
        if (found[i] && !done[i]) planners[i]->assignGuidesCore();
    });
}

// the planners vigo_rebound_reguide works on (vigo.h): what is left of the NEEDS_HOST ones is the forced A* of
// failCount >= 4 and the planners with a dynamic collision only
bool bsplineTraj::reguideEligible(const Rebound& r) { return r.devStatus == VIGO_RB_NEEDS_HOST && r.gateStatic && r.failCount < 4; }

// reboundStep for such a planner with the guide step's twin in place of assignGuidePointsSemiCircle: what
// vigo_rebound_reguide computes (csrc/vigo_reguide_core.hpp restates isReguideRequired, vigo_path_search the host's
// pathSearch), without its capacities
void bsplineTraj::reguideStepCore(Rebound& r, PlanBatch& pb) {
    if (pb.o.reguideStepLog) {
        ReguideStepRecord rec;
        rec.N = this->optData_.controlPoints.cols();
        rec.ctrl.assign(this->optData_.controlPoints.data(), this->optData_.controlPoints.data() + 3 * (size_t)rec.N);
        rec.goff.assign(1, 0);
        vigo_host::appendGuides(this->optData_, rec.N, rec.goff, rec.gpv);
        for (const auto& s : this->collisionSeg_) { rec.seg.push_back(s.first); rec.seg.push_back(s.second); }
        rec.failCount = r.failCount;
        rec.gateDynamic = r.gateDynamic ? 1 : 0;
        const double w[4] = {this->weightDistance_, this->weightSmoothness_, this->weightFeasibility_, this->weightDynamicObstacle_};
        std::copy(w, w + 4, rec.weights);
        std::lock_guard<std::mutex> lock(pb.logMutex);
        pb.o.reguideStepLog->push_back(std::move(rec));
    }
    std::vector<std::pair<int, int>> reguideCollisionSeg;
    std::vector<std::vector<Eigen::Vector3d>> paths;
    if (this->isReguideRequired(reguideCollisionSeg) && this->pathSearch(reguideCollisionSeg, paths)) {
        this->astarPaths_ = paths;
        this->assignGuidesCoreOn(reguideCollisionSeg, paths);
    } else {
        this->weightDistance_ *= 2.0;
        ++r.failCount;
    }
    if (r.gateDynamic) this->weightDynamicObstacle_ *= 2.0;
    r.needOptimize = true;
}

// deviceReguide = 1: per group of planners that share a batch key and a node pool, the eligible ones as one staged
// batch (control points, guide CSR, weights, state) through vigo_rebound_reguide, one round of downloads, the results
// installed per planner.  pairCap: the old pairs plus four new ones per control point on average over the group, and
// pointCap two full-length paths per planner, are budgets as in prologueOnDevice: a group over either gets
// VIGO_ERR_INVALID_ARG (nothing written, the message is printed) and runs the twin on the workers.
void bsplineTraj::reguideOnDevice(PlanBatch& pb, const std::vector<uint8_t>& devOk) {
    std::vector<bsplineTraj*>& active = pb.active;
    std::vector<size_t> owners;
    for (size_t a = 0; a < active.size(); ++a)
        if (devOk[a] && reguideEligible(pb.rb[pb.activeIdx[a]]) && active[a]->collisionSeg_.size() <= (size_t)VIGO_MAX_COLLISION_SEGS) owners.push_back(a);
    long long nDecided = 0;
    SearchGroup::forEach(active, owners, true, pb.o.mixedPrologue, [&](bsplineTraj* lead, const SearchGroup& g, const std::vector<size_t>& who) {
        const int N = g.N, B = (int)who.size();           // (mixedPrologue: rows of the group's largest count, as deviceRounds stages them)
        if (N > VIGO_MAX_CTRL_POINTS) return;
        HostBatch hb(N);
        std::vector<vigo_rebound_state_t> state;
        for (size_t a : who) {
            const bsplineTraj* p = active[a];
            const Rebound& r = pb.rb[pb.activeIdx[a]];
            hb.add(p->optData_.controlPoints.data(), (int)p->optData_.controlPoints.cols(), p->optData_,
                   {p->weightDistance_, p->weightSmoothness_, p->weightFeasibility_, p->weightDynamicObstacle_});
            vigo_rebound_state_t st;
            std::memset(&st, 0, sizeof(st));
            st.status = VIGO_RB_NEEDS_HOST;
            st.lbfgs_status = p->lastStatus_;
            st.fail_count = r.failCount;
            st.gate_static = 1;
            st.gate_dynamic = r.gateDynamic ? 1 : 0;
            st.n_seg = (int32_t)p->collisionSeg_.size();
            for (int q = 0; q < st.n_seg; ++q) { st.seg[2 * q] = p->collisionSeg_[q].first; st.seg[2 * q + 1] = p->collisionSeg_[q].second; }
            state.push_back(st);
        }
        const long long segCap = (long long)B * VIGO_MAX_COLLISION_SEGS, pointCap = (long long)B * 2 * (kAstarPathCap + 1),
                        pairCap = (long long)hb.guides() + (long long)B * N * 4;
        static thread_local ReguideStage dv;
        vigo_handle_t h = lead->link_.handle();
        std::vector<int32_t> status(B), off((size_t)B * N + 1), pathSegOff(B + 1);
        DeviceBatch d;
        if (!uploadBatch(h, hb, d) || !dv.state.upload(state) || !dv.off.alloc(off.size()) || !dv.pv.alloc((size_t)pairCap * 6) ||
            !dv.pathSegOff.alloc(pathSegOff.size()) || !dv.pathOff.alloc((size_t)segCap + 1) || !dv.path.alloc((size_t)pointCap * 3) ||
            !dv.status.alloc(status.size()))
            return;
        pb.stats.reguideGroups += 1;
        // (no pairs at all: "no guides")
        if (d.npts ? !deviceCallOk(vigo_rebound_reguide_mixed(h, B, N, d.npts, d.ctrl, d.gpv ? d.goff : nullptr, d.gpv, d.gunk, d.weights,
                                                              lead->notCheckRatio_, g.res, g.pool, lead->minHeight_, lead->maxHeight_, pb.o.deviceAstarBudget,
                                                              kAstarPathCap, dv.state.get(), pairCap, dv.off.get(), dv.pv.get(), nullptr, segCap, pointCap,
                                                              dv.pathSegOff.get(), dv.pathOff.get(), dv.path.get(), dv.status.get()),
                                   "vigo_rebound_reguide_mixed", h)
                   : !deviceCallOk(vigo_rebound_reguide(h, B, N, d.ctrl, d.gpv ? d.goff : nullptr, d.gpv, d.gunk, d.weights,
                                                        lead->notCheckRatio_, g.res, g.pool, lead->minHeight_, lead->maxHeight_, pb.o.deviceAstarBudget,
                                                        kAstarPathCap, dv.state.get(), pairCap, dv.off.get(), dv.pv.get(), nullptr, segCap, pointCap,
                                                        dv.pathSegOff.get(), dv.pathOff.get(), dv.path.get(), dv.status.get()),
                                   "vigo_rebound_reguide", h))
            return;
        if (!vigo_host::threadSync() || !dv.status.download(status) || !dv.off.download(off) || !dv.pathSegOff.download(pathSegOff) ||
            !dv.state.download(state) || !batchStage().weights.download(hb.weights))
            return;
        const int S = pathSegOff[B];
        if (S < 0 || S > segCap || off.back() < 0 || off.back() > pairCap) return;
        std::vector<int32_t> pathOff;
        std::vector<double> path, pv;
        if (!downloadPathsAndPairs(S, pointCap, off.back(), dv.pathOff, dv.path, dv.pv, pathOff, path, pv)) return;
        for (int b = 0; b < B; ++b) {
            if (status[b] != VIGO_REGUIDE_DONE && status[b] != VIGO_REGUIDE_SEARCH_FAILED && status[b] != VIGO_REGUIDE_NOT_REQUIRED) continue;
            bsplineTraj* p = active[who[b]];
            Rebound& r = pb.rb[pb.activeIdx[who[b]]];
            const vigo_rebound_state_t& st = state[b];
            p->collisionSeg_.clear();
            for (int q = 0; q < st.n_seg; ++q) p->collisionSeg_.push_back({st.seg[2 * q], st.seg[2 * q + 1]});
            if (status[b] == VIGO_REGUIDE_DONE) {
                vigo_host::installPaths(p->astarPaths_, pathSegOff[b], pathSegOff[b + 1], pathOff.data(), path.data());
                // the merged CSR holds a control point's old pairs first: what follows them is this step's
                vigo_host::installGuides(p->optData_, hb.npts[b], off.data() + (size_t)b * N, pv.data(), true);
            }
            p->weightDistance_ = hb.weights[4 * (size_t)b + 0];
            p->weightDynamicObstacle_ = hb.weights[4 * (size_t)b + 3];
            r.failCount = st.fail_count;
            r.needOptimize = st.solve_first != 0;
            r.devStatus = st.status;                   // VIGO_RB_ACTIVE: the step is done
            ++nDecided;
        }
    });
    pb.stats.reguideDecided += nDecided;
}

// The loop runs on the device between two A* calls (vigo_rebound_rounds): gates, success exit, isReguideRequired,
// weight doubling and re-solve are queued for up to kRounds rounds without a host round trip; the host only sees
// the planners that are done, need A* (re-guide, or failCount >= 4) or ran out of queued rounds.  Under
// deviceReguide the re-guide step is vigo_rebound_reguide's (or its twin's on the workers).
void bsplineTraj::reboundOnDevice(PlanBatch& pb, bool timing) {
    const int kRounds = 4;   // failCount reaches 4 after at most four device rounds: then every round needs A*
    std::vector<bsplineTraj*>& active = pb.active;
    auto same = [&](size_t a, size_t b) { return active[a]->sameSolveGroup(*active[b], pb.o.mixedBatches); };
    const double t0 = wallSeconds();
    const double budget = 0.03 * std::max<size_t>(1, active.size());
    while (!active.empty()) {
        const double tr0 = wallSeconds();
        // one device batch per group of planners the lead's handle state fits (mixedBatches: whatever their counts,
        // within a shape class)
        std::vector<uint8_t> devOk(active.size(), 0);
        vigo_host::forEachGroup(active.size(), same, [&](const std::vector<size_t>& members) {
            std::vector<bsplineTraj*> grp;
            std::vector<Rebound*> grb;
            for (size_t m : members) {
                grp.push_back(active[m]);
                grb.push_back(&pb.rb[pb.activeIdx[m]]);
            }
            const bool ok = deviceRounds(grp, grb, kRounds, pb.o, pb.stats);
            for (size_t m : members) devOk[m] = ok ? 1 : 0;
        });
        const double tr1 = wallSeconds();
        const bool timedOut = wallSeconds() - t0 > budget;
        if (timedOut) {
            // BT.cpp:633-637: out of time.  The reference tests the budget right after the gates: the planners still
            // in the loop get one more gate (a trajectory that is collision free by now succeeds), the rest fail.
            // (gateBatch forms the same device batches as the rounds above)
            std::vector<uint8_t> col, dyn;
            gateBatch(active, col, dyn);
            for (size_t a = 0; a < active.size(); ++a) {
                Rebound& r = pb.rb[pb.activeIdx[a]];
                if (r.devStatus == VIGO_RB_DONE) continue;
                r.devStatus = (!col[a] && !dyn[a] && devOk[a]) ? VIGO_RB_DONE : VIGO_RB_NEEDS_HOST;
                r.gateStatic = col[a] != 0;
                r.gateDynamic = dyn[a] != 0;
            }
        }
        // the re-guide step of the planners the device takes (deviceReguide); out of time, every planner leaves below
        const int reguide = timedOut ? 0 : pb.o.deviceReguide;
        if (reguide == 1) reguideOnDevice(pb, devOk);
        size_t nHost = 0;
        long long nTwin = 0;
        for (size_t a = 0; a < active.size(); ++a) {
            nHost += pb.rb[pb.activeIdx[a]].devStatus == VIGO_RB_NEEDS_HOST ? 1 : 0;
            nTwin += reguide != 0 && devOk[a] && reguideEligible(pb.rb[pb.activeIdx[a]]) ? 1 : 0;
        }
        pb.stats.reguideHost += nTwin;
        parallelFor(active.size(), [&](size_t a) {
            Rebound& r = pb.rb[pb.activeIdx[a]];
            bsplineTraj* p = active[a];
            if (!devOk[a]) { p->reboundFinish(r, false); return; }             // no device: nothing to plan with
            if (r.devStatus == VIGO_RB_DONE) p->reboundFinish(r, true);          // BT.cpp:628-631
            else if (reguide != 0 && reguideEligible(r)) p->reguideStepCore(r, pb);  // what the device left, or setting 2: its twin
            else if (r.devStatus == VIGO_RB_NEEDS_HOST) p->reboundStep(r, r.gateStatic, r.gateDynamic, timedOut);   // A* and the rest of the pass
            // (still active: its next step is the gate, or the optimize() the device left for the next call)
        });
        const size_t n = active.size();
        retireFinished(pb);
        if (timing)
            cout << "[BsplineTraj]:   device rounds (<= " << kRounds << ") of " << n << ": " << (tr1 - tr0) * 1e3 << " ms, host step of "
                 << nHost << " planners " << (wallSeconds() - tr1) * 1e3 << " ms, " << active.size() << " continue" << endl;
    }
}

// The same loop driven round by round from the host (gates, one pass of the loop body, solve); the reference the
// device-resident loop is tested against.
void bsplineTraj::reboundFromHost(PlanBatch& pb, bool timing) {
    std::vector<bsplineTraj*>& active = pb.active;
    double tr0 = wallSeconds();
    solveBatch(active, pb.o, pb.stats);
    if (timing) cout << "[BsplineTraj]:   first solve of " << active.size() << ": " << (wallSeconds() - tr0) * 1e3 << " ms" << endl;
    const double t0 = wallSeconds();
    const double budget = 0.03 * std::max<size_t>(1, active.size());
    while (!active.empty()) {
        std::vector<uint8_t> col, dyn;
        tr0 = wallSeconds();
        gateBatch(active, col, dyn);
        const double tr1 = wallSeconds();
        const bool timedOut = wallSeconds() - t0 > budget;
        // one pass of the loop body per planner (validation outcome -> re-guide / weight doubling, BT.cpp:619-681):
        // planner-local, incl. the A* of a re-guide, so spread over the host cores
        parallelFor(active.size(), [&](size_t a) { active[a]->reboundStep(pb.rb[pb.activeIdx[a]], col[a] != 0, dyn[a] != 0, timedOut); });
        const size_t n = active.size();
        retireFinished(pb);
        std::vector<bsplineTraj*> solve;
        for (size_t a = 0; a < active.size(); ++a)
            if (pb.rb[pb.activeIdx[a]].needOptimize) solve.push_back(active[a]);
        const double tr2 = wallSeconds();
        solveBatch(solve, pb.o, pb.stats);
        if (timing)
            cout << "[BsplineTraj]:   round of " << n << ": gates " << (tr1 - tr0) * 1e3 << " ms, rebound step " << (tr2 - tr1) * 1e3
                 << " ms, solve of " << solve.size() << " " << (wallSeconds() - tr2) * 1e3 << " ms" << endl;
    }
}

// the planners whose loop has ended leave the active set; their result is the loop's
void bsplineTraj::retireFinished(PlanBatch& pb) {
    std::vector<bsplineTraj*> next;
    std::vector<size_t> nextIdx;
    for (size_t a = 0; a < pb.active.size(); ++a) {
        const Rebound& r = pb.rb[pb.activeIdx[a]];
        if (r.done) {
            pb.result[pb.activeIdx[a]] = r.ok;
            if (!r.ok) cout << "[BsplineTraj]: Fail because of optimizer not finding a solution." << endl;
        } else {
            next.push_back(pb.active[a]);
            nextIdx.push_back(pb.activeIdx[a]);
        }
    }
    pb.active.swap(next);
    pb.activeIdx.swap(nextIdx);
}

namespace {
constexpr int kFinishSampleCap = 2048;   // samples per trajectory the stage's buffers are sized for (a 7 m path at ts 0.1: ~110)
struct FinishStage {
    Staged<double> ctrl, limits, factor, pos, vel;
    Staged<int32_t> npts, n, status;
};
}  // namespace

// deviceEpilogue: per group of planners that share a device target, ts_ and controlPointsTs_ (the sample step
// of evalTrajToMsg(yaw) is ts_) — whatever their counts — the rows padded to the group's largest count, one
// vigo_traj_finish, one download; linearFactor_, bspline_ and the path installed.  What the call does not decide stays in todo.
void bsplineTraj::finishOnDevice(const std::vector<bsplineTraj*>& ps, std::vector<uint8_t>& todo, nav_msgs::Path* paths, bool yaw, BatchStats& stats) {
    std::vector<size_t> owners;
    for (size_t i = 0; i < ps.size(); ++i)
        if (todo[i]) owners.push_back(i);
    auto same = [&](size_t a, size_t b) {
        const bsplineTraj *x = ps[owners[a]], *y = ps[owners[b]];
        return x->link_.sameTarget(y->link_) && x->ts_ == y->ts_ && x->controlPointsTs_ == y->controlPointsTs_;
    };
    vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
        bsplineTraj* lead = ps[owners[members[0]]];
        std::vector<size_t> who;
        int Ns = 0;
        for (size_t m : members) {
            const int n = (int)ps[owners[m]]->optData_.controlPoints.cols();
            if (n < 7 || n > VIGO_MAX_CTRL_POINTS) continue;
            who.push_back(owners[m]);
            Ns = std::max(Ns, n);
        }
        if (who.empty() || !lead->syncDevice()) return;
        const double dt = lead->ts_;
        // the samples of the longest row, as far as the buffers go: a row with more is reported CAPACITY and stays with the host
        int S_cap = 1;
        if (paths) {
            S_cap = 0;
            const double longest = (Ns - 3) * lead->controlPointsTs_;
            if (!(dt > 0.0)) return;
            for (double t = 0.0; t <= longest && S_cap < kFinishSampleCap; t += dt) ++S_cap;
        }
        const bool wantVel = paths && yaw;
        HostBatch hb(Ns);
        std::vector<double> limits;
        for (size_t i : who) {
            hb.addRow(ps[i]->optData_.controlPoints.data(), (int)ps[i]->optData_.controlPoints.cols());
            limits.push_back(ps[i]->maxVel_);
            limits.push_back(ps[i]->maxAcc_);
        }
        const size_t B = who.size(), rows = B * (size_t)S_cap * 3;
        static thread_local FinishStage st;
        if (!st.ctrl.upload(hb.ctrl) || !st.limits.upload(limits) || (!hb.uniform() && !st.npts.upload(hb.npts)) || !st.factor.alloc(B) ||
            !st.n.alloc(B) || !st.status.alloc(B) || !st.pos.alloc(rows) || (wantVel && !st.vel.alloc(rows)))
            return;
        vigo_handle_t h = lead->link_.handle();
        stats.epilogueGroups += 1;
        if (!deviceCallOk(vigo_traj_finish(h, (int)B, Ns, hb.uniform() ? nullptr : st.npts.get(), st.ctrl.get(), st.limits.get(), dt, S_cap,
                                           st.factor.get(), nullptr, st.n.get(), st.pos.get(), wantVel ? st.vel.get() : nullptr, st.status.get()),
                          "vigo_traj_finish", h))
            return;
        std::vector<double> factor(B), pos(paths ? rows : 0), vel(wantVel ? rows : 0);
        std::vector<int32_t> n(B), status(B);
        if (!vigo_host::threadSync() || !st.factor.download(factor) || !st.n.download(n) || !st.status.download(status) ||
            (paths && !st.pos.download(pos)) || (wantVel && !st.vel.download(vel)))
            return;
        parallelFor(B, [&](size_t b) {
            // without paths one sample row is all the call was given: CAPACITY then says nothing about the factor
            if (status[b] != VIGO_FINISH_OK && !(status[b] == VIGO_FINISH_CAPACITY && !paths)) return;
            bsplineTraj* p = ps[who[b]];
            p->bspline_ = trajPlanner::bspline(bsplineDegree, p->optData_.controlPoints, p->controlPointsTs_);  // step 5
            p->linearFactor_ = factor[b];                                                                    // step 6
            if (paths) {
                std::vector<Eigen::Vector3d> pts;
                const double* q = pos.data() + b * (size_t)S_cap * 3;
                for (int i = 0; i < n[b]; ++i) pts.push_back(Eigen::Vector3d(q[3 * i], q[3 * i + 1], q[3 * i + 2]));
                nav_msgs::Path& traj = paths[who[b]];
                p->eigenPointsToPathMsg(pts, traj);
                const double* v = wantVel ? vel.data() + b * (size_t)S_cap * 3 : nullptr;
                for (int i = 0; v && i < n[b]; ++i)   // BT.cpp:1512, on the velocity the device evaluated at (double)i * dt
                    traj.poses[i].pose.orientation = trajPlanner::quaternion_from_rpy(0, 0, std::atan2(v[3 * i + 1], v[3 * i]));
            }
            todo[who[b]] = 0;
        });
    });
}

// steps 5-6 for the planners that succeeded, and with `paths` their evalTrajToMsg(yaw)
void bsplineTraj::planEpilogue(const std::vector<bsplineTraj*>& planners, const std::vector<bool>& result, nav_msgs::Path* paths, bool yaw,
                               const BatchOptions& o, BatchStats& stats) {
    std::vector<uint8_t> todo(result.begin(), result.end());   // the planners the host route below still owes
    if (o.deviceEpilogue) {
        long long want = 0, left = 0;
        for (uint8_t t : todo) want += t;
        finishOnDevice(planners, todo, paths, yaw, stats);
        for (uint8_t t : todo) left += t;
        stats.epilogueDecided += want - left;
        stats.epilogueHost += left;
    }
    parallelFor(planners.size(), [&](size_t i) {
        if (!todo[i]) return;
        bsplineTraj* p = planners[i];
        p->bspline_ = trajPlanner::bspline(bsplineDegree, p->optData_.controlPoints, p->controlPointsTs_);  // step 5
        p->linearFeasibilityReparam();                                                                  // step 6
        if (paths) paths[i] = p->evalTrajToMsg(yaw);
    });
}

void bsplineTraj::finishBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>* trajectories, bool yaw, const BatchOptions& options,
                              BatchStats* stats) {
    if (trajectories) trajectories->assign(planners.size(), nav_msgs::Path());
    BatchStats st;
    planEpilogue(planners, std::vector<bool>(planners.size(), true), trajectories ? trajectories->data() : nullptr, yaw, options.normalized(), st);
    reportBatchStats(st, stats);
}

void bsplineTraj::finishBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>* trajectories, bool yaw) {
    finishBatch(planners, trajectories, yaw, defaultBatchOptions());
}

namespace {
struct ValidateStage {
    Staged<double> ctrl, obs, pos;
    Staged<int32_t> npts, ooff, status, first;
};
}  // namespace

// isCurrTrajValidBatch's device stage: per group of planners that share a device target, maxVel_ (the gate step) and
// notCheckRatio_ — whatever their counts — the rows padded to the group's largest count, the obstacle lists as one CSR, one
// vigo_traj_validate under the index rule, one download.  What the call does not decide stays in todo.
void bsplineTraj::validateOnDevice(const std::vector<bsplineTraj*>& ps, std::vector<uint8_t>& todo, std::vector<bool>& valid,
                                   std::vector<Eigen::Vector3d>* firstCollisionPos, std::vector<bool>* dynamicCollision, BatchStats& stats) {
    std::vector<size_t> owners;
    for (size_t i = 0; i < ps.size(); ++i)
        if (todo[i]) owners.push_back(i);
    auto same = [&](size_t a, size_t b) { return ps[owners[a]]->sameBatchKeyAnyCount(*ps[owners[b]]); };
    vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
        std::vector<size_t> who;
        int Ns = 0;
        for (size_t m : members) {
            const int n = (int)ps[owners[m]]->optData_.controlPoints.cols();
            if (n < 4 || n > VIGO_MAX_CTRL_POINTS) continue;
            who.push_back(owners[m]);
            Ns = std::max(Ns, n);
        }
        if (who.empty()) return;
        bsplineTraj* lead = ps[who[0]];
        if (!lead->syncDevice() || !lead->link_.map()) return;
        HostBatch hb(Ns);
        for (size_t i : who) {
            hb.addRow(ps[i]->optData_.controlPoints.data(), (int)ps[i]->optData_.controlPoints.cols());
            vigo_host::appendObstacles(ps[i]->optData_, hb.obs);
            hb.ooff.push_back((int32_t)(hb.obs.size() / 9));
        }
        const size_t B = who.size();
        static thread_local ValidateStage st;
        if (!st.ctrl.upload(hb.ctrl) || (!hb.uniform() && !st.npts.upload(hb.npts)) || !st.ooff.upload(hb.ooff) || !st.obs.upload(hb.obs) ||
            !st.status.alloc(B) || !st.first.alloc(B) || !st.pos.alloc(3 * B))
            return;
        vigo_handle_t h = lead->link_.handle();
        const double dt = lead->link_.map()->getRes() / lead->maxVel_ / 2.0;  // BT.h:312, evalTraj()'s step
        stats.validateGroups += 1;
        if (!deviceCallOk(vigo_traj_validate(h, (int)B, Ns, hb.uniform() ? nullptr : st.npts.get(), st.ctrl.get(), dt, lead->notCheckRatio_,
                                             VIGO_VALIDATE_BY_INDEX, st.ooff.get(), hb.obs.empty() ? nullptr : st.obs.get(), 0, st.status.get(),
                                             st.first.get(), st.pos.get(), nullptr, nullptr, nullptr),
                          "vigo_traj_validate", h))
            return;
        std::vector<int32_t> status(B);
        std::vector<double> pos(3 * B);
        if (!vigo_host::threadSync() || !st.status.download(status) || !st.pos.download(pos)) return;
        for (size_t b = 0; b < B; ++b) {
            if (status[b] & VIGO_VALID_BAD_COUNT) continue;
            const size_t i = who[b];
            valid[i] = !(status[b] & VIGO_VALID_STATIC);
            if (!valid[i] && firstCollisionPos) (*firstCollisionPos)[i] = Eigen::Vector3d(pos[3 * b], pos[3 * b + 1], pos[3 * b + 2]);
            if (dynamicCollision) (*dynamicCollision)[i] = (status[b] & VIGO_VALID_DYNAMIC) != 0;
            todo[i] = 0;
        }
    });
}

std::vector<bool> bsplineTraj::isCurrTrajValidBatch(const std::vector<bsplineTraj*>& planners, std::vector<Eigen::Vector3d>* firstCollisionPos,
                                                    std::vector<bool>* dynamicCollision, BatchStats* stats) {
    const size_t n = planners.size();
    std::vector<bool> valid(n, false);
    if (firstCollisionPos && firstCollisionPos->size() != n) firstCollisionPos->resize(n, Eigen::Vector3d(0.0, 0.0, 0.0));
    if (dynamicCollision) dynamicCollision->assign(n, false);
    BatchStats st;
    std::vector<uint8_t> todo(n, 0);    // the planners the per-planner route below still owes
    long long want = 0, left = 0;
    for (size_t i = 0; i < n; ++i) todo[i] = planners[i]->init_ ? 1 : 0, want += todo[i];
    validateOnDevice(planners, todo, valid, firstCollisionPos, dynamicCollision, st);
    for (size_t i = 0; i < n; ++i) {
        if (!todo[i]) continue;
        ++left;
        bsplineTraj* p = planners[i];
        Eigen::Vector3d hit;
        valid[i] = p->isCurrTrajValid(hit);
        if (!valid[i] && firstCollisionPos) (*firstCollisionPos)[i] = hit;
        if (dynamicCollision) (*dynamicCollision)[i] = p->hasDynamicCollisionTrajectory(p->optData_.controlPoints);
    }
    st.validateDecided = want - left;
    st.validateHost = left;
    reportBatchStats(st, stats);
    return valid;
}

}  // namespace trajPlanner
