// cabiPlanBatch.cpp — vigo_host_plan_batch and the pieces it shares with cabi_host.cpp (cabiPlanBatch.h)
#ifdef VIGO_WITH_ROS
#error "tools of the in-tree dense map (standin/dense_occmap.h): not part of a build against map_manager"
#endif
#include "cabiPlanBatch.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <future>
#include <thread>

#include "../../../include/vigo.h"
#include "batchLayout.h"
#include "workerPool.h"

extern "C" int vigo_host_rebound_reguide_core(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                                              const int* guide_off, const double* guide_pv, const unsigned char* guide_unk, const double* weights,
                                              double traj_time, double dist_threshold, double step, const int* pool, double min_height, double max_height,
                                              int cap_log2, int max_nodes, int heap_cap, int max_expansions, int astar_path_cap, int guide_path_cap, int mode,
                                              vigo_rebound_state_t* state, long long pair_cap, int* out_guide_off, double* out_guide_pv,
                                              unsigned char* out_guide_unk, int out_seg_cap, int out_path_cap, int* out_path_seg_off, int* out_path_off,
                                              double* out_path, int* out_status);

namespace cabi {

std::shared_ptr<mapManager::occMap> denseMap(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels) {
    auto map = std::make_shared<mapManager::occMap>(nx, ny, nz, Eigen::Vector3d(origin[0], origin[1], origin[2]), res);
    std::memcpy(map->voxels().data(), voxels, (size_t)nx * ny * nz);
    return map;
}

void setBsplineParams(ros::NodeHandle& nh, const double* cfg) {
    nh.setParam("bspline_traj/distance_threshold", cfg[0]);
    nh.setParam("bspline_traj/min_height", cfg[1]);
    nh.setParam("bspline_traj/max_height", cfg[2]);
    nh.setParam("bspline_traj/max_obstacle_size", std::vector<double>{cfg[3], cfg[4], cfg[5]});
}

void nodePool(const double* cfg, double res, int pool[3]) {
    for (int a = 0; a < 3; ++a) pool[a] = 2 * int(cfg[3 + a] / res);
}

nav_msgs::Path pathFromXyz(const double* q, int n_pts) {
    nav_msgs::Path path;
    for (int i = 0; i < n_pts; ++i) {
        geometry_msgs::PoseStamped ps;
        ps.pose.position.x = q[3 * i]; ps.pose.position.y = q[3 * i + 1]; ps.pose.position.z = q[3 * i + 2];
        path.poses.push_back(ps);
    }
    return path;
}

BatchFixture::BatchFixture(const unsigned char* vox, const int* dims, const double* origin, double res, const double* cfg, int n, const int* path_off,
                           const double* path_xyz, const unsigned char* vox2, int n_maps, const int* planner_device, const double* planner_timestep)
    : cond(n, std::vector<Eigen::Vector3d>(4, Eigen::Vector3d(0, 0, 0))) {
    for (int k = 0; k < n_maps; ++k) maps.push_back(denseMap(dims[0], dims[1], dims[2], origin, res, (vox2 && (k & 1)) ? vox2 : vox));
    setBsplineParams(nh, cfg);
    nh.setParam("bspline_traj/max_path_length", 1000.0);
    nh.setParam("bspline_traj/plan_in_z_axis", 0.0);
    for (int t = 0; t < n; ++t) in.push_back(pathFromXyz(path_xyz + (size_t)path_off[t] * 3, path_off[t + 1] - path_off[t]));
    if (planner_device) device.assign(planner_device, planner_device + n);
    for (int t = 0; planner_timestep && t < n; ++t) {
        stepNh.push_back(nh);
        if (std::isnan(planner_timestep[t])) continue;
        stepNh.back() = ros::NodeHandle();            // (a copy of a NodeHandle shares its parameters: copy the map itself)
        *stepNh.back().params = *nh.params;
        stepNh.back().setParam("bspline_traj/timestep", planner_timestep[t]);
    }
}

FreshPlanners freshPlanners(const BatchFixture& fx) {
    FreshPlanners fp;
    for (size_t t = 0; t < fx.in.size(); ++t) {
        fp.owners.emplace_back(new bsplineTraj(fx.stepNh.empty() ? fx.nh : fx.stepNh[t]));
        if (!fx.device.empty() && fx.device[t] >= 0) fp.owners.back()->setDevice(fx.device[t]);
        fp.owners.back()->setMap(fx.maps[t % fx.maps.size()]);
        fp.owners.back()->updateMaxVel(2.0);
        fp.owners.back()->updateMaxAcc(3.0);
        fp.ps.push_back(fp.owners.back().get());
    }
    bsplineTraj::updatePathBatch(fp.ps, fx.in, fx.cond);
    return fp;
}

std::vector<bool> timedPlan(const std::vector<bsplineTraj*>& ps, double& ms, std::vector<nav_msgs::Path>* traj, bool yaw) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<bool> planned = traj ? bsplineTraj::makePlanBatch(ps, *traj, yaw) : bsplineTraj::makePlanBatch(ps);
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return planned;
}
std::vector<bool> timedPlan(const std::vector<bsplineTraj*>& ps, const bsplineTraj::BatchOptions& o, double& ms, bsplineTraj::BatchStats& st,
                            std::vector<nav_msgs::Path>* traj, bool yaw) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<bool> planned = traj ? bsplineTraj::makePlanBatch(ps, *traj, yaw, o, &st) : bsplineTraj::makePlanBatch(ps, o, &st);
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return planned;
}

int dumpSlot(const std::vector<bsplineTraj*>& ps, const std::vector<bool>& planned, int slot, const vigo_host_plan_batch_job_t& out) {
    const size_t n = ps.size();
    const long long cap = out.cap;
    long long g = 0, w = 0, sg = 0;
    for (size_t t = 0; t < n; ++t) {
        const size_t o = (size_t)slot * n + t;
        const Eigen::MatrixXd c = ps[t]->getControlPoints();
        if (out.ok) out.ok[o] = planned[t] ? 1 : 0;
        if (out.solver) out.solver[o] = ps[t]->getLastSolverStatus();
        if (out.ncp) out.ncp[o] = (int)c.cols();
        if (out.factor) out.factor[o] = ps[t]->getLinearFactor();
        if (out.ctrl) {
            if (c.cols() > out.ncp_cap) return -2;
            for (int i = 0; i < (int)c.cols(); ++i) for (int k = 0; k < 3; ++k) out.ctrl[(o * out.ncp_cap + i) * 3 + k] = c(k, i);
        }
        if (out.guides) {
            std::vector<int32_t> off{0};
            std::vector<double> pv;
            vigo_host::appendGuides(ps[t]->getOptData(), (int)c.cols(), off, pv);
            out.n_guides[o] = (int)(pv.size() / 6);
            if (g + (long long)pv.size() / 6 > cap) return -2;
            std::memcpy(out.guides + ((size_t)slot * cap + g) * 6, pv.data(), pv.size() * sizeof(double));
            g += (long long)pv.size() / 6;
        }
        if (out.segs) {
            const auto& cs = ps[t]->getCollisionSeg();
            out.n_seg[o] = (int)cs.size();
            if (sg + (long long)cs.size() > cap) return -2;
            for (const auto& s : cs) { out.segs[((size_t)slot * cap + sg) * 2] = s.first; out.segs[((size_t)slot * cap + sg) * 2 + 1] = s.second; ++sg; }
        }
        if (out.paths) {
            int pts = 0;
            for (const auto& path : ps[t]->getAstarPaths())
                for (const auto& v : path) {
                    if (w + 1 > cap) return -2;
                    for (int k = 0; k < 3; ++k) out.paths[((size_t)slot * cap + w) * 3 + k] = v(k);
                    ++w; ++pts;
                }
            out.n_path_pts[o] = pts;
        }
    }
    return 0;
}

int dumpPoses(const std::vector<nav_msgs::Path>& traj, size_t n, int slot, int pose_cap, int* n_poses, double* pos, double* quat) {
    for (size_t t = 0; t < n; ++t) {
        const size_t o = (size_t)slot * n + t;
        n_poses[o] = t < traj.size() ? (int)traj[t].poses.size() : 0;
        if (n_poses[o] > pose_cap) return -2;
        for (int i = 0; i < n_poses[o]; ++i) {
            const auto& ps = traj[t].poses[i].pose;
            double* p = pos + (o * pose_cap + i) * 3;
            double* q = quat + (o * pose_cap + i) * 4;
            p[0] = ps.position.x; p[1] = ps.position.y; p[2] = ps.position.z;
            q[0] = ps.orientation.x; q[1] = ps.orientation.y; q[2] = ps.orientation.z; q[3] = ps.orientation.w;
        }
    }
    return 0;
}

void statCounts(const bsplineTraj::BatchStats& s, long long* out) {
    const long long v[kStatCounts] = {s.astarDecided,    s.astarHost,      s.guidesDecided,  s.guidesHost,     s.prologueDecided,
                                      s.prologueHost,    s.reguideDecided, s.reguideHost,    s.epilogueDecided, s.epilogueHost,
                                      s.seedDecided,     s.seedHost,       s.epilogueGroups, s.solveBatches,   s.solvePlanners,
                                      s.prologueGroups,  s.reguideGroups,  s.validateDecided, s.validateHost,  s.validateGroups};
    std::copy(v, v + kStatCounts, out);
}

bsplineTraj::BatchOptions optionsOfMask(int mask, int budget) {
    bsplineTraj::BatchOptions o;
    o.deviceAstar = (mask & 1) != 0;
    o.deviceGuides = (mask >> 1) & 3;
    o.devicePrologue = (mask & 8) != 0;
    o.deviceReguide = (mask >> 4) & 3;
    o.mixedBatches = (mask & 64) != 0;
    o.deviceEpilogue = (mask & 128) != 0;
    o.mixedPrologue = (mask & 256) != 0;
    o.deviceAstarBudget = budget;
    return o;
}

void setDefaults(const bsplineTraj::BatchOptions& o) {
    bsplineTraj::setDeviceAstar(o.deviceAstar);
    bsplineTraj::setDeviceGuides(o.deviceGuides);
    bsplineTraj::setDevicePrologue(o.devicePrologue);
    bsplineTraj::setDeviceReguide(o.deviceReguide);
    bsplineTraj::setMixedBatches(o.mixedBatches);
    bsplineTraj::setDeviceEpilogue(o.deviceEpilogue);
    bsplineTraj::setMixedPrologue(o.mixedPrologue);
    bsplineTraj::setDeviceAstarBudget(o.deviceAstarBudget);
}

}  // namespace cabi

namespace {
using namespace cabi;
using Job = vigo_host_plan_batch_job_t;

bool goodJob(const Job& j) {
    if (!j.vox || !j.dims || !j.origin || !j.cfg || !j.path_off || !j.path_xyz || !j.slot_mask || !j.slot_budget || !j.slot_route || !j.run_slot) return false;
    if (j.n < 1 || j.n_maps < 1 || j.n_slots < 1 || j.n_runs < 1 || !(j.res > 0.0) || j.ncp_cap < 0 || j.cap < 0 || j.pose_cap < 0) return false;
    if ((j.segs && !j.n_seg) || (j.paths && !j.n_path_pts) || (j.guides && !j.n_guides) || (j.n_poses && (!j.pos || !j.quat))) return false;
    for (int t = 0; t < j.n; ++t)
        if (j.path_off[t + 1] - j.path_off[t] < 2 || (j.planner_timestep && j.planner_timestep[t] <= 0.0)) return false;     // (NaN: as cfg)
    for (int s = 0; s < j.n_slots; ++s)
        if (j.slot_mask[s] < 0 || j.slot_mask[s] >= 512 || j.slot_route[s] < 0 || j.slot_route[s] > 2 || (j.slot_route[s] == 2 && j.slot_mask[s] != 0))
            return false;
    for (int r = 0; r < j.n_runs; ++r)
        if (j.run_slot[r] < 0 || j.run_slot[r] >= j.n_slots) return false;
    if (j.replay_slot < -1 || j.replay_slot >= j.n_slots) return false;
    if (j.replay_slot >= 0 && (j.concurrent || !j.twin || j.slot_route[j.replay_slot] != 0)) return false;
    if (j.concurrent && (j.n_runs != 2 || j.run_slot[0] == j.run_slot[1] || j.slot_route[j.run_slot[0]] != 0 || j.slot_route[j.run_slot[1]] != 0)) return false;
    return true;
}

// one run: its planners, what the call returned, and what its stages did
struct Run {
    FreshPlanners fp;
    std::vector<bool> planned;
    std::vector<nav_msgs::Path> traj;
    std::vector<bsplineTraj::ReguideStepRecord> log;
    long long counts[kStatCounts];
    double seconds[3];
};

// what the stats moved by from a to b: the counts, and seconds[0..1]
void moved(const bsplineTraj::BatchStats& a, const bsplineTraj::BatchStats& b, long long* counts, double* seconds = nullptr) {
    long long ca[kStatCounts];
    statCounts(a, ca);
    statCounts(b, counts);
    for (int k = 0; k < kStatCounts; ++k) counts[k] -= ca[k];
    if (!seconds) return;
    seconds[0] = b.prologueSeconds - a.prologueSeconds;
    seconds[1] = b.chainSeconds - a.chainSeconds;
}

void plan(const Job& j, int slot, bool logSteps, Run& r) {
    bsplineTraj::BatchOptions o = optionsOfMask(j.slot_mask[slot], j.slot_budget[slot]);
    if (logSteps) o.reguideStepLog = &r.log;
    std::vector<nav_msgs::Path>* traj = j.with_paths ? &r.traj : nullptr;
    double ms = 0.0;
    if (j.slot_route[slot] == 0) {
        bsplineTraj::BatchStats st;
        r.planned = timedPlan(r.fp.ps, o, ms, st, traj, j.yaw != 0);
        moved(bsplineTraj::BatchStats(), st, r.counts, r.seconds);
        r.seconds[2] = ms * 1e-3;
        return;
    }
    struct PutBack {
        bool on;
        ~PutBack() { if (on) setDefaults(bsplineTraj::BatchOptions()); }
    } putBack{j.slot_route[slot] == 1};
    const bsplineTraj::BatchStats before = bsplineTraj::batchTotals();
    if (putBack.on) setDefaults(o);
    r.planned = timedPlan(r.fp.ps, ms, traj, j.yaw != 0);
    moved(before, bsplineTraj::batchTotals(), r.counts, r.seconds);
    r.seconds[2] = ms * 1e-3;
}

// the results of a slot's last run
int dump(const Job& j, int slot, const Run& r) {
    if (j.stats) std::copy(r.counts, r.counts + kStatCounts, j.stats + (size_t)slot * kStatCounts);
    const int rc = dumpSlot(r.fp.ps, r.planned, slot, j);
    return rc == 0 && j.n_poses ? dumpPoses(r.traj, (size_t)j.n, slot, j.pose_cap, j.n_poses, j.pos, j.quat) : rc;
}

// the logged steps, one by one (a trajectory's result does not depend on its batch), by the kernels' twin
void replay(const Job& j, std::vector<bsplineTraj::ReguideStepRecord>& log) {
    int pool[3];
    nodePool(j.cfg, j.res, pool);
    std::vector<int> deferred(log.size(), 0);
    vigo_host::parallelFor(log.size(), [&](size_t k) {
        bsplineTraj::ReguideStepRecord& R = log[k];
        vigo_rebound_state_t st;
        std::memset(&st, 0, sizeof(st));
        st.status = VIGO_RB_NEEDS_HOST;
        st.gate_static = 1;
        st.gate_dynamic = R.gateDynamic;
        st.fail_count = R.failCount;
        st.n_seg = (int)std::min<size_t>(R.seg.size() / 2, VIGO_MAX_COLLISION_SEGS);
        std::copy(R.seg.begin(), R.seg.begin() + 2 * st.n_seg, st.seg);
        if (R.seg.size() / 2 > (size_t)VIGO_MAX_COLLISION_SEGS) { deferred[k] = 1; return; }   // (the facade keeps these off the device)
        const long long pairCap = (long long)R.gpv.size() / 6 + (long long)R.N * (VIGO_MAX_COLLISION_SEGS + 4);
        std::vector<int> off((size_t)R.N + 1);
        std::vector<double> pv((size_t)pairCap * 6 + 6);
        R.gpv.resize(R.gpv.size() + 6);
        int status = VIGO_REGUIDE_DEFERRED;
        const int r = vigo_host_rebound_reguide_core(j.vox, j.dims, j.origin, j.res, 1, R.N, R.ctrl.data(), R.goff.data(), R.gpv.data(), nullptr, R.weights,
                                                     0.0, j.cfg[0], j.res, pool, j.cfg[1], j.cfg[2], j.caps[0], j.caps[1], j.caps[2],
                                                     j.slot_budget[j.replay_slot], 128, j.caps[3], 1, &st, pairCap, off.data(), pv.data(), nullptr, 0, 0,
                                                     nullptr, nullptr, nullptr, &status);
        deferred[k] = (r != 0 || status == VIGO_REGUIDE_DEFERRED) ? 1 : 0;
    });
    j.twin[0] = (long long)log.size();
    j.twin[1] = (long long)std::count(deferred.begin(), deferred.end(), 0);
}

// two runs at the same time: each thread makes its planners (their handles with them), waits for the other to have done
// so, and plans
int planTwoAtOnce(const Job& j, const BatchFixture* fx[2]) {
    Run run[2];
    bool threw[2] = {false, false};
    std::promise<void> ready[2];
    std::shared_future<void> other[2] = {ready[1].get_future().share(), ready[0].get_future().share()};
    auto work = [&](int c) {
        try {
            run[c].fp = freshPlanners(*fx[c]);
        } catch (...) { threw[c] = true; }
        ready[c].set_value();
        other[c].wait();
        if (threw[0] || threw[1]) return;
        try {
            plan(j, j.run_slot[c], false, run[c]);
        } catch (...) { threw[c] = true; }
    };
    std::thread a(work, 0), b(work, 1);
    a.join();
    b.join();
    if (threw[0] || threw[1]) return -3;
    int rc = 0;
    for (int c = 0; c < 2 && rc == 0; ++c) {
        if (j.seconds) std::copy(run[c].seconds, run[c].seconds + 3, j.seconds + 3 * c);
        rc = dump(j, j.run_slot[c], run[c]);
    }
    return rc;
}

int planInTurn(const Job& j, const BatchFixture& fx) {
    std::vector<int> lastRun(j.n_slots, -1);
    for (int r = 0; r < j.n_runs; ++r) lastRun[j.run_slot[r]] = r;
    for (int r = 0; r < j.n_runs; ++r) {
        const int slot = j.run_slot[r];
        const bool last = lastRun[slot] == r, logged = last && slot == j.replay_slot;
        Run run;
        run.fp = freshPlanners(fx);
        plan(j, slot, logged, run);
        if (j.seconds) std::copy(run.seconds, run.seconds + 3, j.seconds + 3 * (size_t)r);
        if (logged) replay(j, run.log);
        const int rc = last ? dump(j, slot, run) : 0;
        if (rc != 0) return rc;
    }
    return 0;
}
}  // namespace

extern "C" {

int vigo_host_plan_batch_job_size(void) { return (int)sizeof(vigo_host_plan_batch_job_t); }

int vigo_host_plan_batch(const vigo_host_plan_batch_job_t* job) {
    if (!job || job->size != (int)sizeof(*job) || !goodJob(*job)) return -1;
    const Job& j = *job;
    if (j.twin) j.twin[0] = j.twin[1] = 0;
    try {
        std::unique_ptr<BatchFixture> fx[2];
        for (int c = 0; c < (j.concurrent ? 2 : 1); ++c)
            fx[c].reset(new BatchFixture(j.vox, j.dims, j.origin, j.res, j.cfg, j.n, j.path_off, j.path_xyz, j.vox2, j.n_maps, j.planner_device,
                                         j.planner_timestep));
        const bsplineTraj::BatchStats before = bsplineTraj::batchTotals();     // (making the planners below counts nothing)
        const BatchFixture* both[2] = {fx[0].get(), fx[1].get()};
        const int rc = j.concurrent ? planTwoAtOnce(j, both) : planInTurn(j, *fx[0]);
        if (rc != 0) return rc;
        if (j.totals) moved(before, bsplineTraj::batchTotals(), j.totals);
    } catch (...) {
        return -3;
    }
    return 0;
}

int vigo_host_switches(void) {
    return (bsplineTraj::deviceAstar() ? 1 : 0) | (bsplineTraj::deviceGuides() << 1) | (bsplineTraj::devicePrologue() ? 8 : 0) |
           (bsplineTraj::deviceReguide() << 4) | (bsplineTraj::mixedBatches() ? 64 : 0) | (bsplineTraj::deviceEpilogue() ? 128 : 0) |
           (bsplineTraj::mixedPrologue() ? 256 : 0);
}

}  // extern "C"
