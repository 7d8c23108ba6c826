// bsplineTraj.cpp — trajPlanner::bsplineTraj over the MI355X back-end.
//
// Behaviour follows the reference's bsplineTraj.{h,cpp} (cited per function as BT.cpp / BT.h);
// the numerics of optimize(), the collision gates and isUnknown(guide) run in libvigo_hip.so
// through the C ABI of include/vigo.h.  Own implementation: host bookkeeping only.
#include <trajectory_planner/bsplineTraj.h>
#include <trajectory_planner/polyTrajOccMap.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <cstdlib>
#include <cmath>
#include <fstream>
#include <cstring>
#include <iostream>
#include <set>

#include "../../../include/vigo.h"
#include "../../csrc/vigo_guide_core.hpp"
#include "../../csrc/vigo_pathsearch_core.hpp"
#include "batchLayout.h"
#include "devbuf.h"
#include "workerPool.h"

using std::cout;
using std::endl;

namespace {

using vigo_host::StagingBuf;

using vigo_host::parallelFor;

double wallSeconds() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

#ifndef VIGO_WITH_ROS
ros::Time ros::Time::now() {
    ros::Time t;
    t.sec = wallSeconds();
    return t;
}
#endif

namespace trajPlanner {

// The reference keeps the length of the previous call's path in a function-static shared by all instances (BT.cpp:755):
// kept here as one process-wide value, read and written through adjustPathLengthWith so that updatePathBatch can run
// the planners' prologues on several host threads and still hand every planner the value its predecessor left.
// (atomic only so that two host threads planning two batches do not race on it formally; WHICH value a planner of one
// batch sees when another batch runs at the same time is as unspecified as it is for the reference's static)
namespace {
std::atomic<double> g_prevPathLength{0.0};
}


bsplineTraj::bsplineTraj() {}

bsplineTraj::bsplineTraj(const ros::NodeHandle& nh) : nh_(nh) { this->initParam(); }

bsplineTraj::~bsplineTraj() {}

void bsplineTraj::init(const ros::NodeHandle& nh) {
    this->nh_ = nh;
    this->initParam();
}

// BT.cpp:24-172: same keys, same fall-back values
void bsplineTraj::initParam() {
    auto get = [this](const char* key, double& dst, double fallback) {
        if (!this->nh_.getParam(key, dst)) dst = fallback;
    };
    get("bspline_traj/timestep", ts_, 0.1);
    get("bspline_traj/distance_threshold", dthresh_, 0.5);
    get("bspline_traj/max_vel", maxVel_, 1.0);
    get("bspline_traj/max_acc", maxAcc_, 0.5);
    get("bspline_traj/weight_distance", weightDistance_, 0.5);
    get("bspline_traj/weight_smoothness", weightSmoothness_, 1.0);
    get("bspline_traj/weight_feasibility", weightFeasibility_, 1.0);
    get("bspline_traj/weight_dynamic_obstacle", weightDynamicObstacle_, 1.0);
    if (!nh_.getParam("bspline_traj/plan_in_z_axis", planInZAxis_)) planInZAxis_ = true;
    get("bspline_traj/min_height", minHeight_, 0.5);
    get("bspline_traj/max_height", maxHeight_, 2.0);
    get("bspline_traj/uncertain_aware_factor", uncertainAwareFactor_, 2.0);
    get("bspline_traj/prediction_horizon", predHorizon_, 2.0);
    get("bspline_traj/distance_threshold_dynamic", distThreshDynamic_, 1.0);
    get("bspline_traj/max_path_length", maxPathLength_, 7.0);
    std::vector<double> mos;
    if (!nh_.getParam("bspline_traj/max_obstacle_size", mos) || mos.size() < 3) maxObstacleSize_ = Eigen::Vector3d(10.0, 10.0, 10.0);
    else maxObstacleSize_ = Eigen::Vector3d(mos[0], mos[1], mos[2]);
}

// What the device searches of a group of planners share, from the group's lead: the map's resolution, the A* node pool
// setMap sizes from maxObstacleSize_ (BT.cpp:187-195), the control-point count.
struct bsplineTraj::SearchGroup {
    double res;
    int32_t pool[3];
    double half[3];        // reach of a search's node pool around the midpoint of its ends: pool / 2 + 1 nodes
    int N;
    double notCheckRatio;
    explicit SearchGroup(const bsplineTraj& lead)
        : res(lead.link_.map()->getRes()), N(lead.optData_.controlPoints.cols()), notCheckRatio(lead.notCheckRatio_) {
        for (int k = 0; k < 3; ++k) {
            pool[k] = 2 * int(lead.maxObstacleSize_(k) / res);
            half[k] = (pool[k] / 2 + 1) * res;
        }
    }
    // the ranges the device entries take: the pool's always, with `scan` vigo_path_search's for the segment scan too
    bool valid(bool scan) const {
        for (int k = 0; k < 3; ++k)
            if (pool[k] < 3 || pool[k] > VIGO_ASTAR_MAX_POOL_AXIS) return false;
        return !scan || (N >= 7 && notCheckRatio >= 0.0 && notCheckRatio <= 1.0);
    }
    // x and y may share such a group: a device batch and a node pool
    static bool same(const bsplineTraj& x, const bsplineTraj& y) {
        return x.sameBatchKey(y) && x.maxObstacleSize_(0) == y.maxObstacleSize_(0) && x.maxObstacleSize_(1) == y.maxObstacleSize_(1) &&
               x.maxObstacleSize_(2) == y.maxObstacleSize_(2);
    }
};

// BT.cpp:187-195
void bsplineTraj::setMap(const std::shared_ptr<mapManager::occMap>& map) {
    link_.setMap(map);
    this->pathSearch_.reset(new AStar);
    const SearchGroup g(*this);
    this->pathSearch_->initGridMap(map, Eigen::Vector3i(g.pool[0], g.pool[1], g.pool[2]), this->minHeight_, this->maxHeight_);
}

void bsplineTraj::setMapRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) { link_.setRegion(boxMin, boxMax); }
void bsplineTraj::refreshMap() { link_.refresh(); }
void bsplineTraj::setDevice(int ordinal) { link_.setDevice(ordinal); }

void bsplineTraj::updateMaxVel(double maxVel) { this->maxVel_ = maxVel; }
void bsplineTraj::updateMaxAcc(double maxAcc) { this->maxAcc_ = maxAcc; }

// every hot-path parameter the device sees for this planner
void bsplineTraj::fillParams(vigo_params_s* Pp) const {
    vigo_params_t& P = *Pp;
    vigo_default_params(&P);
    P.dthresh = dthresh_;
    P.dist_thresh_dynamic = distThreshDynamic_;
    P.ts_ctrl = controlPointsTs_;
    P.ts = ts_;
    P.pred_horizon = predHorizon_;
    P.uncertain_factor = uncertainAwareFactor_;
    P.w_distance = weightDistance_;
    P.w_smoothness = weightSmoothness_;
    P.w_feasibility = weightFeasibility_;
    P.w_dynamic = weightDynamicObstacle_;
    P.min_height = minHeight_;
    P.max_height = maxHeight_;
    P.plan_in_z = planInZAxis_ ? 1 : 0;
    P.mem_size = 16;          // BT.cpp:697
    P.max_iterations = 200;   // BT.cpp:698
    P.g_epsilon = 0.01;       // BT.cpp:699
}

// Two planners may share a device batch when the lead's handle state fits both: the same map object AND the same
// box of it to snapshot (setMapRegion), the same control-point count, gate step (maxVel_) and every parameter of fillParams() except the four weights, which
// travel per trajectory.
bool bsplineTraj::sameBatchKey(const bsplineTraj& o) const {
    if (!link_.sameTarget(o.link_) || maxVel_ != o.maxVel_ || notCheckRatio_ != o.notCheckRatio_ ||
        optData_.controlPoints.cols() != o.optData_.controlPoints.cols())
        return false;
    vigo_params_t a, b;
    this->fillParams(&a);
    o.fillParams(&b);
    a.w_distance = b.w_distance; a.w_smoothness = b.w_smoothness; a.w_feasibility = b.w_feasibility; a.w_dynamic = b.w_dynamic;
    return std::memcmp(&a, &b, sizeof(a)) == 0;
}

// handle creation, parameter push and (re)snapshot of the map when it changed (DeviceLink::sync); a planner without a map
// still gets its handle and parameters
bool bsplineTraj::syncDevice() {
    vigo_params_t P;
    this->fillParams(&P);
    const DeviceLink::Sync r = link_.sync(false, &P);
    if (r == DeviceLink::kNoDevice)
        cout << "[BsplineTraj]: HIP device " << link_.ordinal() << " is not available (there is no CPU fallback)." << endl;
    if (r == DeviceLink::kNoHandle) cout << "[BsplineTraj]: no HIP device for the ViGO back-end (there is no CPU fallback)." << endl;
    return r == DeviceLink::kSynced;
}

// BT.cpp:207-245
bool bsplineTraj::inputPathCheck(const nav_msgs::Path& path, nav_msgs::Path& adjustedPath, double dt, double& finalTime) {
    bool wrote = false;
    double prevOut = 0.0;
    const bool ok = this->inputPathCheckWith(path, adjustedPath, dt, finalTime, g_prevPathLength.load(), prevOut, wrote);
    if (wrote) g_prevPathLength.store(prevOut);
    return ok;
}

// the same with the previous path length passed in and out (wrote: the call reached adjustPathLengthDirect)
bool bsplineTraj::inputPathCheckWith(const nav_msgs::Path& path, nav_msgs::Path& adjustedPath, double dt, double& finalTime, double prevIn,
                                     double& prevOut, bool& wrote) {
    wrote = false;
    prevOut = prevIn;
    if (path.poses.size() == 0) return true;
    std::vector<Eigen::Vector3d> curveFitPoints, adjustedCurveFitPoints;
    this->pathMsgToEigenPoints(path, curveFitPoints);
    this->adjustPathLengthWith(curveFitPoints, adjustedCurveFitPoints, prevIn, prevOut);
    wrote = true;
    for (size_t i = 0; i + 1 < adjustedCurveFitPoints.size(); ++i) {
        double dist = (adjustedCurveFitPoints[i] - adjustedCurveFitPoints[i + 1]).norm();
        if (dist > this->controlPointDistance_ * 1.5) return false;
    }
    Eigen::Vector3d prevPoint;
    std::vector<Eigen::Vector3d> adjustedPoints;
    for (size_t i = 0; i < adjustedCurveFitPoints.size(); ++i) {
        Eigen::Vector3d p = adjustedCurveFitPoints[i];
        if (i == 0) {
            adjustedPoints.push_back(p);
            prevPoint = p;
        } else if ((p - prevPoint).norm() >= this->controlPointDistance_ * 0.8) {
            adjustedPoints.push_back(p);
            prevPoint = p;
        }
    }
    adjustedPoints.push_back(adjustedPoints.back());
    this->eigenPointsToPathMsg(adjustedPoints, adjustedPath);
    finalTime = (adjustedCurveFitPoints.size() - 1) * dt;
    return true;
}

// BT.cpp:247-288
bool bsplineTraj::fillPath(const nav_msgs::Path& path, nav_msgs::Path& adjustedPath) {
    const int n = int(path.poses.size());
    if (n <= 1) return false;
    auto P = [&](int i) { return Eigen::Vector3d(path.poses[i].pose.position.x, path.poses[i].pose.position.y, path.poses[i].pose.position.z); };
    std::vector<Eigen::Vector3d> out;
    if (n == 2) {
        Eigen::Vector3d ps = P(0), pf = P(1);
        out = {ps, (pf - ps) / 3.0 + ps, 2.0 * (pf - ps) / 3.0 + ps, pf};
    } else if (n == 3) {
        Eigen::Vector3d ps = P(0), pm = P(1), pf = P(2);
        out = {ps, (ps + pm) / 2.0, pm, (pm + pf) / 2.0, pf};
    } else {
        adjustedPath = path;
        return true;
    }
    adjustedPath.poses.clear();
    for (const auto& q : out) {
        geometry_msgs::PoseStamped ps;
        ps.pose.position.x = q(0); ps.pose.position.y = q(1); ps.pose.position.z = q(2);
        adjustedPath.poses.push_back(ps);
    }
    return true;
}

// BT.cpp:290-312: everything of updatePath() before the fit — goal check, path-length adjustment,
// filling short paths, clear() — leaving the curve-fit points
bool bsplineTraj::prepareFitPoints(const nav_msgs::Path& adjustedPath, std::vector<Eigen::Vector3d>& adjustedCurveFitPoints) {
    bool wrote = false;
    const double prevIn = g_prevPathLength.load();
    double prevOut = prevIn;
    const bool ok = this->prepareFitPointsWith(adjustedPath, adjustedCurveFitPoints, prevIn, prevOut, wrote);
    if (wrote) g_prevPathLength.store(prevOut);
    return ok;
}

bool bsplineTraj::prepareFitPointsWith(const nav_msgs::Path& adjustedPath, std::vector<Eigen::Vector3d>& adjustedCurveFitPoints, double prevIn,
                                       double& prevOut, bool& wrote) {
    wrote = false;
    prevOut = prevIn;
    adjustedCurveFitPoints.clear();
    if (adjustedPath.poses.empty() || !link_.map()) return false;
    Eigen::Vector3d goal(adjustedPath.poses.back().pose.position.x, adjustedPath.poses.back().pose.position.y,
                         adjustedPath.poses.back().pose.position.z);
    if (this->link_.map()->isInflatedOccupied(goal)) {
        cout << "[bsplineTraj]: Invalid goal position: " << goal(0) << " " << goal(1) << " " << goal(2) << endl;
        return false;
    }
    std::vector<Eigen::Vector3d> adjustedPathVec, inputPathVec;
    this->pathMsgToEigenPoints(adjustedPath, adjustedPathVec);
    this->adjustPathLengthWith(adjustedPathVec, inputPathVec, prevIn, prevOut);
    wrote = true;
    nav_msgs::Path inputPath;
    this->eigenPointsToPathMsg(inputPathVec, inputPath);
    if (inputPath.poses.size() < 4) {
        if (!this->fillPath(adjustedPath, inputPath)) {
            cout << "[bsplineTraj]: Input path point size is less (or equal) than 1." << endl;
            return false;
        }
    }
    this->clear();
    this->pathMsgToEigenPoints(inputPath, adjustedCurveFitPoints);
    return true;
}

// BT.cpp:315-322
void bsplineTraj::installControlPoints(const Eigen::MatrixXd& controlPoints, const std::vector<Eigen::Vector3d>& adjustedCurveFitPoints) {
    this->optData_.controlPoints = controlPoints;
    int controlPointNum = controlPoints.cols();
    this->optData_.guidePoints.assign(controlPointNum, {});
    this->optData_.guideDirections.assign(controlPointNum, {});
    this->optData_.findGuidePoint.assign(controlPointNum, false);
    this->init_ = true;
    this->inputPathVis_ = adjustedCurveFitPoints;
}

// BT.cpp:290-323
bool bsplineTraj::updatePath(const nav_msgs::Path& adjustedPath, const std::vector<Eigen::Vector3d>& startEndConditions) {
    std::vector<Eigen::Vector3d> adjustedCurveFitPoints;
    if (!this->prepareFitPoints(adjustedPath, adjustedCurveFitPoints)) return false;
    Eigen::MatrixXd controlPoints;
    if (!trajPlanner::bspline::parameterizeToBspline(this->controlPointsTs_, adjustedCurveFitPoints, startEndConditions, controlPoints))
        return false;  // the reference exit(0)s here (bspline.cpp:80-91)
    this->installControlPoints(controlPoints, adjustedCurveFitPoints);
    return true;
}

// updatePath() for many planners: the host prologue per planner, then ONE vigo_bspline_fit launch
// per group of equal waypoint count (bspline::parameterizeToBspline, bspline.cpp:74-138, batched).
std::vector<bool> bsplineTraj::updatePathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<nav_msgs::Path>& paths,
                                               const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions) {
    std::vector<bool> ok(planners.size(), false);
    if (paths.size() != planners.size() || startEndConditions.size() != planners.size()) return ok;
    std::vector<std::vector<Eigen::Vector3d>> fitPts(planners.size());
    std::vector<bool> ready(planners.size(), false);
    // The prologues (goal check, path-length adjustment with its line checks against the map, filling) run on the host
    // workers, each as if its predecessor had left a previous path length not above its own max_path_length — then the
    // value does not enter (BT.cpp:762: max(prevPathLength, maxPathLength_)); a serial pass hands the real value down the
    // line and repeats, in order, the rare planner for which it does enter.  Same results as one planner after another.
    std::vector<uint8_t> okv(planners.size(), 0), wrote(planners.size(), 0);
    std::vector<double> prevOut(planners.size(), 0.0);
    parallelFor(planners.size(), [&](size_t i) {
        if (startEndConditions[i].size() != 4) return;
        bool w = false;
        okv[i] = planners[i]->prepareFitPointsWith(paths[i], fitPts[i], 0.0, prevOut[i], w) ? 1 : 0;
        wrote[i] = w ? 1 : 0;
    });
    double prev = g_prevPathLength.load();
    for (size_t i = 0; i < planners.size(); ++i) {
        if (startEndConditions[i].size() == 4 && wrote[i] && prev > planners[i]->maxPathLength_) {
            bool w = false;
            okv[i] = planners[i]->prepareFitPointsWith(paths[i], fitPts[i], prev, prevOut[i], w) ? 1 : 0;
        }
        if (wrote[i]) prev = prevOut[i];
        ready[i] = okv[i] && fitPts[i].size() > 3;
    }
    g_prevPathLength.store(prev);
    fitGroups(planners, fitPts, ready, startEndConditions, ok);
    return ok;
}

// The fit stage of updatePathBatch and seedPathBatch: ONE vigo_bspline_fit launch per group of ready planners with equal
// point count and knot span, the control points installed (BT.cpp:315-322).
void bsplineTraj::fitGroups(const std::vector<bsplineTraj*>& planners, const std::vector<std::vector<Eigen::Vector3d>>& fitPts,
                            const std::vector<bool>& ready, const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions,
                            std::vector<bool>& ok) {
    auto sameFit = [&](size_t a, size_t b) {
        return ready[a] && ready[b] && fitPts[a].size() == fitPts[b].size() && planners[a]->controlPointsTs_ == planners[b]->controlPointsTs_ &&
               planners[a]->link_.sameTarget(planners[b]->link_);   // the fit runs on the lead's handle: a lead without a device fails its own group only
    };
    vigo_host::forEachGroup(planners.size(), sameFit, [&](const std::vector<size_t>& grp) {
        bsplineTraj* lead = planners[grp[0]];
        const int K = (int)fitPts[grp[0]].size();
        const double ts = lead->controlPointsTs_;
        if (K + 2 > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return;
        const int B = (int)grp.size();
        std::vector<double> pts((size_t)B * K * 3), cond((size_t)B * 12), ctrl((size_t)B * (K + 2) * 3);
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < K; ++i)
                for (int q = 0; q < 3; ++q) pts[((size_t)b * K + i) * 3 + q] = fitPts[grp[b]][i](q);
            for (int i = 0; i < 4; ++i)
                for (int q = 0; q < 3; ++q) cond[((size_t)b * 4 + i) * 3 + q] = startEndConditions[grp[b]][i](q);
        }
        static thread_local StagingBuf dPts, dCond, dCtrl;
        if (!dPts.upload(pts.data(), pts.size() * 8) || !dCond.upload(cond.data(), cond.size() * 8) || !dCtrl.alloc(ctrl.size() * 8)) return;
        if (vigo_bspline_fit(lead->link_.handle(), B, K, ts, (const double*)dPts.p, (const double*)dCond.p, (double*)dCtrl.p) != VIGO_OK) {
            cout << "[BsplineTraj]: vigo_bspline_fit failed: " << vigo_last_error(lead->link_.handle()) << endl;
            return;
        }
        if (!vigo_host::threadSync() || !dCtrl.download(ctrl.data(), ctrl.size() * 8)) return;
        parallelFor((size_t)B, [&](size_t b) {
            Eigen::MatrixXd controlPoints;
            controlPoints.resize(3, K + 2);
            std::memcpy(controlPoints.data(), ctrl.data() + b * (K + 2) * 3, sizeof(double) * 3 * (K + 2));
            planners[grp[b]]->installControlPoints(controlPoints, fitPts[grp[b]]);
        });
        for (int b = 0; b < B; ++b) ok[grp[b]] = true;
    });
}

// ---- the seed-path stage for many planners (bspline_node.cpp:317-378): seedPathBatch -------------------------------
namespace {
std::atomic<bool> g_deviceSeed{false};
std::atomic<int> g_seedMaxTries{16};
std::atomic<long long> g_seedDevice{0}, g_seedHost{0};
constexpr int kSeedPointCap = 128;   // rows of the launch's seed / fit outputs per planner; a longer list is the host's
}  // namespace

void bsplineTraj::setDeviceSeed(bool on) { g_deviceSeed.store(on); }
bool bsplineTraj::deviceSeed() { return g_deviceSeed.load(); }
void bsplineTraj::setSeedMaxTries(int n) { g_seedMaxTries.store(n < 1 ? 1 : n); }
int bsplineTraj::seedMaxTries() { return g_seedMaxTries.load(); }
void bsplineTraj::deviceSeedTotals(long long* deviceDecided, long long* hostRun) {
    if (deviceDecided) *deviceDecided = g_seedDevice.load();
    if (hostRun) *hostRun = g_seedHost.load();
}

// bspline_node.cpp:338-352 for one planner, the loop ending on the try count
void bsplineTraj::seedSearchWith(polyTrajOccMap& poly, double dt0, int maxTries, double prevIn, SeedInfo& s, nav_msgs::Path& seed) {
    s = SeedInfo();
    s.dt = dt0;
    seed.poses.clear();
    double prev = prevIn;
    for (int k = 0; k < maxTries; ++k) {
        ++s.tries;
        const nav_msgs::Path input = poly.getTrajectory(s.dt);
        bool wrote = false;
        double prevOut = prev;
        const bool ok = this->inputPathCheckWith(input, seed, s.dt, s.finalTime, prev, prevOut, wrote);
        if (wrote) {
            prev = prevOut;
            s.wrote = true;
        }
        if (ok) {
            s.found = true;
            break;
        }
        s.dt *= 0.8;
    }
    s.prevOut = prev;
}

void bsplineTraj::seedSteps(polyTrajOccMap& poly, double dt0, int maxTries, double prevSeedIn, double prevFitIn, SeedSteps& out) {
    out = SeedSteps();
    this->seedSearchWith(poly, dt0, maxTries, prevSeedIn, out.search, out.seed);
    out.fitOk = this->prepareFitPointsWith(out.seed, out.fitPoints, prevFitIn, out.prevFitOut, out.fitWrote);
}

// what seedPathBatch keeps per planner between its passes
struct bsplineTraj::SeedBatch {
    int maxTries;
    std::vector<nav_msgs::Path> seed;
    std::vector<SeedInfo> info;
    std::vector<std::vector<Eigen::Vector3d>> fitPts;
    std::vector<uint8_t> eligible, onDevice, okv, wroteFit;
    std::vector<double> prevFitOut;
    explicit SeedBatch(size_t n, int tries)
        : maxTries(tries), seed(n), info(n), fitPts(n), eligible(n, 0), onDevice(n, 0), okv(n, 0), wroteFit(n, 0), prevFitOut(n, 0.0) {}
};

// ONE vigo_seed_paths launch per group of eligible planners that share a device batch and a polynomial degree, as if
// every predecessor had left a previous path length of 0; one upload, one download.  A trajectory the launch defers or
// refuses stays with the host steps.
void bsplineTraj::seedOnDevice(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys, SeedBatch& sb) {
    auto same = [&](size_t a, size_t b) {
        return sb.eligible[a] && sb.eligible[b] && planners[a]->sameBatchKey(*planners[b]) &&
               polys[a]->getSolver()->getPolyDegree() == polys[b]->getSolver()->getPolyDegree();
    };
    vigo_host::forEachGroup(planners.size(), same, [&](const std::vector<size_t>& grp) {
        bsplineTraj* lead = planners[grp[0]];
        const int deg = polys[grp[0]]->getSolver()->getPolyDegree();
        if (deg < 0 || deg > 15 || !lead->syncDevice()) return;
        const int T = (int)grp.size(), cap = kSeedPointCap;
        std::vector<int32_t> segOff(1, 0);
        for (size_t i : grp) segOff.push_back(segOff.back() + (int32_t)polys[i]->getSolver()->timeKnots().size() - 1);
        const int S = segOff.back();
        // the inputs as one block: per-trajectory scalars [6][T], knots [S + T], coefficients [S][3][deg + 1], offsets
        const size_t nD = 6 * (size_t)T + (size_t)S + T + (size_t)S * 3 * (deg + 1);
        std::vector<double> in(nD + (segOff.size() + 1) / 2);
        double *duration = in.data(), *dt0 = duration + T, *cpd = dt0 + T, *maxLen = cpd + T, *prevSeed = maxLen + T, *prevFit = prevSeed + T;
        double *knots = prevFit + T, *coeffs = knots + S + T;
        std::memcpy(in.data() + nD, segOff.data(), segOff.size() * sizeof(int32_t));
        for (int b = 0; b < T; ++b) {
            bsplineTraj* p = planners[grp[b]];
            const polyTrajSolver* sol = polys[grp[b]]->getSolver();
            duration[b] = polys[grp[b]]->getDuration();
            dt0[b] = p->getInitTs();
            cpd[b] = p->controlPointDistance_;
            maxLen[b] = p->maxPathLength_;
            prevSeed[b] = 0.0;
            prevFit[b] = 0.0;
            const std::vector<double>& k = sol->timeKnots();
            std::copy(k.begin(), k.end(), knots + segOff[b] + b);
            for (int sgm = 0; sgm < segOff[b + 1] - segOff[b]; ++sgm)
                for (int ax = 0; ax < 3; ++ax)
                    std::copy(sol->getSolution(ax).begin() + (size_t)sgm * (deg + 1), sol->getSolution(ax).begin() + (size_t)(sgm + 1) * (deg + 1),
                              coeffs + ((size_t)(segOff[b] + sgm) * 3 + ax) * (deg + 1));
        }
        // the outputs as one block: [4][T] ints, [4][T] doubles, seed and fit points [T][cap][3] each
        const size_t outBytes = 16 * (size_t)T + 32 * (size_t)T + 2 * (size_t)T * cap * 24;
        std::vector<double> out(outBytes / 8);
        static thread_local StagingBuf dIn, dOut;
        if (!dIn.upload(in.data(), in.size() * 8) || !dOut.alloc(outBytes)) return;
        const double* di = (const double*)dIn.p;
        int32_t* oi = (int32_t*)dOut.p;
        double* od = (double*)dOut.p + 2 * (size_t)T;
        if (vigo_seed_paths(lead->link_.handle(), T, S, deg, (const int32_t*)(di + nD), di + 6 * (size_t)T + S + T, di + 6 * (size_t)T, di, di + T,
                            di + 2 * (size_t)T, di + 3 * (size_t)T, di + 4 * (size_t)T, di + 5 * (size_t)T, sb.maxTries, cap, oi, oi + T, od, od + T,
                            oi + 2 * (size_t)T, od + 4 * (size_t)T, oi + 3 * (size_t)T, od + 4 * (size_t)T + (size_t)T * cap * 3, od + 2 * (size_t)T,
                            od + 3 * (size_t)T) != VIGO_OK) {
            cout << "[BsplineTraj]: vigo_seed_paths failed: " << vigo_last_error(lead->link_.handle()) << endl;
            return;
        }
        if (!vigo_host::threadSync() || !dOut.download(out.data(), outBytes)) return;
        const int32_t *status = (const int32_t*)out.data(), *tries = status + T, *seedN = tries + T, *fitN = seedN + T;
        const double *dt = out.data() + 2 * (size_t)T, *finalTime = dt + T, *prevSeedOut = finalTime + T, *prevFitOut = prevSeedOut + T;
        const double *seedPts = prevFitOut + T, *fitPts = seedPts + (size_t)T * cap * 3;
        parallelFor((size_t)T, [&](size_t b) {
            const size_t i = grp[b];
            if (status[b] == VIGO_SEED_DEFERRED || status[b] == VIGO_SEED_BAD_INPUT) return;
            SeedInfo& s = sb.info[i];
            s = SeedInfo();
            s.found = status[b] != VIGO_SEED_NO_SPACING;
            s.tries = tries[b];
            s.dt = dt[b];
            s.finalTime = finalTime[b];
            s.wrote = !(status[b] == VIGO_SEED_TOO_SHORT && seedN[b] == 0);
            s.prevOut = prevSeedOut[b];
            std::vector<Eigen::Vector3d> pts;
            for (int q = 0; q < seedN[b]; ++q) {
                const double* v = seedPts + ((size_t)b * cap + q) * 3;
                pts.push_back(Eigen::Vector3d(v[0], v[1], v[2]));
            }
            sb.seed[i].poses.clear();
            if (!pts.empty()) planners[i]->eigenPointsToPathMsg(pts, sb.seed[i]);
            sb.fitPts[i].clear();
            for (int q = 0; q < fitN[b]; ++q) {
                const double* v = fitPts + ((size_t)b * cap + q) * 3;
                sb.fitPts[i].push_back(Eigen::Vector3d(v[0], v[1], v[2]));
            }
            sb.okv[i] = status[b] == VIGO_SEED_OK ? 1 : 0;
            sb.wroteFit[i] = sb.okv[i];
            sb.prevFitOut[i] = prevFitOut[b];
            sb.onDevice[i] = 1;
        });
    });
}

std::vector<bool> bsplineTraj::seedPathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys,
                                             const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions,
                                             std::vector<nav_msgs::Path>* seeds, std::vector<SeedInfo>* info) {
    const size_t n = planners.size();
    std::vector<bool> ok(n, false);
    if (polys.size() != n || startEndConditions.size() != n) return ok;
    SeedBatch sb(n, g_seedMaxTries.load());
    if (g_deviceSeed.load()) {
        for (size_t i = 0; i < n; ++i) {
            const polyTrajSolver* sol = polys[i]->getSolver();
            sb.eligible[i] = startEndConditions[i].size() == 4 && planners[i]->link_.map() && sol && sol->hasSolution() &&
                             !polys[i]->usesPwlFallback();
        }
        seedOnDevice(planners, polys, sb);
    }
    // The searches run as if every predecessor had left a previous path length not above the planner's own
    // max_path_length — then the value does not enter (BT.cpp:762) — and a serial pass in the reference's order (every
    // planner's search, then every planner's updatePath) hands the real value down and repeats, on the host and in
    // order, the rare planner for which it does enter: updatePathBatch's scheme, over both phases.
    parallelFor(n, [&](size_t i) {
        if (!sb.onDevice[i]) planners[i]->seedSearchWith(*polys[i], planners[i]->getInitTs(), sb.maxTries, 0.0, sb.info[i], sb.seed[i]);
    });
    double prev = g_prevPathLength.load();
    std::vector<uint8_t> redone(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (sb.info[i].wrote && prev > planners[i]->maxPathLength_) {
            planners[i]->seedSearchWith(*polys[i], planners[i]->getInitTs(), sb.maxTries, prev, sb.info[i], sb.seed[i]);
            redone[i] = 1;
        }
        if (sb.info[i].wrote) prev = sb.info[i].prevOut;
    }
    parallelFor(n, [&](size_t i) {
        if ((sb.onDevice[i] && !redone[i]) || startEndConditions[i].size() != 4) return;
        bool w = false;
        sb.okv[i] = planners[i]->prepareFitPointsWith(sb.seed[i], sb.fitPts[i], 0.0, sb.prevFitOut[i], w) ? 1 : 0;
        sb.wroteFit[i] = w ? 1 : 0;
    });
    std::vector<bool> ready(n, false);
    for (size_t i = 0; i < n; ++i) {
        if (startEndConditions[i].size() == 4 && sb.wroteFit[i] && prev > planners[i]->maxPathLength_) {
            bool w = false;
            sb.okv[i] = planners[i]->prepareFitPointsWith(sb.seed[i], sb.fitPts[i], prev, sb.prevFitOut[i], w) ? 1 : 0;
            redone[i] = 1;
        }
        if (sb.wroteFit[i]) prev = sb.prevFitOut[i];
        ready[i] = startEndConditions[i].size() == 4 && sb.okv[i] && sb.fitPts[i].size() > 3;
        if (sb.onDevice[i] && !redone[i]) {
            if (sb.okv[i]) planners[i]->clear();             // prepareFitPointsWith's clear() (BT.cpp:308), for the launch's own
            g_seedDevice.fetch_add(1);
        } else {
            g_seedHost.fetch_add(1);
        }
    }
    g_prevPathLength.store(prev);
    fitGroups(planners, sb.fitPts, ready, startEndConditions, ok);
    if (seeds) *seeds = sb.seed;
    if (info) *info = sb.info;
    return ok;
}

void bsplineTraj::updateDynamicObstacles(const std::vector<Eigen::Vector3d>& obstaclesPos, const std::vector<Eigen::Vector3d>& obstaclesVel,
                                         const std::vector<Eigen::Vector3d>& obstaclesSize) {
    this->optData_.dynamicObstaclesPos = obstaclesPos;
    this->optData_.dynamicObstaclesVel = obstaclesVel;
    this->optData_.dynamicObstaclesSize = obstaclesSize;
}

// BT.cpp:333-385
bool bsplineTraj::makePlan() {
    std::vector<bsplineTraj*> one{this};
    return makePlanBatch(one)[0];
}

bool bsplineTraj::makePlan(nav_msgs::Path& trajectory, bool yaw) {
    bool success = this->makePlan();
    trajectory = this->evalTrajToMsg(yaw);
    return success;
}

void bsplineTraj::clear() {
    this->optData_.guidePoints.clear();
    this->optData_.guideDirections.clear();
    this->optData_.dynamicObstaclesPos.clear();
    this->optData_.dynamicObstaclesVel.clear();
    this->optData_.dynamicObstaclesSize.clear();
    this->collisionSeg_.clear();
    this->astarPaths_.clear();
}

// BT.cpp:403-445 (incl. the corner case that can duplicate a segment, :426-430)
void bsplineTraj::findCollisionSeg(const Eigen::MatrixXd& controlPoints, std::vector<std::pair<int, int>>& collisionSeg) {
    collisionSeg.clear();
    bool previousHasCollision = false;
    const int N = controlPoints.cols();
    int endIdx = int((N - bsplineDegree - 1) - this->notCheckRatio_ * (N - 2 * bsplineDegree));
    int pairStartIdx = bsplineDegree, pairEndIdx = bsplineDegree;
    for (int i = bsplineDegree; i <= endIdx; ++i) {
        Eigen::Vector3d p = controlPoints.col(i);
        bool hasCollision = this->link_.map()->isInflatedOccupied(p);
        if (hasCollision != previousHasCollision) {
            if (hasCollision) {
                pairStartIdx = i - 1;
            } else {
                pairEndIdx = i;
                collisionSeg.push_back({pairStartIdx, pairEndIdx});
            }
        }
        if (hasCollision && i == endIdx - 1) {
            pairEndIdx = N - 1;
            collisionSeg.push_back({pairStartIdx, pairEndIdx});
        }
        if (i != bsplineDegree && !previousHasCollision && !hasCollision) {
            if (this->link_.map()->isInflatedOccupiedLine(controlPoints.col(i - 1), p)) collisionSeg.push_back({i - 1, i});
        }
        previousHasCollision = hasCollision;
    }
}

namespace {
// BT.cpp:497-511: the segments after the merges of pathSearch
void applyMerges(std::vector<std::pair<int, int>>& collisionSeg, const std::vector<int>& mergeIndices) {
    if (mergeIndices.empty()) return;
    const int collisionSegNum = int(collisionSeg.size());
    int midx = 0;
    std::vector<std::pair<int, int>> collisionSegTemp;
    for (int i = 0; i < collisionSegNum; ++i) {
        if (midx < int(mergeIndices.size()) && i == mergeIndices[midx]) {
            collisionSegTemp.push_back({collisionSeg[i].first, collisionSeg[i + 1].second});
            ++i;
            ++midx;
        } else {
            collisionSeg.push_back(collisionSeg[i]);  // BT.cpp:507 pushes into the input...
        }
    }
    collisionSeg = collisionSegTemp;  // ...and :510 overwrites it: unmerged segments are dropped
}
}  // namespace

// BT.cpp:447-514 (merge bookkeeping reproduced as written, Appendix B of SURVEY.md)
bool bsplineTraj::pathSearch(std::vector<std::pair<int, int>>& collisionSeg, std::vector<std::vector<Eigen::Vector3d>>& paths) {
    paths.clear();
    std::vector<int> mergeIndices;
    int collisionSegNum = int(collisionSeg.size());
    for (int i = 0; i < collisionSegNum; ++i) {
        std::pair<int, int> seg = collisionSeg[i];
        Eigen::Vector3d pStart = this->optData_.controlPoints.col(seg.first);
        Eigen::Vector3d pEnd = this->optData_.controlPoints.col(seg.second);
        if (this->pathSearch_->AstarSearch(this->link_.map()->getRes(), pStart, pEnd)) {
            std::vector<Eigen::Vector3d> searchedPath = this->pathSearch_->getPath();
            searchedPath[0] = pStart;
            searchedPath.push_back(pEnd);
            paths.push_back(searchedPath);
        } else {
            if (i + 1 < collisionSegNum) {
                std::pair<int, int> nextSeg = collisionSeg[i + 1];
                if (nextSeg.first - seg.second <= 2) {
                    Eigen::Vector3d pEnd2 = this->optData_.controlPoints.col(nextSeg.second);
                    if (this->pathSearch_->AstarSearch(this->link_.map()->getRes(), pStart, pEnd2)) {
                        std::vector<Eigen::Vector3d> searchedPath = this->pathSearch_->getPath();
                        searchedPath[0] = pStart;
                        searchedPath.push_back(pEnd2);
                        paths.push_back(searchedPath);
                        mergeIndices.push_back(i);
                        ++i;
                        continue;
                    }
                }
            }
            cout << "[BsplineTraj]: Path Search Error. Force return." << endl;
            return false;
        }
    }
    applyMerges(collisionSeg, mergeIndices);
    return true;
}

// BT.h:196-204
bool bsplineTraj::checkCollisionLine(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2) {
    for (double a = 0.0; a <= 1.0; a += this->link_.map()->getRes()) {
        Eigen::Vector3d pMid = a * p1 + (1 - a) * p2;
        if (this->link_.map()->isInflatedOccupied(pMid)) return true;
    }
    return false;
}

// BT.h:206-240
void bsplineTraj::shortcutPath(const std::vector<Eigen::Vector3d>& path, std::vector<Eigen::Vector3d>& pathSC) {
    pathSC.clear();
    size_t ptr1 = 0, ptr2 = 2;
    pathSC.push_back(path[ptr1]);
    if (path.size() == 1) return;
    if (path.size() == 2) { pathSC.push_back(path[1]); return; }
    while (true) {
        if (ptr2 > path.size() - 1) break;
        if (!this->checkCollisionLine(path[ptr1], path[ptr2])) {
            if (ptr2 >= path.size() - 1) { pathSC.push_back(path[ptr2]); break; }
            ++ptr2;
        } else {
            pathSC.push_back(path[ptr2 - 1]);
            ptr1 = ptr2 - 1;
            ptr2 = ptr1 + 2;
        }
    }
}

// BT.h:251-304
bool bsplineTraj::findGuidePointSemiCircle(int controlPointIdx, const std::pair<int, int>& seg,
                                           const std::vector<Eigen::Vector3d>& path, Eigen::Vector3d& guidePoint) {
    double minAngle = 0.0, maxAngle = PI_const;
    int numControlpoints = seg.second - seg.first - 1;
    double targetAngle;
    Eigen::Vector3d pseudo;
    if (numControlpoints != 0) {
        int order = controlPointIdx - seg.first;
        targetAngle = order * PI_const / (numControlpoints + 2);
        targetAngle = std::min(std::max(minAngle, targetAngle), maxAngle);
        double ratio = double(order) / double(numControlpoints + 1.0);
        pseudo = ratio * (path.back() - path[0]) + path[0];
    } else {
        targetAngle = PI_const / 2.0;
        pseudo = (path[0] + path.back()) / 2.0;
    }
    Eigen::Vector3d direction = path[0] - pseudo;
    for (size_t i = 0; i + 1 < path.size(); ++i) {
        Eigen::Vector3d wpCurr = path[i], wpNext = path[i + 1];
        double angleCurr = angleBetweenVectors(direction, wpCurr - pseudo);
        double angleNext = angleBetweenVectors(direction, wpNext - pseudo);
        if (targetAngle >= angleCurr && targetAngle <= angleNext) {
            double prevAngleDiff = 0.0;
            Eigen::Vector3d prevTempPoint;
            for (double a = 1.0; a >= 0.0; a -= 0.1) {
                Eigen::Vector3d tempPoint = a * wpCurr + (1 - a) * wpNext;
                double angleDiff = angleBetweenVectors(direction, tempPoint - pseudo) - targetAngle;
                if (angleDiff == 0) { guidePoint = tempPoint; return true; }
                if (angleDiff * prevAngleDiff < 0) {
                    double totalDiff = std::abs(angleDiff) + std::abs(prevAngleDiff);
                    guidePoint = std::abs(prevAngleDiff) / totalDiff * (tempPoint - prevTempPoint) + prevTempPoint;
                    return true;
                }
                prevAngleDiff = angleDiff;
                prevTempPoint = tempPoint;
            }
        }
    }
    return false;
}

// BT.cpp:517-571
void bsplineTraj::assignGuidePointsSemiCircle(const std::vector<std::vector<Eigen::Vector3d>>& paths,
                                              const std::vector<std::pair<int, int>>& collisionSeg) {
    std::vector<std::vector<Eigen::Vector3d>> pathsSC;
    this->shortcutPaths(paths, pathsSC);
    const int N = this->optData_.controlPoints.cols();
    Eigen::Vector3d guidePoint, guideDirection;
    for (size_t i = 0; i < collisionSeg.size() && i < pathsSC.size(); ++i) {
        const std::pair<int, int> seg = collisionSeg[i];
        const std::vector<Eigen::Vector3d>& path = pathsSC[i];
        for (int idx = seg.first + 1; idx < seg.second; ++idx) {
            if (idx < 0 || idx >= N) continue;
            this->findGuidePointSemiCircle(idx, seg, path, guidePoint);
            this->optData_.guidePoints[idx].push_back(guidePoint);
            Eigen::Vector3d diff = guidePoint - this->optData_.controlPoints.col(idx);
            this->optData_.guideDirections[idx].push_back(diff / diff.norm());
        }
        if (seg.second - seg.first - 1 == 0) {  // line collision
            this->findGuidePointSemiCircle(seg.first, seg, path, guidePoint);
            Eigen::Vector3d midPoint = (this->optData_.controlPoints.col(seg.first) + this->optData_.controlPoints.col(seg.second)) / 2.0;
            Eigen::Vector3d diff = guidePoint - midPoint;
            guideDirection = diff / diff.norm();
            for (int idx = seg.first - 1; idx <= seg.second + 1; ++idx) {
                if (idx >= bsplineDegree && idx <= N - bsplineDegree - 1) {
                    this->optData_.guidePoints[idx].push_back(guidePoint);
                    this->optData_.guideDirections[idx].push_back(guideDirection);
                }
            }
        }
    }
}

bool bsplineTraj::indexInCollisionSeg(const std::vector<std::pair<int, int>>& collisionSeg, int idx) {
    for (const auto& seg : collisionSeg)
        if (idx >= seg.first && idx <= seg.second) return true;
    return false;
}

int bsplineTraj::findCollisionSegIndex(const std::vector<std::pair<int, int>>& collisionSeg, int idx) {
    int k = 0;
    for (const auto& seg : collisionSeg) {
        if (idx >= seg.first && idx <= seg.second) return k;
        ++k;
    }
    return -1;
}

// BT.h:417-429
bool bsplineTraj::isControlPointRequireNewGuide(int controlPointIdx) {
    Eigen::Vector3d c = this->optData_.controlPoints.col(controlPointIdx);
    for (size_t i = 0; i < this->optData_.guidePoints[controlPointIdx].size(); ++i) {
        double dist = (c - this->optData_.guidePoints[controlPointIdx][i]).dot(this->optData_.guideDirections[controlPointIdx][i]);
        if (this->dthresh_ - dist > 0) return false;
    }
    return true;
}

// BT.h:379-403: the control points of the new collision segments, split into those the previous segments already held
// and the fresh ones (a segment without interior points contributes both of its ends)
void bsplineTraj::compareCollisionSeg(const std::vector<std::pair<int, int>>& prevCollisionSeg, const std::vector<std::pair<int, int>>& newCollisionSeg,
                                      std::vector<int>& newCollisionPoints, std::vector<int>& overlappedCollisionPoints) {
    for (const auto& s : newCollisionSeg) {
        for (int i = s.first + 1; i <= s.second - 1; ++i) (indexInCollisionSeg(prevCollisionSeg, i) ? overlappedCollisionPoints : newCollisionPoints).push_back(i);
        if (s.second - s.first - 1 == 0)
            for (int i = s.first; i <= s.second; ++i) (indexInCollisionSeg(prevCollisionSeg, i) ? overlappedCollisionPoints : newCollisionPoints).push_back(i);
    }
}

// BT.h:250-257
void bsplineTraj::shortcutPaths(const std::vector<std::vector<Eigen::Vector3d>>& paths, std::vector<std::vector<Eigen::Vector3d>>& pathsSC) {
    pathsSC.clear();
    for (const auto& p : paths) {
        std::vector<Eigen::Vector3d> sc;
        this->shortcutPath(p, sc);
        pathsSC.push_back(sc);
    }
}

// BT.cpp:573-608
bool bsplineTraj::isReguideRequired(std::vector<std::pair<int, int>>& reguideCollisionSeg) {
    std::vector<std::pair<int, int>> prev = this->collisionSeg_;
    this->findCollisionSeg(this->optData_.controlPoints, this->collisionSeg_);
    std::vector<int> fresh, overlapped;
    this->compareCollisionSeg(prev, this->collisionSeg_, fresh, overlapped);
    std::set<int> segIdx;
    for (int i : fresh) segIdx.insert(findCollisionSegIndex(this->collisionSeg_, i));
    for (int i : overlapped)
        if (this->isControlPointRequireNewGuide(i)) segIdx.insert(findCollisionSegIndex(this->collisionSeg_, i));
    segIdx.erase(-1);
    if (segIdx.empty()) return false;
    for (int s : segIdx) reguideCollisionSeg.push_back(this->collisionSeg_[s]);
    return true;
}

// ---- device calls ---------------------------------------------------------------------

namespace {
using vigo_host::HostBatch;

// device pointers to a HostBatch's lists; an empty guide or obstacle list is null (vigo.h: "no guides" / "no obstacles")
struct DeviceBatch {
    double* ctrl;
    const int32_t* goff;
    const double* gpv;
    const uint8_t* gunk;
    const int32_t* ooff;
    const double* obs;
    double* weights;
};

// hb into the calling thread's staging buffers, then map_->isUnknown(guidePoint) (BT.cpp:841) for its guides, hoisted
// out of the solve.  The buffers live across calls (hipMalloc/hipFree per rebound round cost more than the round's
// kernels): the thread's next upload overwrites them, so what a call reads back is read back before that.
bool uploadBatch(vigo_handle_t h, const HostBatch& hb, DeviceBatch& d) {
    static thread_local StagingBuf dCtrl, dGoff, dGpv, dGunk, dOoff, dObs, dW;
    const size_t G = hb.guides();
    if (!dCtrl.upload(hb.ctrl.data(), hb.ctrl.size() * 8) || !dGoff.upload(hb.goff.data(), hb.goff.size() * 4) ||
        !dGpv.upload(hb.gpv.data(), hb.gpv.size() * 8) || !dGunk.alloc(G) || !dOoff.upload(hb.ooff.data(), hb.ooff.size() * 4) ||
        !dObs.upload(hb.obs.data(), hb.obs.size() * 8) || !dW.upload(hb.weights.data(), hb.weights.size() * 8))
        return false;
    if (G && vigo_guides_unknown(h, (int64_t)G, (const double*)dGpv.p, (uint8_t*)dGunk.p) != VIGO_OK) return false;
    d = {(double*)dCtrl.p, (const int32_t*)dGoff.p, G ? (const double*)dGpv.p : nullptr, G ? (const uint8_t*)dGunk.p : nullptr,
         (const int32_t*)dOoff.p, hb.obs.empty() ? nullptr : (const double*)dObs.p, (double*)dW.p};
    return true;
}

// vigo_cost_grad of the one trajectory in hb; grad receives its 3 (N - 6) free scalars
bool costGrad(vigo_handle_t h, const HostBatch& hb, double& cost, double* grad) {
    static thread_local StagingBuf dCost, dGrad;
    const size_t n = 3 * (size_t)(hb.N - 2 * bsplineDegree);
    DeviceBatch d;
    if (!uploadBatch(h, hb, d) || !dCost.alloc(8) || !dGrad.alloc(n * 8)) return false;
    if (vigo_cost_grad(h, 1, hb.N, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, (double*)dCost.p, (double*)dGrad.p, nullptr) != VIGO_OK)
        return false;
    return vigo_host::threadSync() && dCost.download(&cost, 8) && dGrad.download(grad, n * 8);
}
}  // namespace

void bsplineTraj::solveBatch(const std::vector<bsplineTraj*>& ps) {
    // groups of equal N share a launch (vigo_optimize takes one N per call)
    auto same = [&](size_t a, size_t b) { return ps[a]->sameBatchKey(*ps[b]); };
    vigo_host::forEachGroup(ps.size(), same, [&](const std::vector<size_t>& grp) {
        bsplineTraj* lead = ps[grp[0]];
        const int N = lead->optData_.controlPoints.cols();
        for (size_t k : grp) ps[k]->lastStatus_ = VIGO_ERR_HIP;
        if (N < 7 || N > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return;
        HostBatch hb(N);
        for (size_t k : grp) {
            const bsplineTraj* p = ps[k];
            hb.add(p->optData_.controlPoints.data(), p->optData_, {p->weightDistance_, p->weightSmoothness_, p->weightFeasibility_, p->weightDynamicObstacle_});
        }
        static thread_local StagingBuf dStatus;
        DeviceBatch d;
        if (!uploadBatch(lead->link_.handle(), hb, d) || !dStatus.alloc(hb.B * 4)) return;
        if (vigo_optimize(lead->link_.handle(), hb.B, N, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, nullptr, (int32_t*)dStatus.p, nullptr,
                          nullptr, nullptr) != VIGO_OK) {
            cout << "[BsplineTraj]: vigo_optimize failed: " << vigo_last_error(lead->link_.handle()) << endl;
            return;
        }
        std::vector<int32_t> status(hb.B);
        if (!vigo_host::threadSync() || !vigo_host::download(hb.ctrl.data(), d.ctrl, hb.ctrl.size() * 8) ||
            !dStatus.download(status.data(), status.size() * 4))
            return;
        for (int b = 0; b < hb.B; ++b) {
            // optData_.controlPoints = the last evaluated point, as costFunction leaves it (BT.cpp:803)
            std::memcpy(ps[grp[b]]->optData_.controlPoints.data(), hb.ctrl.data() + (size_t)b * 3 * N, sizeof(double) * 3 * N);
            ps[grp[b]]->lastStatus_ = status[b];
        }
    });
}

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
        static thread_local StagingBuf dCtrl, dFlag, dDyn, dOoff, dObs;
        if (!dCtrl.upload(ctrl.data(), ctrl.size() * 8) || !dFlag.alloc(B) || !dDyn.alloc(B) ||
            !dOoff.upload(ooff.data(), ooff.size() * 4) || !dObs.upload(obs.data(), obs.size() * 8))
            return;
        const double dt = lead->link_.map()->getRes() / lead->maxVel_ / 2.0;  // BT.h:312
        if (vigo_traj_collision(lead->link_.handle(), B, N, (const double*)dCtrl.p, dt, (uint8_t*)dFlag.p, nullptr) != VIGO_OK) return;
        std::vector<uint8_t> f(B), d(B, 0);
        if (!obs.empty()) {
            if (vigo_traj_dynamic_collision(lead->link_.handle(), B, N, (const double*)dCtrl.p, dt, (const int32_t*)dOoff.p,
                                            (const double*)dObs.p, 0, (uint8_t*)dDyn.p) != VIGO_OK)
                return;
        }
        if (!vigo_host::threadSync() || !dFlag.download(f.data(), B)) return;
        if (!obs.empty() && !dDyn.download(d.data(), B)) return;
        for (int b = 0; b < B; ++b) {
            col[idx[b]] = f[b];
            // BT.cpp:621-626: the dynamic gate only runs when the planner has obstacles
            dyn[idx[b]] = ps[idx[b]]->optData_.dynamicObstaclesPos.empty() ? 0 : d[b];
        }
    });
}

namespace {
std::atomic<bool> g_deviceResidentRebound{true};
}
void bsplineTraj::setDeviceResidentRebound(bool on) { g_deviceResidentRebound.store(on); }
bool bsplineTraj::deviceResidentRebound() { return g_deviceResidentRebound.load(); }

// BT.cpp:611-685 between two A* calls, on the device, for one group of planners (one batch): upload the planners'
// state, queue the rounds (vigo_rebound_rounds), bring back what the host part of the loop needs.
bool bsplineTraj::deviceRounds(const std::vector<bsplineTraj*>& grp, const std::vector<Rebound*>& rb, int maxRounds) {
    bsplineTraj* lead = grp[0];
    const int N = lead->optData_.controlPoints.cols();
    std::vector<int> prevStatus(grp.size());
    for (size_t k = 0; k < grp.size(); ++k) { prevStatus[k] = grp[k]->lastStatus_; grp[k]->lastStatus_ = VIGO_ERR_HIP; }
    if (N < 7 || N > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return false;
    HostBatch hb(N);
    std::vector<vigo_rebound_state_t> state(grp.size());
    for (size_t k = 0; k < grp.size(); ++k) {
        bsplineTraj* p = grp[k];
        hb.add(p->optData_.controlPoints.data(), p->optData_, {p->weightDistance_, p->weightSmoothness_, p->weightFeasibility_, p->weightDynamicObstacle_});
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
    static thread_local StagingBuf dState;
    DeviceBatch d;
    if (!uploadBatch(lead->link_.handle(), hb, d) || !dState.upload(state.data(), state.size() * sizeof(vigo_rebound_state_t))) return false;
    vigo_handle_t h = lead->link_.handle();
    const double dt = lead->link_.map()->getRes() / lead->maxVel_ / 2.0;  // BT.h:312
    if (vigo_rebound_rounds(h, hb.B, N, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, dt, lead->notCheckRatio_, maxRounds,
                            (vigo_rebound_state_t*)dState.p) != VIGO_OK) {
        cout << "[BsplineTraj]: vigo_rebound_rounds failed: " << vigo_last_error(h) << endl;
        return false;
    }
    // everything is read back here: the solveBatch of the overflow planners below reuses the staging buffers
    if (!vigo_host::threadSync() || !vigo_host::download(hb.ctrl.data(), d.ctrl, hb.ctrl.size() * 8) ||
        !vigo_host::download(hb.weights.data(), d.weights, hb.weights.size() * 8) ||
        !dState.download(state.data(), state.size() * sizeof(vigo_rebound_state_t)))
        return false;
    std::vector<size_t> overflow;
    for (size_t k = 0; k < grp.size(); ++k) {
        bsplineTraj* p = grp[k];
        const vigo_rebound_state_t& st = state[k];
        if (st.rounds == 0 && st.status == VIGO_RB_NEEDS_HOST) { overflow.push_back(k); continue; }
        // optData_.controlPoints = the last evaluated point, as costFunction leaves it (BT.cpp:803)
        std::memcpy(p->optData_.controlPoints.data(), hb.ctrl.data() + k * 3 * N, sizeof(double) * 3 * N);
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
        if (r.needOptimize) solveBatch(one);
        std::vector<uint8_t> col, dyn;
        gateBatch(one, col, dyn);
        r.gateStatic = col[0] != 0;
        r.gateDynamic = dyn[0] != 0;
        r.devStatus = (!r.gateStatic && !r.gateDynamic) ? VIGO_RB_DONE : VIGO_RB_NEEDS_HOST;
    }
    return true;
}

// BT.cpp:687-718
int bsplineTraj::optimize() {
    std::vector<bsplineTraj*> one{this};
    solveBatch(one);
    return lastStatus_;
}

// the lbfgs_evaluate_t seam on the device (BT.cpp:796-821)
double bsplineTraj::costFunction(const double* x, double* grad, const int n) {
    const int N = optData_.controlPoints.cols();
    if (n != 3 * (N - 2 * bsplineDegree) || !syncDevice()) return std::nan("");
    std::memcpy(optData_.controlPoints.data() + 3 * bsplineDegree, x, n * sizeof(double));  // BT.cpp:803
    HostBatch hb(N);
    hb.add(optData_.controlPoints.data(), optData_, {weightDistance_, weightSmoothness_, weightFeasibility_, weightDynamicObstacle_});
    double cost = 0;
    return costGrad(link_.handle(), hb, cost, grad) ? cost : std::nan("");
}

// BT.cpp:796-800: the lbfgs_evaluate_t-shaped entry (instance pointer first)
double bsplineTraj::solverCostFunction(void* func_data, const double* x, double* grad, const int n) {
    return reinterpret_cast<bsplineTraj*>(func_data)->costFunction(x, grad, n);
}

// One cost term and its gradient for the given control points, evaluated by the device kernel with a
// unit weight on that term (vigo_cost_grad's per-trajectory weights).  Columns of the three fixed control
// points at either end stay zero: the reference computes and then discards them (BT.cpp:819).
bool bsplineTraj::termCost(int term, const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient) {
    cost = 0;
    const int N = controlPoints.cols();
    gradient = Eigen::MatrixXd::Zero(3, N);
    if (N < 7 || N > VIGO_MAX_CTRL_POINTS || (int)optData_.guidePoints.size() < N || !syncDevice()) return false;
    std::array<double, 4> w{};
    w[term] = 1.0;
    HostBatch hb(N);
    hb.add(controlPoints.data(), optData_, w);
    std::vector<double> g(3 * (N - 2 * bsplineDegree));
    if (!costGrad(link_.handle(), hb, cost, g.data())) return false;
    std::memcpy(gradient.data() + 3 * bsplineDegree, g.data(), g.size() * 8);
    return true;
}
// BT.cpp:823-932, :934-950, :952-999, :1001-1064
void bsplineTraj::getDistanceCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient) { termCost(0, controlPoints, cost, gradient); }
void bsplineTraj::getSmoothnessCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient) { termCost(1, controlPoints, cost, gradient); }
void bsplineTraj::getFeasibilityCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient) { termCost(2, controlPoints, cost, gradient); }
void bsplineTraj::getDynamicObstacleCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient) { termCost(3, controlPoints, cost, gradient); }

// BT.cpp:1464-1496: velocity / acceleration samples of the current trajectory as text files, raw and
// with the linear feasibility re-parameterisation.  (The reference fills acc_adjusted_info.txt from the
// VELOCITY spline scaled by factor^2, BT.cpp:1488 — reproduced.)
void bsplineTraj::writeCurrentTrajInfo(const std::string& filePath, double dt) {
    if (!(dt > 0)) return;
    std::ofstream velInfo(filePath + "/vel_info.txt"), accInfo(filePath + "/acc_info.txt");
    std::ofstream velAdj(filePath + "/vel_adjusted_info.txt"), accAdj(filePath + "/acc_adjusted_info.txt");
    trajPlanner::bspline vel = this->bspline_.getDerivative();
    trajPlanner::bspline acc = vel.getDerivative();
    for (double t = 0.0; t <= this->bspline_.getDuration(); t += dt) {
        const Eigen::Vector3d v = vel.at(t), a = acc.at(t);
        velInfo << t << " " << v(0) << " " << v(1) << " " << v(2) << "\n";
        accInfo << t << " " << a(0) << " " << a(1) << " " << a(2) << "\n";
    }
    const double f = this->getLinearFactor();
    for (double t = 0.0; this->getLinearReparamTime(t) <= this->bspline_.getDuration(); t += dt) {
        const Eigen::Vector3d v = vel.at(this->getLinearReparamTime(t));
        velAdj << t << " " << v(0) * f << " " << v(1) * f << " " << v(2) * f << "\n";
        accAdj << t << " " << v(0) * f * f << " " << v(1) * f * f << " " << v(2) * f * f << "\n";
    }
}

// BT.h:307-325 / :344-368 through the device gates
bool bsplineTraj::hasCollisionTrajectory(const Eigen::MatrixXd& controlPoints) {
    Eigen::MatrixXd keep = optData_.controlPoints;
    optData_.controlPoints = controlPoints;
    std::vector<bsplineTraj*> one{this};
    std::vector<uint8_t> col, dyn;
    gateBatch(one, col, dyn);
    optData_.controlPoints = keep;
    return col[0] != 0;
}

bool bsplineTraj::hasDynamicCollisionTrajectory(const Eigen::MatrixXd& controlPoints) {
    Eigen::MatrixXd keep = optData_.controlPoints;
    optData_.controlPoints = controlPoints;
    std::vector<bsplineTraj*> one{this};
    std::vector<uint8_t> col, dyn;
    gateBatch(one, col, dyn);
    optData_.controlPoints = keep;
    return dyn[0] != 0;
}

void bsplineTraj::reboundBegin(Rebound& r) {
    r = Rebound();
    r.w0 = this->weightDistance_;
    r.wo0 = this->weightDynamicObstacle_;
}

// leaving the loop: the weights the loop doubled are restored (BT.cpp:629-630, :635-636, :651-652)
void bsplineTraj::reboundFinish(Rebound& r, bool ok) {
    this->weightDistance_ = r.w0;
    this->weightDynamicObstacle_ = r.wo0;
    r.done = true;
    r.ok = ok;
}

// the body of the while loop of BT.cpp:619-681, one pass
void bsplineTraj::reboundStep(Rebound& r, bool hasCollision, bool hasDynamicCollision, bool timedOut) {
    r.needOptimize = false;
    auto finish = [&](bool ok) { this->reboundFinish(r, ok); };
    if (!hasCollision && !hasDynamicCollision) { finish(true); return; }
    if (timedOut) { cout << "[BsplineTraj]: Optimization timeout." << endl; finish(false); return; }
    std::vector<std::vector<Eigen::Vector3d>> tempAstarPaths;
    if (r.failCount >= 4) {
        std::vector<std::pair<int, int>> collisionSeg;
        this->findCollisionSeg(this->optData_.controlPoints, collisionSeg);
        if (this->pathSearch(collisionSeg, tempAstarPaths)) {
            this->astarPaths_ = tempAstarPaths;
            this->assignGuidePointsSemiCircle(tempAstarPaths, collisionSeg);
        }
    }
    if (r.failCount >= 8) { finish(false); return; }
    if (hasCollision) {
        std::vector<std::pair<int, int>> reguideCollisionSeg;
        if (this->isReguideRequired(reguideCollisionSeg)) {
            if (this->pathSearch(reguideCollisionSeg, tempAstarPaths)) {
                this->astarPaths_ = tempAstarPaths;
                this->assignGuidePointsSemiCircle(tempAstarPaths, reguideCollisionSeg);
            } else {
                this->weightDistance_ *= 2.0;
                ++r.failCount;
            }
        } else {
            this->weightDistance_ *= 2.0;
            ++r.failCount;
        }
    }
    if (hasDynamicCollision) this->weightDynamicObstacle_ *= 2.0;
    r.needOptimize = true;
}

void bsplineTraj::setLoopState(const std::vector<std::pair<int, int>>& collisionSeg, const std::vector<std::vector<Eigen::Vector3d>>& guidePoints,
                               const std::vector<std::vector<Eigen::Vector3d>>& guideDirections, double weightDistance, double weightDynamicObstacle) {
    this->collisionSeg_ = collisionSeg;
    for (size_t i = 0; i < guidePoints.size() && i < this->optData_.guidePoints.size(); ++i) {
        this->optData_.guidePoints[i] = guidePoints[i];
        this->optData_.guideDirections[i] = guideDirections[i];
    }
    this->weightDistance_ = weightDistance;
    this->weightDynamicObstacle_ = weightDynamicObstacle;
}

void bsplineTraj::runLoopBody(bool hasCollision, bool hasDynamicCollision, int& failCount, bool& needOptimize, bool& done) {
    Rebound r;
    reboundBegin(r);
    r.failCount = failCount;
    reboundStep(r, hasCollision, hasDynamicCollision, false);
    failCount = r.failCount;
    needOptimize = r.needOptimize;
    done = r.done;
}

// BT.cpp:611-685 for one planner
bool bsplineTraj::optimizeTrajectory() {
    std::vector<bsplineTraj*> one{this};
    // makePlanBatch's inner loop without the A* prologue
    Rebound r;
    reboundBegin(r);
    solveBatch(one);
    const double t0 = wallSeconds();
    while (!r.done) {
        std::vector<uint8_t> col, dyn;
        gateBatch(one, col, dyn);
        reboundStep(r, col[0] != 0, dyn[0] != 0, wallSeconds() - t0 > 0.03);
        if (!r.done && r.needOptimize) solveBatch(one);
    }
    return r.ok;
}

namespace {
using vigo_host::Companion;
std::atomic<size_t> g_pipelineThreshold{2048};
thread_local bool t_insidePipeline = false;

// one opt-in device stage of makePlanBatch: its setting, and over the process how many of its work items the device
// decided and how many ran on the host instead
struct StageSwitch {
    std::atomic<int> mode{0};
    std::atomic<long long> deviceDecided{0}, hostRun{0};
    void totals(long long* decided, long long* host) const {
        if (decided) *decided = deviceDecided.load();
        if (host) *host = hostRun.load();
    }
};
StageSwitch g_astar, g_guides, g_prologue, g_reguide;
std::atomic<long long> g_prologueNs{0}, g_prologueChainNs{0};
std::atomic<int> g_deviceAstarBudget{16384};
constexpr int kAstarPathCap = 128;   // path points a device search returns (a longer path is searched again by the host)
int onOffOrTwin(int mode) { return mode == 1 || mode == 2 ? mode : 0; }
}  // namespace
void bsplineTraj::setBatchPipelineThreshold(size_t planners) { g_pipelineThreshold.store(planners); }

void bsplineTraj::setDeviceAstar(bool on) { g_astar.mode.store(on); }
bool bsplineTraj::deviceAstar() { return g_astar.mode.load() != 0; }
void bsplineTraj::setDeviceAstarBudget(int maxExpansions) { g_deviceAstarBudget.store(maxExpansions < 0 ? 0 : maxExpansions); }
void bsplineTraj::deviceAstarTotals(long long* deviceDecided, long long* hostRun, double* prologueSeconds) {
    g_astar.totals(deviceDecided, hostRun);
    if (prologueSeconds) *prologueSeconds = g_prologueNs.load() * 1e-9;
}
void bsplineTraj::setDeviceGuides(int mode) { g_guides.mode.store(onOffOrTwin(mode)); }
int bsplineTraj::deviceGuides() { return g_guides.mode.load(); }
void bsplineTraj::deviceGuideTotals(long long* deviceDecided, long long* hostRun) { g_guides.totals(deviceDecided, hostRun); }
void bsplineTraj::setDevicePrologue(bool on) { g_prologue.mode.store(on); }
bool bsplineTraj::devicePrologue() { return g_prologue.mode.load() != 0; }
void bsplineTraj::devicePrologueTotals(long long* deviceDecided, long long* hostRun, double* chainSeconds) {
    g_prologue.totals(deviceDecided, hostRun);
    if (chainSeconds) *chainSeconds = g_prologueChainNs.load() * 1e-9;
}
void bsplineTraj::setDeviceReguide(int mode) { g_reguide.mode.store(onOffOrTwin(mode)); }
int bsplineTraj::deviceReguide() { return g_reguide.mode.load(); }
void bsplineTraj::deviceReguideTotals(long long* deviceDecided, long long* hostRun) { g_reguide.totals(deviceDecided, hostRun); }

// one unsplit makePlanBatch call: per planner (index into the call's planners) its loop state and result; the planners
// still in the loop, in call order, with their indices
struct bsplineTraj::PlanBatch {
    std::vector<Rebound> rb;
    std::vector<bool> result;
    std::vector<bsplineTraj*> active;
    std::vector<size_t> activeIdx;
    std::atomic<long long> nsSeg{0}, nsAstar{0}, nsGuide{0};   // prologue CPU time summed over the worker threads
    std::atomic<long long> nsChain{0};                         // setDevicePrologue: wall time of the device chains (all three steps)
    explicit PlanBatch(size_t P) : rb(P), result(P, false) {}
    // step 1 of planner p and, with `search`, step 2 on the calling worker, timed; false: its A* failed
    bool hostSteps(bsplineTraj* p, bool search) {
        const double t0 = wallSeconds();
        p->findCollisionSeg(p->optData_.controlPoints, p->collisionSeg_);           // step 1
        const double t1 = wallSeconds();
        nsSeg += (long long)((t1 - t0) * 1e9);
        if (!search) return true;
        const bool found = p->pathSearch(p->collisionSeg_, p->astarPaths_);         // step 2
        nsAstar += (long long)((wallSeconds() - t1) * 1e9);
        return found;
    }
};

// BT.cpp:333-385 for many planners at once: host prologue per planner, then the rebound loops in
// lock-step so each optimize() round is one launch over all still-active planners.
std::vector<bool> bsplineTraj::makePlanBatch(const std::vector<bsplineTraj*>& planners) {
    const size_t P = planners.size();
    const size_t threshold = g_pipelineThreshold.load();
    if (!t_insidePipeline && threshold > 0 && P >= threshold && P >= 2) return makePlanPipelined(planners, threshold);
    PlanBatch pb(P);
    const bool timing = getenv("VIGO_FACADE_TIMING") != nullptr;
    const double tp0 = wallSeconds();
    planPrologue(planners, pb);
    const double tp1 = wallSeconds();
    g_prologueNs += (long long)((tp1 - tp0) * 1e9);
    // step 4: rebound loops.  The 30 ms budget of BT.cpp:633 is per makePlan() call in the
    // reference; a batch keeps it per round so one slow planner cannot starve the others.
    if (deviceResidentRebound()) reboundOnDevice(pb, timing);
    else reboundFromHost(pb, timing);
    const double tp2 = wallSeconds();
    planEpilogue(planners, pb.result);
    if (timing) {
        cout << "[BsplineTraj]: prologue CPU time summed over the workers: findCollisionSeg " << pb.nsSeg.load() * 1e-6 << " ms, A* "
             << pb.nsAstar.load() * 1e-6 << " ms, guide assignment " << pb.nsGuide.load() * 1e-6 << " ms; device chains (wall) "
             << pb.nsChain.load() * 1e-6 << " ms" << endl;
        cout << "[BsplineTraj]: makePlanBatch of " << P << ": prologue " << (tp1 - tp0) * 1e3 << " ms, rebound loop " << (tp2 - tp1) * 1e3
             << " ms, epilogue " << (wallSeconds() - tp2) * 1e3 << " ms" << endl;
    }
    return pb.result;
}

// A large batch runs as two to four pipelined parts of >= threshold / 2 planners, all but the first on companion
// host threads with their own handles and HIP streams: while one part waits for its device rounds (a chain of
// single-wave solves, ~10 ms per 1024 planners) the others' host work (A*, guide assignment) and device rounds
// proceed — what a caller otherwise gets only by planning from several threads of its own.  Planners are independent
// (per-trajectory results do not depend on which batch carries them), so the plans are those of the unsplit call.
std::vector<bool> bsplineTraj::makePlanPipelined(const std::vector<bsplineTraj*>& planners, size_t threshold) {
    constexpr size_t kMaxParts = 4;
    static thread_local Companion companions[kMaxParts - 1];
    const size_t P = planners.size();
    const size_t per = threshold / 2 > 0 ? threshold / 2 : 1;
    const size_t parts = std::min(kMaxParts, std::max<size_t>(2, P / per));
    std::vector<std::vector<bsplineTraj*>> piece(parts);
    std::vector<std::vector<bool>> res(parts);
    for (size_t k = 0; k < parts; ++k) {
        const size_t lo = P * k / parts, hi = P * (k + 1) / parts;
        piece[k].assign(planners.begin() + lo, planners.begin() + hi);
        res[k].assign(hi - lo, false);
    }
    for (size_t k = 1; k < parts; ++k) {
        companions[k - 1].start([&piece, &res, k]() {
            t_insidePipeline = true;
            res[k] = bsplineTraj::makePlanBatch(piece[k]);
        });
    }
    // the jobs hold piece and res: every part has ended before an exception leaves (the first one in part order)
    std::exception_ptr err;
    t_insidePipeline = true;
    try { res[0] = bsplineTraj::makePlanBatch(piece[0]); } catch (...) { err = std::current_exception(); }
    t_insidePipeline = false;
    for (size_t k = 1; k < parts; ++k)
        try { companions[k - 1].wait(); } catch (...) { if (!err) err = std::current_exception(); }
    if (err) std::rethrow_exception(err);
    std::vector<bool> all;
    for (size_t k = 0; k < parts; ++k) all.insert(all.end(), res[k].begin(), res[k].end());
    return all;
}

// steps 1-3 (collision segments, A*, guide assignment) touch only the planner's own state and the read-only map: the
// planners are spread over the host cores.  Those that get through enter the rebound loop.
void bsplineTraj::planPrologue(const std::vector<bsplineTraj*>& planners, PlanBatch& pb) {
    const size_t P = planners.size();
    std::vector<uint8_t> prepared(P, 0), hasPaths(P, 0);
    const int guides = devicePrologue() ? 0 : deviceGuides();
    if (devicePrologue()) {
        // the three steps as one device chain per group; what the device does not decide runs the host steps there too
        std::vector<uint8_t> outcome(P, 0);
        prologueOnDevice(planners, pb, outcome);
        for (size_t i = 0; i < P; ++i) prepared[i] = outcome[i] == 1;
    } else {
        // The host steps, per planner on the workers, all three in one pass.  setDeviceAstar gathers step 2 over the
        // planners (pathSearchBatch: the searches of all of them on the device): steps 1 and 3 are then a pass each
        // around it.  setDeviceGuides gathers step 3 (below).
        const bool gathered = deviceAstar();
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
            pathSearchBatch(planners, ready, hasPaths);                                 // step 2
            pb.nsAstar += (long long)((wallSeconds() - t1) * 1e9);
            if (guides == 0)
                parallelFor(P, [&](size_t i) {
                    if (hasPaths[i]) assignGuides(i);
                });
        }
    }
    if (guides != 0) {
        // step 3 gathered over the planners (setDeviceGuides): the device, or its twin on the workers
        const double t2 = wallSeconds();
        assignGuidesBatch(planners, hasPaths);
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

#ifdef VIGO_WITH_ROS
namespace {
// The snapshot of this map type covers the planner's region only, and the device takes everything outside it for occupied
// while the host asks the map itself: what a device stage may read has to lie inside the region.  This is the test:
// the axis-aligned box of the n points xyz (triples), grown by half[k] along axis k, lies inside R, bounds included.
// (No region set, or a NaN coordinate: it does not.  No points: it does.)
bool boxInRegion(const mapRegion& R, const double* xyz, size_t n, const double half[3]) {
    if (!R.set) return false;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (size_t q = 0; q < 3 * n; ++q) {
        const double v = xyz[q];
        if (v < lo[q % 3] || std::isnan(v)) lo[q % 3] = v;       // (a NaN stays: nothing compares below or above it)
        if (v > hi[q % 3] || std::isnan(v)) hi[q % 3] = v;
    }
    for (int k = 0; k < 3; ++k)
        if (!(lo[k] - half[k] >= R.boxMin(k) && hi[k] + half[k] <= R.boxMax(k))) return false;
    return true;
}
}  // namespace
#endif

// one AstarSearch(res, pStart, pEnd) of planner `planner`: from the start of segment `seg` to the end of segment `endSeg`
struct bsplineTraj::AstarJob {
    size_t planner;
    int seg, endSeg;
    Eigen::Vector3d s, e;
    bool ok = false;                       // AstarSearch's return value
    std::vector<Eigen::Vector3d> path;     // getPath()
};

// The jobs' searches: one vigo_astar_search per group of planners that share a snapshot, a node pool and a height band;
// what the device does not decide (deferred, path too long, no device or snapshot) is searched by the planner's own
// host A* on the workers.
void bsplineTraj::runAstarJobs(const std::vector<bsplineTraj*>& planners, std::vector<AstarJob>& jobs) {
    if (jobs.empty()) return;
    const size_t P = planners.size();
    std::vector<uint8_t> decided(jobs.size(), 0);
    std::vector<std::vector<size_t>> jobsOf(P);
    for (size_t j = 0; j < jobs.size(); ++j) jobsOf[jobs[j].planner].push_back(j);
    std::vector<size_t> owners;                       // the planners with jobs, in call order
    for (size_t i = 0; i < P; ++i)
        if (!jobsOf[i].empty()) owners.push_back(i);
    auto same = [&](size_t a, size_t b) { return SearchGroup::same(*planners[owners[a]], *planners[owners[b]]); };
    vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
        bsplineTraj* lead = planners[owners[members[0]]];
        if (!lead->syncDevice()) return;
        const SearchGroup g(*lead);
        if (!g.valid(false)) return;
        std::vector<size_t> idx;
        std::vector<double> se[2];
        for (size_t m : members)
            for (size_t j : jobsOf[owners[m]]) {
#ifdef VIGO_WITH_ROS
                // a search whose node pool (around the midpoint of its ends) is not inside the region stays with the host
                const double mid[3] = {(jobs[j].s(0) + jobs[j].e(0)) / 2, (jobs[j].s(1) + jobs[j].e(1)) / 2, (jobs[j].s(2) + jobs[j].e(2)) / 2};
                if (!boxInRegion(planners[owners[m]]->link_.region(), mid, 1, g.half)) continue;
#endif
                idx.push_back(j);
                for (int k = 0; k < 3; ++k) { se[0].push_back(jobs[j].s(k)); se[1].push_back(jobs[j].e(k)); }
            }
        const int Q = (int)idx.size();
        if (Q == 0) return;
        static thread_local StagingBuf dS, dE, dStatus, dLen, dPath;
        if (!dS.upload(se[0].data(), se[0].size() * 8) || !dE.upload(se[1].data(), se[1].size() * 8) || !dStatus.alloc((size_t)Q * 4) ||
            !dLen.alloc((size_t)Q * 4) || !dPath.alloc((size_t)Q * kAstarPathCap * 24))
            return;
        if (vigo_astar_search(lead->link_.handle(), Q, (const double*)dS.p, (const double*)dE.p, g.res, g.pool, lead->minHeight_, lead->maxHeight_,
                              g_deviceAstarBudget.load(), kAstarPathCap, (int32_t*)dStatus.p, (int32_t*)dLen.p, (double*)dPath.p,
                              nullptr) != VIGO_OK) {
            cout << "[BsplineTraj]: vigo_astar_search failed: " << vigo_last_error(lead->link_.handle()) << endl;
            return;
        }
        std::vector<int32_t> status(Q), len(Q);
        std::vector<double> path((size_t)Q * kAstarPathCap * 3);
        if (!vigo_host::threadSync() || !dStatus.download(status.data(), (size_t)Q * 4) || !dLen.download(len.data(), (size_t)Q * 4) ||
            !dPath.download(path.data(), path.size() * 8))
            return;
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
    g_astar.deviceDecided += nDecided;
    g_astar.hostRun += (long long)jobs.size() - nDecided;
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
void bsplineTraj::pathSearchBatch(const std::vector<bsplineTraj*>& planners, const std::vector<uint8_t>& ready, std::vector<uint8_t>& found) {
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
    runAstarJobs(planners, first);
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
    runAstarJobs(planners, retry);
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
bool downloadPathsAndPairs(int S, long long pointCap, long long nPairs, const StagingBuf& dPathOff, const StagingBuf& dPath, const StagingBuf& dPv,
                           std::vector<int32_t>& pathOff, std::vector<double>& path, std::vector<double>& pv) {
    pathOff.assign((size_t)S + 1, 0);
    if (S > 0 && !dPathOff.download(pathOff.data(), pathOff.size() * 4)) return false;
    if (pathOff[S] < 0 || pathOff[S] > pointCap) return false;
    path.resize((size_t)pathOff[S] * 3);
    pv.resize((size_t)nPairs * 6);
    return (path.empty() || dPath.download(path.data(), path.size() * 8)) && (pv.empty() || dPv.download(pv.data(), pv.size() * 8));
}
}  // namespace

// Steps 1-3 for all planners under setDevicePrologue(true).  Per group of planners that share a batch key and a node
// pool: control points up, vigo_path_search on the scanned segments, vigo_guide_assign on its output (device pointers,
// nothing repacked), then one round of downloads and the results installed per planner.  What is left (see the header)
// runs findCollisionSeg -> pathSearch -> assignGuidesCore on the workers.
// Buffer sizes: segCap = B * VIGO_MAX_COLLISION_SEGS is the entry's own bound.  pointCap = B * 2 * (kAstarPathCap + 1) and
// pairCap = B * N * 4 are budgets, not bounds (the bounds, 48 full-length paths per planner and every path point a pair,
// would be ~150 MB per 1024 planners): two full-length paths and four pairs per control point on AVERAGE over the
// group, against 17 path points and 4.4 pairs per PLANNER on the pipeline batches.  A group over pointCap gets
// VIGO_ERR_INVALID_ARG from vigo_path_search (nothing written, the message is printed) and runs the host steps as a
// whole; a group over pairCap keeps the device's segments and paths and has the twin assign its guides.  Both are
// correct and slow, and both show in devicePrologueTotals' hostRun.
void bsplineTraj::prologueOnDevice(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, std::vector<uint8_t>& outcome) {
    const size_t P = planners.size();
    std::vector<uint8_t> needGuides(P, 0);            // segments and paths are installed, the pairs are not
    std::vector<uint8_t> failedOnDevice(P, 0);        // the device's walk failed: the host's replay leaves the lists
    std::vector<size_t> owners;
    for (size_t i = 0; i < P; ++i)
        if (planners[i]->init_ && planners[i]->link_.map()) owners.push_back(i);
    auto same = [&](size_t a, size_t b) { return SearchGroup::same(*planners[owners[a]], *planners[owners[b]]); };
    const double tc0 = wallSeconds();
    vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
        bsplineTraj* lead = planners[owners[members[0]]];
        if (!lead->syncDevice()) return;
        const SearchGroup g(*lead);
        const int N = g.N;
        if (!g.valid(true)) return;
        std::vector<size_t> who;
        std::vector<double> ctrl;
        for (size_t m : members) {
            const bsplineTraj* p = planners[owners[m]];
#ifdef VIGO_WITH_ROS
            // Every search's node pool (around the midpoint of two control points) and with it every path point lies in
            // the control points' box grown by the pool's reach: a planner whose grown box is not inside the region
            // keeps to its own map.
            if (!boxInRegion(p->link_.region(), p->optData_.controlPoints.data(), N, g.half)) continue;
#endif
            vigo_host::appendCtrl(p->optData_.controlPoints, ctrl);
            who.push_back(owners[m]);
        }
        const int B = (int)who.size();
        if (B == 0) return;
        const long long segCap = (long long)B * VIGO_MAX_COLLISION_SEGS, pointCap = (long long)B * 2 * (kAstarPathCap + 1),
                        pairCap = (long long)B * N * 4;
        static thread_local StagingBuf dCtrl, dStatus, dSegOff, dSeg, dPathOff, dPath, dCounts, dOff, dPv, dGStatus;
        if (!dCtrl.upload(ctrl.data(), ctrl.size() * 8) || !dStatus.alloc((size_t)B * 4) || !dSegOff.alloc(((size_t)B + 1) * 4) ||
            !dSeg.alloc((size_t)segCap * 8) || !dPathOff.alloc(((size_t)segCap + 1) * 4) || !dPath.alloc((size_t)pointCap * 24) ||
            !dCounts.alloc((size_t)B * 8) || !dOff.alloc(((size_t)B * N + 1) * 4) || !dPv.alloc((size_t)pairCap * 48) || !dGStatus.alloc((size_t)B * 4))
            return;
        if (vigo_path_search(lead->link_.handle(), B, N, (const double*)dCtrl.p, nullptr, nullptr, lead->notCheckRatio_, g.res, g.pool, lead->minHeight_,
                             lead->maxHeight_, g_deviceAstarBudget.load(), kAstarPathCap, segCap, pointCap, (int32_t*)dStatus.p,
                             (int32_t*)dSegOff.p, (int32_t*)dSeg.p, (int32_t*)dPathOff.p, (double*)dPath.p, (int32_t*)dCounts.p) != VIGO_OK) {
            cout << "[BsplineTraj]: vigo_path_search failed: " << vigo_last_error(lead->link_.handle()) << endl;
            return;
        }
        const bool guided = vigo_guide_assign(lead->link_.handle(), B, N, (const double*)dCtrl.p, (const int32_t*)dSegOff.p, (const int32_t*)dSeg.p,
                                              (const int32_t*)dPathOff.p, (const double*)dPath.p, pairCap, (int32_t*)dOff.p, (double*)dPv.p,
                                              nullptr, (int32_t*)dGStatus.p) == VIGO_OK;   // (not: the pairs do not fit — the twin assigns them)
        std::vector<int32_t> status(B), segOff(B + 1), counts((size_t)B * 2), off((size_t)B * N + 1, 0), gstatus(B, VIGO_GUIDE_DEFERRED);
        if (!vigo_host::threadSync() || !dStatus.download(status.data(), (size_t)B * 4) || !dSegOff.download(segOff.data(), ((size_t)B + 1) * 4) ||
            !dCounts.download(counts.data(), counts.size() * 4))
            return;
        if (guided && (!dOff.download(off.data(), off.size() * 4) || !dGStatus.download(gstatus.data(), (size_t)B * 4))) return;
        const int S = segOff[B];
        if (S < 0 || S > segCap || off.back() < 0 || off.back() > pairCap) return;
        std::vector<int32_t> seg((size_t)S * 2), pathOff;
        std::vector<double> path, pv;
        if (S > 0 && !dSeg.download(seg.data(), seg.size() * 4)) return;
        if (!downloadPathsAndPairs(S, pointCap, off.back(), dPathOff, dPath, dPv, pathOff, path, pv)) return;
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
            vigo_host::installGuides(p->optData_, N, off.data() + (size_t)b * N, pv.data());
            outcome[who[b]] = 1;
        }
    });
    const long long chainNs = (long long)((wallSeconds() - tc0) * 1e9);
    pb.nsChain += chainNs;
    g_prologueChainNs += chainNs;
    long long nDecided = 0;
    for (size_t i : owners) nDecided += (outcome[i] != 0 && !needGuides[i]) || failedOnDevice[i];
    g_prologue.deviceDecided += nDecided;
    g_prologue.hostRun += (long long)owners.size() - nDecided;
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
void bsplineTraj::assignGuidesBatch(const std::vector<bsplineTraj*>& planners, const std::vector<uint8_t>& found) {
    const size_t P = planners.size();
    std::vector<uint8_t> done(P, 0);
    if (deviceGuides() == 1) {
        std::vector<size_t> owners;
        for (size_t i = 0; i < P; ++i)
            if (found[i]) owners.push_back(i);
        auto same = [&](size_t a, size_t b) {
            const bsplineTraj* x = planners[owners[a]];
            const bsplineTraj* y = planners[owners[b]];
            return x->sameBatchKey(*y) && x->optData_.controlPoints.cols() == y->optData_.controlPoints.cols();
        };
        vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
            bsplineTraj* lead = planners[owners[members[0]]];
            if (!lead->syncDevice()) return;
            const int N = lead->optData_.controlPoints.cols();
            std::vector<size_t> who;
            std::vector<double> ctrl, path;
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
                for (size_t k = seg0; k < seg.size() / 2; ++k) pairs += vigo::guide_pushes_total(N, seg[2 * k], seg[2 * k + 1]);
                segOff.push_back((int32_t)(seg.size() / 2));
                vigo_host::appendCtrl(p->optData_.controlPoints, ctrl);
                who.push_back(owners[m]);
            }
            const int B = (int)who.size();
            if (B == 0) return;
            if (seg.empty()) {                       // no segments anywhere: nothing to assign
                for (size_t i : who) done[i] = 1;
                return;
            }
            const long long cap = std::max<long long>(pairs, 1);
            static thread_local StagingBuf dCtrl, dSegOff, dSeg, dPathOff, dPath, dOff, dPv, dStatus;
            if (!dCtrl.upload(ctrl.data(), ctrl.size() * 8) || !dSegOff.upload(segOff.data(), segOff.size() * 4) ||
                !dSeg.upload(seg.data(), seg.size() * 4) || !dPathOff.upload(pathOff.data(), pathOff.size() * 4) ||
                !dPath.upload(path.data(), path.size() * 8) || !dOff.alloc(((size_t)B * N + 1) * 4) || !dPv.alloc((size_t)cap * 48) ||
                !dStatus.alloc((size_t)B * 4))
                return;
            if (vigo_guide_assign(lead->link_.handle(), B, N, (const double*)dCtrl.p, (const int32_t*)dSegOff.p, (const int32_t*)dSeg.p,
                                  (const int32_t*)dPathOff.p, (const double*)dPath.p, cap, (int32_t*)dOff.p, (double*)dPv.p, nullptr,
                                  (int32_t*)dStatus.p) != VIGO_OK) {
                cout << "[BsplineTraj]: vigo_guide_assign failed: " << vigo_last_error(lead->link_.handle()) << endl;
                return;
            }
            std::vector<int32_t> off((size_t)B * N + 1), status(B);
            if (!vigo_host::threadSync() || !dOff.download(off.data(), off.size() * 4) || !dStatus.download(status.data(), (size_t)B * 4)) return;
            std::vector<double> pv((size_t)off.back() * 6);
            if (off.back() < 0 || off.back() > cap || (!pv.empty() && !dPv.download(pv.data(), pv.size() * 8))) return;
            for (int b = 0; b < B; ++b) {
                if (status[b] != VIGO_GUIDE_OK) continue;
                vigo_host::installGuides(planners[who[b]]->optData_, N, off.data() + (size_t)b * N, pv.data());
                done[who[b]] = 1;
            }
        });
    }
    long long nDone = 0, nFound = 0;
    for (size_t i = 0; i < P; ++i) { nDone += done[i]; nFound += found[i] ? 1 : 0; }
    g_guides.deviceDecided += nDone;
    g_guides.hostRun += nFound - nDone;
    parallelFor(P, [&](size_t i) {
        if (found[i] && !done[i]) planners[i]->assignGuidesCore();
    });
}

namespace {
std::mutex g_reguideLogMutex;
std::vector<bsplineTraj::ReguideStepRecord>* g_reguideLog = nullptr;
}  // namespace
void bsplineTraj::setReguideStepLog(std::vector<ReguideStepRecord>* log) {
    std::lock_guard<std::mutex> lock(g_reguideLogMutex);
    g_reguideLog = log;
}

// the planners vigo_rebound_reguide works on (vigo.h): what is left of the NEEDS_HOST ones is the forced A* of
// failCount >= 4 and the planners with a dynamic collision only
bool bsplineTraj::reguideEligible(const Rebound& r) { return r.devStatus == VIGO_RB_NEEDS_HOST && r.gateStatic && r.failCount < 4; }

// reboundStep for such a planner with the guide step's twin in place of assignGuidePointsSemiCircle: what
// vigo_rebound_reguide computes (csrc/vigo_reguide_core.hpp restates isReguideRequired, vigo_path_search the host's
// pathSearch), without its capacities
void bsplineTraj::reguideStepCore(Rebound& r) {
    if (g_reguideLog) {
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
        std::lock_guard<std::mutex> lock(g_reguideLogMutex);
        if (g_reguideLog) g_reguideLog->push_back(std::move(rec));
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

// setDeviceReguide(1): per group of planners that share a batch key and a node pool, the eligible ones as one staged
// batch (control points, guide CSR, weights, state) through vigo_rebound_reguide, one round of downloads, the results
// installed per planner.  pairCap: the old pairs plus four new ones per control point on average over the group, and
// pointCap two full-length paths per planner, are budgets as in prologueOnDevice: a group over either gets
// VIGO_ERR_INVALID_ARG (nothing written, the message is printed) and runs the twin on the workers.
void bsplineTraj::reguideOnDevice(PlanBatch& pb, const std::vector<uint8_t>& devOk) {
    std::vector<bsplineTraj*>& active = pb.active;
    std::vector<size_t> owners;
    for (size_t a = 0; a < active.size(); ++a)
        if (devOk[a] && reguideEligible(pb.rb[pb.activeIdx[a]]) && active[a]->collisionSeg_.size() <= (size_t)VIGO_MAX_COLLISION_SEGS) owners.push_back(a);
    auto same = [&](size_t a, size_t b) { return SearchGroup::same(*active[owners[a]], *active[owners[b]]); };
    long long nDecided = 0;
    vigo_host::forEachGroup(owners.size(), same, [&](const std::vector<size_t>& members) {
        bsplineTraj* lead = active[owners[members[0]]];
        if (!lead->syncDevice()) return;
        const SearchGroup g(*lead);
        const int N = g.N;
        if (!g.valid(true) || N > VIGO_MAX_CTRL_POINTS) return;
        std::vector<size_t> who;
        HostBatch hb(N);
        std::vector<vigo_rebound_state_t> state;
        for (size_t m : members) {
            const size_t a = owners[m];
            const bsplineTraj* p = active[a];
#ifdef VIGO_WITH_ROS
            // as in prologueOnDevice: a planner whose control points' box, grown by the node pool's reach, is not inside
            // the region keeps to its own map
            if (!boxInRegion(p->link_.region(), p->optData_.controlPoints.data(), N, g.half)) continue;
#endif
            const Rebound& r = pb.rb[pb.activeIdx[a]];
            hb.add(p->optData_.controlPoints.data(), p->optData_, {p->weightDistance_, p->weightSmoothness_, p->weightFeasibility_, p->weightDynamicObstacle_});
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
            who.push_back(a);
        }
        const int B = (int)who.size();
        if (B == 0) return;
        const long long segCap = (long long)B * VIGO_MAX_COLLISION_SEGS, pointCap = (long long)B * 2 * (kAstarPathCap + 1),
                        pairCap = (long long)hb.guides() + (long long)B * N * 4;
        static thread_local StagingBuf dState, dOff, dPv, dPathSegOff, dPathOff, dPath, dStatus;
        DeviceBatch d;
        if (!uploadBatch(lead->link_.handle(), hb, d) || !dState.upload(state.data(), state.size() * sizeof(vigo_rebound_state_t)) ||
            !dOff.alloc(((size_t)B * N + 1) * 4) || !dPv.alloc((size_t)pairCap * 48) || !dPathSegOff.alloc(((size_t)B + 1) * 4) ||
            !dPathOff.alloc(((size_t)segCap + 1) * 4) || !dPath.alloc((size_t)pointCap * 24) || !dStatus.alloc((size_t)B * 4))
            return;
        if (vigo_rebound_reguide(lead->link_.handle(), B, N, d.ctrl, d.gpv ? d.goff : nullptr, d.gpv, d.gunk, d.weights,   // (no pairs at all: "no guides")
                                 lead->notCheckRatio_, g.res, g.pool, lead->minHeight_,
                                 lead->maxHeight_, g_deviceAstarBudget.load(), kAstarPathCap, (vigo_rebound_state_t*)dState.p, pairCap,
                                 (int32_t*)dOff.p, (double*)dPv.p, nullptr, segCap, pointCap, (int32_t*)dPathSegOff.p, (int32_t*)dPathOff.p,
                                 (double*)dPath.p, (int32_t*)dStatus.p) != VIGO_OK) {
            cout << "[BsplineTraj]: vigo_rebound_reguide failed: " << vigo_last_error(lead->link_.handle()) << endl;
            return;
        }
        std::vector<int32_t> status(B), off((size_t)B * N + 1), pathSegOff(B + 1);
        if (!vigo_host::threadSync() || !dStatus.download(status.data(), (size_t)B * 4) || !dOff.download(off.data(), off.size() * 4) ||
            !dPathSegOff.download(pathSegOff.data(), pathSegOff.size() * 4) ||
            !dState.download(state.data(), state.size() * sizeof(vigo_rebound_state_t)) ||
            !vigo_host::download(hb.weights.data(), d.weights, hb.weights.size() * 8))
            return;
        const int S = pathSegOff[B];
        if (S < 0 || S > segCap || off.back() < 0 || off.back() > pairCap) return;
        std::vector<int32_t> pathOff;
        std::vector<double> path, pv;
        if (!downloadPathsAndPairs(S, pointCap, off.back(), dPathOff, dPath, dPv, pathOff, path, pv)) return;
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
                vigo_host::installGuides(p->optData_, N, off.data() + (size_t)b * N, pv.data(), true);
            }
            p->weightDistance_ = hb.weights[4 * (size_t)b + 0];
            p->weightDynamicObstacle_ = hb.weights[4 * (size_t)b + 3];
            r.failCount = st.fail_count;
            r.needOptimize = st.solve_first != 0;
            r.devStatus = st.status;                   // VIGO_RB_ACTIVE: the step is done
            ++nDecided;
        }
    });
    g_reguide.deviceDecided += nDecided;
}

// The loop runs on the device between two A* calls (vigo_rebound_rounds): gates, success exit, isReguideRequired,
// weight doubling and re-solve are queued for up to kRounds rounds without a host round trip; the host only sees
// the planners that are done, need A* (re-guide, or failCount >= 4) or ran out of queued rounds.  Under
// setDeviceReguide the re-guide step is vigo_rebound_reguide's (or its twin's on the workers).
void bsplineTraj::reboundOnDevice(PlanBatch& pb, bool timing) {
    const int kRounds = 4;   // failCount reaches 4 after at most four device rounds: then every round needs A*
    std::vector<bsplineTraj*>& active = pb.active;
    auto same = [&](size_t a, size_t b) { return active[a]->sameBatchKey(*active[b]); };
    const double t0 = wallSeconds();
    const double budget = 0.03 * std::max<size_t>(1, active.size());
    while (!active.empty()) {
        const double tr0 = wallSeconds();
        // one device batch per group of planners the lead's handle state fits
        std::vector<uint8_t> devOk(active.size(), 0);
        vigo_host::forEachGroup(active.size(), same, [&](const std::vector<size_t>& members) {
            std::vector<bsplineTraj*> grp;
            std::vector<Rebound*> grb;
            for (size_t m : members) {
                grp.push_back(active[m]);
                grb.push_back(&pb.rb[pb.activeIdx[m]]);
            }
            const bool ok = deviceRounds(grp, grb, kRounds);
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
        // the re-guide step of the planners the device takes (setDeviceReguide); out of time, every planner leaves below
        const int reguide = timedOut ? 0 : deviceReguide();
        if (reguide == 1) reguideOnDevice(pb, devOk);
        size_t nHost = 0;
        long long nTwin = 0;
        for (size_t a = 0; a < active.size(); ++a) {
            nHost += pb.rb[pb.activeIdx[a]].devStatus == VIGO_RB_NEEDS_HOST ? 1 : 0;
            nTwin += reguide != 0 && devOk[a] && reguideEligible(pb.rb[pb.activeIdx[a]]) ? 1 : 0;
        }
        g_reguide.hostRun += nTwin;
        parallelFor(active.size(), [&](size_t a) {
            Rebound& r = pb.rb[pb.activeIdx[a]];
            bsplineTraj* p = active[a];
            if (!devOk[a]) { p->reboundFinish(r, false); return; }             // no device: nothing to plan with
            if (r.devStatus == VIGO_RB_DONE) p->reboundFinish(r, true);          // BT.cpp:628-631
            else if (reguide != 0 && reguideEligible(r)) p->reguideStepCore(r);  // what the device left, or setting 2: its twin
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
    solveBatch(active);
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
        solveBatch(solve);
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

// steps 5-6 for the planners that succeeded
void bsplineTraj::planEpilogue(const std::vector<bsplineTraj*>& planners, const std::vector<bool>& result) {
    std::vector<uint8_t> okv(result.begin(), result.end());
    parallelFor(planners.size(), [&](size_t i) {
        if (!okv[i]) return;
        bsplineTraj* p = planners[i];
        p->bspline_ = trajPlanner::bspline(bsplineDegree, p->optData_.controlPoints, p->controlPointsTs_);  // step 5
        p->linearFeasibilityReparam();                                                                  // step 6
    });
}

// BT.cpp:754-793 — including the function-static previous goal distance shared by all instances
void bsplineTraj::adjustPathLengthDirect(const std::vector<Eigen::Vector3d>& path, std::vector<Eigen::Vector3d>& adjustedPath) {
    double prevOut = 0.0;
    this->adjustPathLengthWith(path, adjustedPath, g_prevPathLength.load(), prevOut);
    g_prevPathLength.store(prevOut);
}

void bsplineTraj::adjustPathLengthWith(const std::vector<Eigen::Vector3d>& path, std::vector<Eigen::Vector3d>& adjustedPath, double prevIn,
                                       double& prevOut) {
    const double prevPathLength = prevIn;
    prevOut = prevIn;
    if (path.empty()) return;
    double totalLength = 0.0;
    bool exceedLength = false;
    double minLength = 0.0;
    Eigen::Vector3d pStart = path[0];
    for (size_t i = 0; i + 1 < path.size(); ++i) {
        Eigen::Vector3d p1 = path[i], p2 = path[i + 1];
        totalLength = (p2 - pStart).norm();
        if (totalLength >= std::max(prevPathLength, this->maxPathLength_)) exceedLength = true;
        adjustedPath.push_back(p1);
        if (exceedLength) {
            bool free = !this->link_.map()->isInflatedOccupiedLine(p1, p2);
            if (free && minLength >= 1.5) {
                adjustedPath.push_back(p2);
                prevOut = totalLength;
                return;
            }
        }
        if (this->link_.map()->isInflatedOccupiedLine(p1, p2)) minLength = 0.0;
        else minLength += (p2 - p1).norm();
    }
    adjustedPath.push_back(path.back());
    prevOut = totalLength;
}

// BT.cpp:1116-1137
void bsplineTraj::linearFeasibilityReparam() {
    double trajMaxVel = 0.0, trajMaxAcc = 0.0;
    trajPlanner::bspline trajVel = this->bspline_.getDerivative();
    trajPlanner::bspline trajAcc = trajVel.getDerivative();
    for (double t = 0.0; t < this->bspline_.getDuration(); t += this->ts_) {
        trajMaxVel = std::max(trajMaxVel, trajVel.at(t).norm());
        trajMaxAcc = std::max(trajMaxAcc, trajAcc.at(t).norm());
    }
    double factorVel = this->maxVel_ / trajMaxVel;
    double factorAcc = std::sqrt(this->maxAcc_ / trajMaxAcc);
    this->linearFactor_ = std::min(factorVel, factorAcc);
}

double bsplineTraj::getLinearReparamTime(double t) { return this->linearFactor_ * t; }
double bsplineTraj::getLinearFactor() { return this->linearFactor_; }
double bsplineTraj::getInitTs() { return this->controlPointDistance_ / this->maxVel_; }
double bsplineTraj::getControlPointTs() { return this->controlPointsTs_; }
double bsplineTraj::getControlPointDist() { return this->controlPointDistance_; }
trajPlanner::bspline bsplineTraj::getTrajectory() { return this->bspline_; }

// BT.cpp:1402-1419
geometry_msgs::PoseStamped bsplineTraj::getPose(double t, bool yaw) {
    geometry_msgs::PoseStamped ps;
    Eigen::Vector3d p = this->bspline_.at(t);
    ps.header.frame_id = "map";
    ps.header.stamp = ros::Time::now();
    ps.pose.position.x = p(0);
    ps.pose.position.y = p(1);
    ps.pose.position.z = p(2);
    if (yaw) {
        trajPlanner::bspline velBspline = this->bspline_.getDerivative();
        Eigen::Vector3d vel = velBspline.at(t);
        ps.pose.orientation = trajPlanner::quaternion_from_rpy(0, 0, std::atan2(vel(1), vel(0)));
    }
    return ps;
}

double bsplineTraj::getDuration() { return this->bspline_.getDuration(); }
double bsplineTraj::getTimestep() { return this->ts_; }
Eigen::MatrixXd bsplineTraj::getControlPoints() { return this->optData_.controlPoints; }

std::vector<Eigen::Vector3d> bsplineTraj::evalTraj() { return this->evalTraj(this->link_.map()->getRes() / this->maxVel_ / 2.0); }

std::vector<Eigen::Vector3d> bsplineTraj::evalTraj(double dt) {
    std::vector<Eigen::Vector3d> traj;
    trajPlanner::bspline sp(bsplineDegree, this->optData_.controlPoints, this->controlPointsTs_);
    for (double t = 0; t <= sp.getDuration(); t += dt) traj.push_back(sp.at(t));
    return traj;
}

bool bsplineTraj::isCurrTrajValid() {
    if (!this->init_) return false;
    return !this->hasCollisionTrajectory(this->optData_.controlPoints);
}

// BT.h:327-342
bool bsplineTraj::isCurrTrajValid(Eigen::Vector3d& firstCollisionPos) {
    if (!this->init_) return false;
    std::vector<Eigen::Vector3d> trajectory = this->evalTraj();
    for (int i = 0; i < (1.0 - this->notCheckRatio_) * int(trajectory.size()); ++i) {
        if (this->link_.map()->isInflatedOccupied(trajectory[i])) {
            firstCollisionPos = trajectory[i];
            return false;
        }
    }
    return true;
}

nav_msgs::Path bsplineTraj::evalTrajToMsg(bool yaw) { return this->evalTrajToMsg(this->ts_, yaw); }

// BT.cpp:1502-1518
nav_msgs::Path bsplineTraj::evalTrajToMsg(double dt, bool yaw) {
    std::vector<Eigen::Vector3d> trajTemp = this->evalTraj(dt);
    nav_msgs::Path traj;
    this->eigenPointsToPathMsg(trajTemp, traj);
    trajPlanner::bspline velBspline = this->bspline_.getDerivative();
    for (size_t i = 0; i < traj.poses.size(); ++i) {
        Eigen::Vector3d vel = velBspline.at((double)i * dt);
        if (yaw) traj.poses[i].pose.orientation = trajPlanner::quaternion_from_rpy(0, 0, std::atan2(vel(1), vel(0)));
    }
    return traj;
}

void bsplineTraj::pathMsgToEigenPoints(const nav_msgs::Path& path, std::vector<Eigen::Vector3d>& points) {
    for (const auto& ps : path.poses) points.push_back(Eigen::Vector3d(ps.pose.position.x, ps.pose.position.y, ps.pose.position.z));
}

void bsplineTraj::eigenPointsToPathMsg(const std::vector<Eigen::Vector3d>& points, nav_msgs::Path& path) {
    path.poses.clear();
    for (const auto& q : points) {
        geometry_msgs::PoseStamped p;
        p.pose.position.x = q(0);
        p.pose.position.y = q(1);
        p.pose.position.z = q(2);
        path.poses.push_back(p);
    }
    path.header.frame_id = "map";
}

}  // namespace trajPlanner
