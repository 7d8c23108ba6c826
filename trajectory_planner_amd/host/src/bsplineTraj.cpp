// bsplineTraj.cpp — trajPlanner::bsplineTraj over the MI355X back-end.
//
// Behaviour follows the reference's bsplineTraj.{h,cpp} (cited per function as BT.cpp / BT.h);
// the numerics of optimize(), the collision gates and isUnknown(guide) run in libvigo_hip.so
// through the C ABI of include/vigo.h.  Own implementation: host bookkeeping only.
#include <trajectory_planner/bsplineTraj.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <fstream>
#include <cstring>
#include <iostream>
#include <set>

#include "bsplineTrajBatch.h"

using std::cout;
using std::endl;

#ifndef VIGO_WITH_ROS
ros::Time ros::Time::now() {
    ros::Time t;
    t.sec = trajPlanner::wallSeconds();
    return t;
}
#endif

namespace trajPlanner {

std::atomic<double> g_prevPathLength{0.0};   // (bsplineTrajBatch.h)

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

// BT.cpp:187-195
void bsplineTraj::setMap(const std::shared_ptr<mapManager::occMap>& map) {
    link_.setMap(map);
    this->pathSearch_.reset(new AStar);
    const SearchGroup g(*this);
    this->pathSearch_->initGridMap(map, Eigen::Vector3i(g.pool[0], g.pool[1], g.pool[2]), this->minHeight_, this->maxHeight_);
}

void bsplineTraj::setMapRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) { link_.setRegion(boxMin, boxMax); }
void bsplineTraj::refreshMap() { link_.refresh(); }
void bsplineTraj::refreshMap(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) { link_.refresh(boxMin, boxMax); }
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
    return optData_.controlPoints.cols() == o.optData_.controlPoints.cols() && sameBatchKeyAnyCount(o);
}
// the batches of the solves and of the device rounds: with `mixed` (BatchOptions::mixedBatches) the count may differ inside
// a shape class of the kernels (7 .. 32 | 33 .. 64: the contract of the vigo_*_mixed entries)
bool bsplineTraj::sameSolveGroup(const bsplineTraj& o, bool mixed) const {
    const long na = optData_.controlPoints.cols(), nb = o.optData_.controlPoints.cols();
    if (na == nb || !mixed) return na == nb && sameBatchKeyAnyCount(o);
    if (na < 7 || nb < 7 || na > 64 || nb > 64 || (na <= 32) != (nb <= 32)) return false;
    return sameBatchKeyAnyCount(o);
}
bool bsplineTraj::sameBatchKeyAnyCount(const bsplineTraj& o) const {
    if (!link_.sameTarget(o.link_) || maxVel_ != o.maxVel_ || notCheckRatio_ != o.notCheckRatio_) return false;
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

// ---- the single-planner device seam ---------------------------------------------------

namespace {
// vigo_cost_grad of the one trajectory in hb; grad receives its 3 (N - 6) free scalars
bool costGrad(vigo_handle_t h, const HostBatch& hb, double& cost, double* grad) {
    struct Stage {
        Staged<double> cost, grad;
    };
    static thread_local Stage st;
    const size_t n = 3 * (size_t)(hb.N - 2 * bsplineDegree);
    DeviceBatch d;
    if (!uploadBatch(h, hb, d) || !st.cost.alloc(1) || !st.grad.alloc(n)) return false;
    if (vigo_cost_grad(h, 1, hb.N, d.ctrl, d.goff, d.gpv, d.gunk, d.ooff, d.obs, 0, d.weights, st.cost.get(), st.grad.get(), nullptr) != VIGO_OK)
        return false;
    return vigo_host::threadSync() && st.cost.download(&cost, 1) && st.grad.download(grad, n);
}
}  // namespace

// BT.cpp:687-718
int bsplineTraj::optimize() {
    std::vector<bsplineTraj*> one{this};
    BatchStats stats;
    solveBatch(one, BatchOptions(), stats);     // (one planner: no option bears on its solve)
    reportBatchStats(stats, nullptr);
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
    std::copy(g.begin(), g.end(), gradient.data() + 3 * bsplineDegree);
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
    const BatchOptions o;                       // (one planner, the host-driven loop: no option bears on it)
    BatchStats stats;
    solveBatch(one, o, stats);
    const double t0 = wallSeconds();
    while (!r.done) {
        std::vector<uint8_t> col, dyn;
        gateBatch(one, col, dyn);
        reboundStep(r, col[0] != 0, dyn[0] != 0, wallSeconds() - t0 > 0.03);
        if (!r.done && r.needOptimize) solveBatch(one, o, stats);
    }
    reportBatchStats(stats, nullptr);
    return r.ok;
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
