// polyTrajOccMap.cpp — min-snap seed planner facade (see the header).  Behaviour follows polyTrajOccMap.cpp (PM below):
// :10-138 parameters, :152-250 setters, :252-423 planning loops, :434-571 sampling, checker and getters.  The solo
// makePlan is the reference loop on the host; makePlanBatch runs the same loop for many planners with the QPs and the
// collision checks on the device.
#include <trajectory_planner/polyTrajOccMap.h>

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <iostream>

#include "../../../include/vigo.h"
#include "devbuf.h"
#include "polyBatch.h"

using std::cout;
using std::endl;

namespace trajPlanner {

// PM.cpp:10-18
polyTrajOccMap::polyTrajOccMap(const ros::NodeHandle& nh) : nh_(nh) {
    this->initParam();
    this->registerPub();
    this->registerCallback();
    if (this->usePWL_) this->initPWLSolver();   // the PWL solver exists only when use_pwl_failsafe is set here
    this->setDefaultInit();
}

polyTrajOccMap::~polyTrajOccMap() {
    if (dev_) vigo_destroy(dev_);
}

// PM.cpp:20-138: the keys under poly_traj/ and their defaults
void polyTrajOccMap::initParam() {
    if (!nh_.getParam("poly_traj/polynomial_degree", polyDegree_)) polyDegree_ = 7;
    if (!nh_.getParam("poly_traj/differential_degree", diffDegree_)) diffDegree_ = 4;
    if (!nh_.getParam("poly_traj/continuity_degree", continuityDegree_)) continuityDegree_ = 4;
    if (!nh_.getParam("poly_traj/desired_velocity", desiredVel_)) desiredVel_ = 1.0;
    if (!nh_.getParam("poly_traj/desired_acceleration", desiredAcc_)) desiredAcc_ = 1.0;
    if (!nh_.getParam("poly_traj/initial_radius", initR_)) initR_ = 0.5;
    if (!nh_.getParam("poly_traj/timeout", timeout_)) timeout_ = 0.1;
    if (!nh_.getParam("poly_traj/corridor_res", corridorRes_)) corridorRes_ = 5.0;
    if (!nh_.getParam("poly_traj/shrinking_factor", fs_)) fs_ = 0.8;
    if (!nh_.getParam("poly_traj/soft_constraint", softConstraint_)) softConstraint_ = false;
    // PM.cpp:108-113: read, and never used (see solveOnHost)
    if (softConstraint_ && !nh_.getParam("poly_traj/constraint_radius", softConstraintRadius_)) softConstraintRadius_ = 0.5;
    if (!nh_.getParam("poly_traj/sample_delta_time", delT_)) delT_ = 0.1;
    if (!nh_.getParam("poly_traj/maximum_iteration_num", maxIter_)) maxIter_ = 20;
    if (!nh_.getParam("poly_traj/use_pwl_failsafe", usePWL_)) usePWL_ = false;
}

void polyTrajOccMap::setMap(const std::shared_ptr<mapManager::occMap>& map) {
    map_ = map;
    mapStamp_ = 0;
}

void polyTrajOccMap::setMapRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) {
    mapRegion_.set = true;
    mapRegion_.boxMin = boxMin;
    mapRegion_.boxMax = boxMax;
    mapStamp_ = 0;
}

void polyTrajOccMap::refreshMap() {
    mapAdapter::bumpGeneration(map_.get());
    mapStamp_ = 0;
}

// see bsplineTraj::setDevice
void polyTrajOccMap::setDevice(int ordinal) {
    if (ordinal == deviceOrdinal_) return;
    if (dev_) { vigo_destroy(dev_); dev_ = nullptr; }
    mapStamp_ = 0;
    deviceOrdinal_ = ordinal;
}

bool polyTrajOccMap::syncDevice() {
    if (!map_) return false;
    if (hipSetDevice(deviceOrdinal_) != hipSuccess) return false;
    if (!dev_ && vigo_create(&dev_, deviceOrdinal_) != VIGO_OK) {
        dev_ = nullptr;
        return false;
    }
    if (vigo_set_stream(dev_, vigo_host::threadStream()) != VIGO_OK) return false;
    return mapAdapter::uploadSnapshot(dev_, map_, mapRegion_, mapStamp_);
}

void polyTrajOccMap::initSolver() {   // PM.cpp:152-154
    trajSolver_.reset(new polyTrajSolver(polyDegree_, diffDegree_, continuityDegree_, desiredVel_));
}

void polyTrajOccMap::initPWLSolver() { pwlTrajSolver_.reset(new pwlTraj(nh_)); }

void polyTrajOccMap::updateDesiredVel(double desiredVel) { desiredVel_ = desiredVel; }

// PM.cpp:164-166: the reference assigns the member to itself — the argument has no effect (kept, not fixed)
void polyTrajOccMap::updateDesiredAcc(double desiredAcc) {
    (void)desiredAcc;
    const double self = desiredAcc_;   // this->desiredAcc_ = desiredAcc_;
    desiredAcc_ = self;
}

void polyTrajOccMap::updatePath(const nav_msgs::Path& path) {
    std::vector<pose> trajPath;
    for (const auto& p : path.poses) trajPath.push_back(pose(p.pose.position.x, p.pose.position.y, p.pose.position.z));
    this->updatePath(trajPath);
}

// PM.cpp:177-187: startEndCondition = start vel, end vel, start acc, end acc
void polyTrajOccMap::updatePath(const nav_msgs::Path& path, const std::vector<Eigen::Vector3d>& startEndCondition) {
    this->updatePath(path);
    const Eigen::Vector3d startVel = startEndCondition[0], endVel = startEndCondition[1];
    const Eigen::Vector3d startAcc = startEndCondition[2], endAcc = startEndCondition[3];
    this->updateInitVel(startVel(0), startVel(1), startVel(2));
    this->updateEndVel(endVel(0), endVel(1), endVel(2));
    this->updateInitAcc(startAcc(0), startAcc(1), startAcc(2));
    this->updateEndAcc(endAcc(0), endAcc(1), endAcc(2));
}

void polyTrajOccMap::updatePath(const std::vector<pose>& path) { path_ = path; }

static geometry_msgs::Twist twist(double x, double y, double z) {
    geometry_msgs::Twist v;
    v.linear.x = x; v.linear.y = y; v.linear.z = z;
    return v;
}
void polyTrajOccMap::updateInitVel(double vx, double vy, double vz) { updateInitVel(twist(vx, vy, vz)); }
void polyTrajOccMap::updateInitVel(const geometry_msgs::Twist& v) { initVel_ = v; }
void polyTrajOccMap::updateEndVel(double vx, double vy, double vz) { updateEndVel(twist(vx, vy, vz)); }
void polyTrajOccMap::updateEndVel(const geometry_msgs::Twist& v) { endVel_ = v; }
void polyTrajOccMap::updateInitAcc(double ax, double ay, double az) { updateInitAcc(twist(ax, ay, az)); }
void polyTrajOccMap::updateInitAcc(const geometry_msgs::Twist& a) { initAcc_ = a; }
void polyTrajOccMap::updateEndAcc(double ax, double ay, double az) { updateEndAcc(twist(ax, ay, az)); }
void polyTrajOccMap::updateEndAcc(const geometry_msgs::Twist& a) { endAcc_ = a; }
void polyTrajOccMap::setDefaultInit() {
    updateInitVel(0, 0, 0);
    updateEndVel(0, 0, 0);
    updateInitAcc(0, 0, 0);
    updateEndAcc(0, 0, 0);
}

// ---- the planning loop of PM.cpp:326-399 in steps: begin, per round the QP (solveOnHost or the device QP), the samples
// and their check, advance(); finish.  makePlan and makePlanBatch keep their own time limits ----
struct polyTrajOccMap::PlanState {
    std::vector<double> corridor;   // corridorSizeVec
    int iters = 0;                  // countIter
    double t0 = 0;
};

// PM.cpp:334-346: a fresh solver for every plan (initSolver), the path and the four conditions, initial_radius everywhere
polyTrajOccMap::PlanState polyTrajOccMap::begin() {
    initSolver();
    trajSolver_->updatePath(path_);
    trajSolver_->updateInitVel(initVel_.linear.x, initVel_.linear.y, initVel_.linear.z);
    trajSolver_->updateEndVel(endVel_.linear.x, endVel_.linear.y, endVel_.linear.z);
    trajSolver_->updateInitAcc(initAcc_.linear.x, initAcc_.linear.y, initAcc_.linear.z);
    trajSolver_->updateEndAcc(endAcc_.linear.x, endAcc_.linear.y, endAcc_.linear.z);
    PlanState s;
    s.corridor.assign(path_.size() - 1, initR_);
    s.t0 = vigo_host::nowSec();
    findValidTraj_ = false;
    lastIterations_ = 0;
    return s;
}

// PM.cpp:355-360 (corridors) and :374 (none).  An infeasible corridor keeps the previous polynomial, like the reference.
void polyTrajOccMap::solveOnHost(bool corridorConstraint, PlanState& s) {
    if (corridorConstraint) {
        trajSolver_->setCorridorConstraint(s.corridor, corridorRes_);
        // PM.cpp:357-358: the bool is passed as the radius — x and y get 1.0 (or 0), z gets 0; constraint_radius is
        // never used (kept, not fixed)
        if (softConstraint_) trajSolver_->setSoftConstraint((double)softConstraint_, (double)softConstraint_, 0.0);
    }
    trajSolver_->solve();
}

// PM.cpp:363-371: shrink the colliding segments' corridors, count the solve; false once the loop ends (no collision, or
// countIter > maximum_iteration_num: up to maxIter_ + 1 solves)
bool polyTrajOccMap::advance(PlanState& s, bool collides, const std::set<int>& collisionSeg) {
    if (collides) this->adjustCorridorSize(collisionSeg, s.corridor);
    lastIterations_ = ++s.iters;
    return collides && s.iters <= maxIter_;
}

// PM.cpp:380-391: the verdict, the PWL fallback (with use_pwl_failsafe only), the visualisation message
void polyTrajOccMap::finish(std::vector<pose>& trajectory, bool valid) {
    findValidTraj_ = valid;
    if (!valid) {
        cout << "[minSnapTraj]: Not found. Return the best. Please consider piecewise linear trajectory!!" << endl;
        if (usePWL_ && pwlTrajSolver_) {
            pwlTrajSolver_->updatePath(path_);
            pwlTrajSolver_->makePlan(trajectory, delT_);
        }
    }
    trajMsgConverter(trajectory, trajVisMsg_);
}

// PM.cpp:252-255, :401-423: makePlan(trajectory) without the bool always plans with corridors (PM.cpp:257-324)
bool polyTrajOccMap::makePlan(bool corridorConstraint) {
    nav_msgs::Path dummyPath;
    return this->makePlan(dummyPath, corridorConstraint);
}

bool polyTrajOccMap::makePlan(std::vector<pose>& trajectory) { return this->makePlan(trajectory, true); }

bool polyTrajOccMap::makePlan(nav_msgs::Path& trajectory) { return this->makePlan(trajectory, true); }

bool polyTrajOccMap::makePlan(nav_msgs::Path& trajectory, bool corridorConstraint) {
    std::vector<pose> trajTemp;
    const bool valid = this->makePlan(trajTemp, corridorConstraint);
    this->trajMsgConverter(trajTemp, trajectory);
    return valid;
}

// PM.cpp:326-399, on the host: host QP, host sampling, the map's own isInflatedOccupied / isUnknown per sample
bool polyTrajOccMap::makePlan(std::vector<pose>& trajectory, bool corridorConstraint) {
    findValidTraj_ = false;
    lastIterations_ = 0;
    if (path_.size() == 1) {   // PM.cpp:328-332
        trajectory = path_;
        findValidTraj_ = true;
        return true;
    }
    if (path_.empty()) return false;
    PlanState s = begin();
    bool valid = false;
    while (ros::ok() && !valid) {
        if (vigo_host::nowSec() - s.t0 >= timeout_) {   // PM.cpp:349-353: tested at the top of each round
            cout << "[minSnapTraj]: Timeout!" << endl;
            break;
        }
        solveOnHost(corridorConstraint, s);
        // no polynomial to sample (the very first QP failed: coincident waypoints, an infeasible first corridor)
        if (!trajSolver_->hasSolution()) break;
        trajSolver_->getTrajectory(trajectory, delT_);
        if (!corridorConstraint) {   // PM.cpp:373-377: one solve, declared valid without any check
            lastIterations_ = ++s.iters;
            valid = true;
            break;
        }
        std::set<int> collisionSeg;
        valid = !this->checkCollisionTraj(trajectory, delT_, collisionSeg);
        if (!advance(s, !valid, collisionSeg)) break;
    }
    finish(trajectory, valid);
    return valid;
}

// PM.cpp:524-546: a sample collides when the map says inflated-occupied AND unknown (a reference quirk, SURVEY Appendix B,
// kept); the blame is collisionSegments' (polyBatch.h)
bool polyTrajOccMap::checkCollisionTraj(const std::vector<pose>& trajectory, double delT, std::set<int>& collisionSeg) {
    collisionSeg.clear();
    if (!trajSolver_) return false;
    std::vector<uint8_t> flags;
    for (const pose& p : trajectory) {
        const Eigen::Vector3d pEig(p.x, p.y, p.z);
        flags.push_back(map_ && map_->isInflatedOccupied(pEig) && map_->isUnknown(pEig));
    }
    return vigo_host::collisionSegments(flags.data(), flags.size(), trajSolver_->getTimeKnot(), delT, collisionSeg);
}

// PM.cpp:548-552
void polyTrajOccMap::adjustCorridorSize(const std::set<int>& collisionSeg, std::vector<double>& corridorSizeVec) {
    for (int collisionIdx : collisionSeg) corridorSizeVec[collisionIdx] = corridorSizeVec[collisionIdx] * fs_;
}

// makePlan(trajectory, corridorConstraint) of many planners in lock-step.  Per round: the time limit of every active
// planner (timeout x planners in the batch, as polyTrajOctomap's batch), then its QP — ONE vigo_minsnap launch per
// (waypoint count, differential / continuity degree, velocity, corridor_res) group; soft constraints (which the device QP
// does not take), shapes vigo_minsnap_supported refuses and device statuses other than "solved" go to the host QP, which
// decides them as the solo plan does — then ONE vigo_traj_point_check launch over every candidate (a trajectory it
// rejects is sampled and checked on the host that round).  Planners the batch cannot take (fewer than two waypoints,
// another polynomial degree than 7, another map, region or device than the first) plan alone; so does every planner when
// the device cannot be reached.  A device failure during the batch ends it: the planners not yet valid fall back.
std::vector<bool> polyTrajOccMap::makePlanBatch(const std::vector<polyTrajOccMap*>& ps, bool corridorConstraint,
                                                std::vector<std::vector<pose>>* trajectories) {
    const size_t P = ps.size();
    std::vector<bool> result(P, false);
    std::vector<std::vector<pose>> local;
    std::vector<std::vector<pose>>& out = trajectories ? *trajectories : local;
    out.assign(P, {});
    polyTrajOccMap* lead = nullptr;
    std::vector<size_t> grp;
    for (size_t i = 0; i < P; ++i) {
        polyTrajOccMap* p = ps[i];
        if (!lead && p->path_.size() >= 2 && p->polyDegree_ == 7 && p->map_) lead = p;
        const bool batchable = lead && p->path_.size() >= 2 && p->polyDegree_ == 7 && p->map_ == lead->map_ &&
                               sameRegion(p->mapRegion_, lead->mapRegion_) && p->deviceOrdinal_ == lead->deviceOrdinal_;
        if (batchable) {
            grp.push_back(i);
        } else {
            result[i] = p->makePlan(out[i], corridorConstraint);
        }
    }
    if (grp.empty()) return result;
    if (!lead->syncDevice()) {
        cout << "[minSnapTraj]: no device for the batch; the planners plan alone." << endl;
        for (size_t i : grp) result[i] = ps[i]->makePlan(out[i], corridorConstraint);
        return result;
    }
    const size_t G = grp.size();
    std::vector<PlanState> st;
    std::vector<bool> active(G, true), valid(G, false);
    for (size_t g = 0; g < G; ++g) st.push_back(ps[grp[g]]->begin());
    bool ok = true;
    while (ok) {
        std::vector<size_t> act;
        for (size_t g = 0; g < G; ++g) {
            if (!active[g]) continue;
            polyTrajOccMap* p = ps[grp[g]];
            if (vigo_host::nowSec() - st[g].t0 >= p->timeout_ * (double)G) {   // PM.cpp:349-353
                cout << "[minSnapTraj]: Timeout!" << endl;
                active[g] = false;
                continue;
            }
            act.push_back(g);
        }
        if (act.empty()) break;
        // ---- the QPs ----
        std::vector<bool> solved(G, false);
        for (size_t a0 = 0; a0 < act.size() && ok; ++a0) {
            const size_t g0 = act[a0];
            if (solved[g0]) continue;
            solved[g0] = true;
            polyTrajOccMap* p0 = ps[grp[g0]];
            const int W = (int)p0->path_.size();
            if (p0->softConstraint_ || !vigo_minsnap_supported(W, 7, p0->diffDegree_, p0->continuityDegree_)) {
                p0->solveOnHost(corridorConstraint, st[g0]);
                continue;
            }
            std::vector<size_t> members{g0};
            for (size_t a = a0 + 1; a < act.size(); ++a) {
                const size_t g = act[a];
                const polyTrajOccMap* p = ps[grp[g]];
                if (!solved[g] && !p->softConstraint_ && (int)p->path_.size() == W && p->diffDegree_ == p0->diffDegree_ &&
                    p->continuityDegree_ == p0->continuityDegree_ && p->desiredVel_ == p0->desiredVel_ &&
                    p->corridorRes_ == p0->corridorRes_) {
                    members.push_back(g);
                    solved[g] = true;
                }
            }
            std::vector<vigo_host::QpMember> qp;
            for (size_t g : members) {
                const polyTrajOccMap* p = ps[grp[g]];
                qp.push_back({&p->path_, corridorConstraint ? &st[g].corridor : nullptr, {&p->initVel_, &p->endVel_, &p->initAcc_, &p->endAcc_}, 0, {}});
            }
            ok = vigo_host::minsnapGroupOnDevice(lead->dev_, p0->diffDegree_, p0->continuityDegree_, p0->desiredVel_, p0->corridorRes_, qp);
            for (size_t a = 0; ok && a < members.size(); ++a) {
                const size_t g = members[a];
                polyTrajOccMap* p = ps[grp[g]];
                if (qp[a].status == 0) {
                    if (corridorConstraint) p->trajSolver_->setCorridorConstraint(st[g].corridor, p->corridorRes_);
                    p->trajSolver_->installSolution(qp[a].sol[0], qp[a].sol[1], qp[a].sol[2]);
                } else {
                    p->solveOnHost(corridorConstraint, st[g]);   // -1 numerical, -2 infeasible: the host QP decides
                }
            }
        }
        if (!ok) break;
        // ---- without corridors: one solve, valid without any check (PM.cpp:373-377) ----
        std::vector<vigo_host::TrajCheck> cand;
        for (size_t g : act) {
            polyTrajOccMap* p = ps[grp[g]];
            active[g] = corridorConstraint;
            if (!p->trajSolver_->hasSolution()) {   // nothing to sample (see makePlan): not found
                active[g] = false;
                continue;
            }
            if (!corridorConstraint) {
                p->lastIterations_ = ++st[g].iters;
                valid[g] = true;
                continue;
            }
            cand.push_back({g, p->trajSolver_.get(), p->delT_, p->path_.back(), 0, false, {}});
        }
        // ---- every candidate checked whole by ONE vigo_traj_point_check launch; verdicts and segment masks come back ----
        ok = vigo_host::checkTrajectoriesOnDevice(cand, [&](int T, int S, const int32_t* segOff, const double* co, const double* kn,
                                                            const double* dt, const double* ep, int32_t* status, int32_t* n,
                                                            uint8_t* flag, int32_t* first, uint8_t* seg) {
            return vigo_traj_point_check(lead->dev_, T, S, 7, segOff, co, kn, dt, ep, status, n, flag, first, nullptr, seg) == VIGO_OK;
        });
        if (!ok) cout << "[minSnapTraj]: device trajectory check failed: " << vigo_last_error(lead->dev_) << endl;
        for (size_t a = 0; ok && a < cand.size(); ++a) {
            const size_t g = cand[a].who;
            polyTrajOccMap* p = ps[grp[g]];
            if (cand[a].status != VIGO_TRAJ_OK) {   // a trajectory the device entry rejects: sampled and checked on the host
                std::vector<pose> traj;
                p->trajSolver_->getTrajectory(traj, p->delT_);
                cand[a].collides = p->checkCollisionTraj(traj, p->delT_, cand[a].segments);   // (clears the segments first)
            }
            valid[g] = !cand[a].collides;
            active[g] = p->advance(st[g], cand[a].collides, cand[a].segments);
        }
    }
    // the returned trajectories: sampled once, from the last polynomial (the reference returns the last candidate when
    // none was valid), then the verdict and the fallback as in makePlan
    for (size_t g = 0; g < G; ++g) {
        polyTrajOccMap* p = ps[grp[g]];
        std::vector<pose>& traj = out[grp[g]];
        if (p->trajSolver_->hasSolution()) p->trajSolver_->getTrajectory(traj, p->delT_);
        p->finish(traj, valid[g]);
        result[grp[g]] = valid[g];
    }
    return result;
}

// PM.cpp:554-571
void polyTrajOccMap::trajMsgConverter(const std::vector<pose>& trajectoryTemp, nav_msgs::Path& trajectory) {
    vigo_host::posesToPathMsg(trajectoryTemp, trajectory);
}

// PM.cpp:434-446: the polynomial sampled every dt while t <= getDuration() (with use_pwl_failsafe and no valid
// polynomial the duration is the PWL's, the positions still the polynomial's — kept)
nav_msgs::Path polyTrajOccMap::getTrajectory(double dt) {
    nav_msgs::Path trajectory;
    trajectory.header.frame_id = "map";
    const double duration = this->getDuration();
    if (!(dt > 0.0)) return trajectory;   // (the reference's loop would not end)
    for (double t = 0; t <= duration; t += dt) {
        const Eigen::Vector3d pos = this->getPos(t);
        geometry_msgs::PoseStamped ps;
        ps.pose.position.x = pos(0);
        ps.pose.position.y = pos(1);
        ps.pose.position.z = pos(2);
        trajectory.poses.push_back(ps);
    }
    return trajectory;
}

// PM.cpp:448-482
geometry_msgs::PoseStamped polyTrajOccMap::getPose(double t) {
    if (t > this->getDuration()) t = this->getDuration();
    if (usePWL_ && !findValidTraj_ && pwlTrajSolver_) return pwlTrajSolver_->getPose(t);
    geometry_msgs::PoseStamped ps;
    ps.header.frame_id = "map";
    if (!trajSolver_) return ps;
    const pose p = trajSolver_->getPose(t);
    ps.pose.position.x = p.x;
    ps.pose.position.y = p.y;
    ps.pose.position.z = p.z;
    ps.pose.orientation = quaternion_from_rpy(0, 0, p.yaw);
    return ps;
}

// PM.cpp:484-506
Eigen::Vector3d polyTrajOccMap::getPos(double t) {
    if (t > this->getDuration()) t = this->getDuration();
    return trajSolver_ ? trajSolver_->getPos(t) : Eigen::Vector3d(0, 0, 0);
}

Eigen::Vector3d polyTrajOccMap::getVel(double t) {
    if (t > this->getDuration()) t = this->getDuration();
    return trajSolver_ ? trajSolver_->getVel(t) : Eigen::Vector3d(0, 0, 0);
}

Eigen::Vector3d polyTrajOccMap::getAcc(double t) {
    if (t > this->getDuration()) t = this->getDuration();
    return trajSolver_ ? trajSolver_->getAcc(t) : Eigen::Vector3d(0, 0, 0);
}

// PM.cpp:508-522: a one-waypoint path has no duration; with use_pwl_failsafe and no valid polynomial, the PWL's last knot
double polyTrajOccMap::getDuration() {
    if (path_.size() == 1) return 0.0;
    if (usePWL_ && !findValidTraj_) {
        if (!pwlTrajSolver_) return 0.0;
        const std::vector<double> k = pwlTrajSolver_->getTimeKnot();
        return k.empty() ? 0.0 : k.back();
    }
    if (!trajSolver_) return 0.0;
    const std::vector<double>& k = trajSolver_->getTimeKnot();
    return k.empty() ? 0.0 : k.back();
}

}  // namespace trajPlanner
