// polyTrajOccMap.cpp — min-snap seed planner facade (see the header).  Behaviour follows polyTrajOccMap.cpp (PM below):
// :10-138 parameters, :152-250 setters, :252-423 planning loops, :434-571 sampling, checker and getters.  The solo
// makePlan is the reference loop on the host; makePlanBatch runs the same loop for many planners with the QPs and the
// collision checks on the device.
#include <trajectory_planner/polyTrajOccMap.h>

#include <cmath>
#include <iostream>

#include "../../../include/vigo.h"
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

polyTrajOccMap::~polyTrajOccMap() {}

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

// the device link (mapAdapter.h); this planner prints nothing about it, and does not sync without a map
void polyTrajOccMap::setMap(const std::shared_ptr<mapManager::occMap>& map) { link_.setMap(map); }
void polyTrajOccMap::setMapRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) { link_.setRegion(boxMin, boxMax); }
void polyTrajOccMap::refreshMap() { link_.refresh(); }
void polyTrajOccMap::refreshMap(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) { link_.refresh(boxMin, boxMax); }
void polyTrajOccMap::setDevice(int ordinal) { link_.setDevice(ordinal); }
bool polyTrajOccMap::syncDevice() { return link_.sync(true) == DeviceLink::kSynced; }

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
// PM.cpp:334-346: a fresh solver for every plan (initSolver), the path and the four conditions, initial_radius everywhere
polyTrajOccMap::PlanState polyTrajOccMap::begin(bool corridorConstraint) {
    initSolver();
    trajSolver_->updatePath(path_);
    trajSolver_->updateInitVel(initVel_.linear.x, initVel_.linear.y, initVel_.linear.z);
    trajSolver_->updateEndVel(endVel_.linear.x, endVel_.linear.y, endVel_.linear.z);
    trajSolver_->updateInitAcc(initAcc_.linear.x, initAcc_.linear.y, initAcc_.linear.z);
    trajSolver_->updateEndAcc(endAcc_.linear.x, endAcc_.linear.y, endAcc_.linear.z);
    PlanState s;
    s.corridors = corridorConstraint;
    s.corridor.assign(path_.size() - 1, initR_);
    s.t0 = vigo_host::nowSec();
    findValidTraj_ = false;
    lastIterations_ = 0;
    return s;
}

// PM.cpp:355-360 (corridors) and :374 (none).  An infeasible corridor keeps the previous polynomial, like the reference.
void polyTrajOccMap::solveOnHost(PlanState& s) {
    if (s.corridors) {
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
    PlanState s = begin(corridorConstraint);
    bool valid = false;
    while (ros::ok() && !valid) {
        if (vigo_host::nowSec() - s.t0 >= timeout_) {   // PM.cpp:349-353: tested at the top of each round
            cout << "[minSnapTraj]: Timeout!" << endl;
            break;
        }
        solveOnHost(s);
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
        flags.push_back(link_.map() && link_.map()->isInflatedOccupied(pEig) && link_.map()->isUnknown(pEig));
    }
    return vigo_host::collisionSegments(flags.data(), flags.size(), trajSolver_->getTimeKnot(), delT, collisionSeg);
}

// PM.cpp:548-552
void polyTrajOccMap::adjustCorridorSize(const std::set<int>& collisionSeg, std::vector<double>& corridorSizeVec) {
    for (int collisionIdx : collisionSeg) corridorSizeVec[collisionIdx] = corridorSizeVec[collisionIdx] * fs_;
}

// makePlan(trajectory, corridorConstraint) of many planners in lock-step: LockStepBatch (polyBatchLoop.h) with the rules
// below and the device steps — ONE vigo_minsnap launch per QP group, ONE vigo_traj_point_check launch over every candidate
// of a round.  A device failure during the batch ends it: the planners not yet valid end as "not found".
struct polyTrajOccMap::DeviceSteps {
    polyTrajOccMap* lead = nullptr;
    bool ready(polyTrajOccMap* l) { lead = l; return l->syncDevice(); }
    bool supported(int W, int diff, int cont) const { return vigo_minsnap_supported(W, 7, diff, cont) != 0; }
    bool solve(int diff, int cont, double vel, double corridorRes, std::vector<vigo_host::QpMember>& qp) {
        return vigo_host::minsnapGroupOnDevice(lead->link_.handle(), diff, cont, vel, corridorRes, qp);
    }
    bool check(std::vector<vigo_host::TrajCheck>& cand) {
        vigo_context* dev = lead->link_.handle();
        return vigo_host::checkTrajectoriesOnDevice(cand, [dev](int T, int S, const int32_t* segOff, const double* co, const double* kn,
                                                                const double* dt, const double* ep, int32_t* status, int32_t* n,
                                                                uint8_t* flag, int32_t* first, uint8_t* seg) {
            return vigo_traj_point_check(dev, T, S, 7, segOff, co, kn, dt, ep, status, n, flag, first, nullptr, seg) == VIGO_OK;
        });
    }
    const char* lastError() const { return vigo_last_error(lead->link_.handle()); }
};

std::vector<bool> polyTrajOccMap::makePlanBatch(const std::vector<polyTrajOccMap*>& ps, bool corridorConstraint,
                                                std::vector<std::vector<pose>>* trajectories) {
    std::vector<std::vector<pose>> local;
    DeviceSteps steps;
    return vigo_host::LockStepBatch<polyTrajOccMap>::run(ps, corridorConstraint, trajectories ? *trajectories : local, steps);
}

// Who is batchable and who leads: the first planner with two or more waypoints, degree 7 and a map leads; the batch takes
// those like it on the same device, map and box.  The others plan alone.
const polyTrajOccMap* polyTrajOccMap::batchReference(const std::vector<polyTrajOccMap*>& ps) {
    for (const polyTrajOccMap* p : ps)
        if (p->path_.size() >= 2 && p->polyDegree_ == 7 && p->link_.map()) return p;
    return nullptr;
}
bool polyTrajOccMap::batchable(const polyTrajOccMap* ref) const {
    return ref && path_.size() >= 2 && polyDegree_ == 7 && link_.sameTarget(ref->link_);
}
bool polyTrajOccMap::planAlone(std::vector<pose>& trajectory, bool corridorConstraint, bool&) { return makePlan(trajectory, corridorConstraint); }

// Without a device: one line, and every planner of the group plans alone.
void polyTrajOccMap::planWithoutDevice(const std::vector<polyTrajOccMap*>& ps, const std::vector<size_t>& grp, bool corridorConstraint,
                                       std::vector<std::vector<pose>>& out, std::vector<bool>& result) {
    cout << "[minSnapTraj]: no device for the batch; the planners plan alone." << endl;
    for (size_t i : grp) result[i] = ps[i]->makePlan(out[i], corridorConstraint);
}

// The time limit, timeout x (planners in the batch), is tested at the top of each round (PM.cpp:349-353).
bool polyTrajOccMap::timedOutBeforeRound(const PlanState& s, size_t G) const {
    if (vigo_host::nowSec() - s.t0 < timeout_ * (double)G) return false;
    cout << "[minSnapTraj]: Timeout!" << endl;
    return true;
}

// The QP group key beside the waypoint count: differential and continuity degree, velocity, corridor_res, and no soft
// constraint — the device QP takes the waypoints as equalities, so a planner with one goes straight to the host QP
// (hostQpOnly), as do the shapes vigo_minsnap_supported refuses.
bool polyTrajOccMap::sameQpGroup(const PlanState&, const polyTrajOccMap& o, const PlanState&) const {
    return !o.softConstraint_ && o.diffDegree_ == diffDegree_ && o.continuityDegree_ == continuityDegree_ && o.desiredVel_ == desiredVel_ &&
           o.corridorRes_ == corridorRes_;
}

// The conditions handed to the QP: the four twists.
vigo_host::QpMember polyTrajOccMap::qpMember(size_t who, const PlanState& s) const {
    return {who, &path_, s.corridors ? &s.corridor : nullptr, {&initVel_, &endVel_, &initAcc_, &endAcc_}, 0, {}};
}

// A solved QP is installed (with the corridor boxes the host solve would have set); any other status (-1 numerical, -2
// infeasible) goes to the host QP, which decides it as the solo plan does.
void polyTrajOccMap::takeQpResult(PlanState& s, const vigo_host::QpMember& m) {
    if (m.status == 0) {
        if (s.corridors) trajSolver_->setCorridorConstraint(s.corridor, corridorRes_);
        trajSolver_->installSolution(m.sol[0], m.sol[1], m.sol[2]);
    } else {
        solveOnHost(s);
    }
}

// The no-corridor round (PM.cpp:373-377): one solve, valid without any check.
bool polyTrajOccMap::validWithoutCheck(PlanState& s) {
    if (s.corridors) return false;
    lastIterations_ = ++s.iters;
    return true;
}

// A candidate the device check rejects is sampled and checked on the host that round, by the solo plan's rule.
void polyTrajOccMap::checkOnHost(polyTrajOccMap&, vigo_host::TrajCheck& c) {
    std::vector<pose> traj;
    trajSolver_->getTrajectory(traj, delT_);
    c.collides = checkCollisionTraj(traj, delT_, c.segments);   // (clears the segments first)
}

// The ending: the last polynomial sampled (the reference returns the last candidate when none was valid), then the verdict
// and the fallback as in makePlan.
bool polyTrajOccMap::finishBatch(std::vector<pose>& trajectory, bool valid) {
    if (trajSolver_->hasSolution()) trajSolver_->getTrajectory(trajectory, delT_);
    finish(trajectory, valid);
    return valid;
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
