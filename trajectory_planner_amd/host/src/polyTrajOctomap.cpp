// polyTrajOctomap.cpp — min-snap + corridor planner facade (see the header).  Behaviour follows
// polyTrajOctomap.cpp:14-110 (parameters), :178-192, :226-545 (planning loops), :547-689 (checker,
// getters); the box sweep of every trajectory sample runs on the device.
#include <trajectory_planner/polyTrajOctomap.h>

#include <cmath>
#include <iostream>

#include "../../../include/vigo.h"
#include "devbuf.h"
#include "polyBatch.h"

using std::cout;
using std::endl;

namespace trajPlanner {

polyTrajOctomap::polyTrajOctomap() : polyTrajOctomap(ros::NodeHandle()) {}

polyTrajOctomap::polyTrajOctomap(const ros::NodeHandle& nh) : nh_(nh) {
    // PO.cpp:14-108: same (un-namespaced) keys and fall-back values
    if (!nh_.getParam("collision_box", collisionBox_) || collisionBox_.size() < 3) collisionBox_ = {0.5, 0.5, 0.5};
    if (!nh_.getParam("polynomial_degree", polyDegree_)) polyDegree_ = 7;
    if (!nh_.getParam("differential_degree", diffDegree_)) diffDegree_ = 4;
    if (!nh_.getParam("continuity_degree", continuityDegree_)) continuityDegree_ = 4;
    if (!nh_.getParam("desired_velocity", desiredVel_)) desiredVel_ = 1.0;
    if (!nh_.getParam("map_resolution", mapRes_)) mapRes_ = 0.2;
    if (!nh_.getParam("maximum_iteration_num", maxIter_)) maxIter_ = 20;
    if (!nh_.getParam("traj_timeout", timeout_)) timeout_ = 0.1;
    if (!nh_.getParam("mode", mode_)) mode_ = true;
    if (!nh_.getParam("sample_delta_time", delT_)) delT_ = 0.1;
    if (!nh_.getParam("initial_radius", initR_)) initR_ = 0.5;
    if (!nh_.getParam("shrinking_factor", fs_)) fs_ = 0.8;
    if (!nh_.getParam("corridor_res", corridorRes_)) corridorRes_ = 5.0;
    if (!nh_.getParam("soft_constraint", softConstraint_)) softConstraint_ = false;                       // PO.cpp:98-107
    if (softConstraint_ && !nh_.getParam("constraint_radius", softConstraintRadius_)) softConstraintRadius_ = 0.5;
}

void polyTrajOctomap::setMap(const std::shared_ptr<mapManager::occMap>& map) { link_.setMap(map); }
void polyTrajOctomap::setDevice(int ordinal) { link_.setDevice(ordinal); }

// the device link's sync (mapAdapter.h) with this planner's console lines; it does not sync without a map
bool polyTrajOctomap::syncDevice() {
    const DeviceLink::Sync r = link_.sync(true);
    if (r == DeviceLink::kNoDevice)
        cout << "[Trajectory Planner INFO]: HIP device " << link_.ordinal() << " is not available (no CPU fallback)." << endl;
    if (r == DeviceLink::kNoHandle) cout << "[Trajectory Planner INFO]: no HIP device for the corridor checker (no CPU fallback)." << endl;
    return r == DeviceLink::kSynced;
}

void polyTrajOctomap::updatePath(const nav_msgs::Path& path) {
    std::vector<pose> trajPath;
    for (const auto& p : path.poses) trajPath.push_back(pose(p.pose.position.x, p.pose.position.y, p.pose.position.z));
    this->updatePath(trajPath);
}

void polyTrajOctomap::updatePath(const std::vector<pose>& path) { this->path_ = path; extKnots_.clear(); }
void polyTrajOctomap::updateInitVel(double vx, double vy, double vz) { initVel_[0] = vx; initVel_[1] = vy; initVel_[2] = vz; }
void polyTrajOctomap::updateInitAcc(double ax, double ay, double az) { initAcc_[0] = ax; initAcc_[1] = ay; initAcc_[2] = az; }
void polyTrajOctomap::setDefaultInit() { updateInitVel(0, 0, 0); updateInitAcc(0, 0, 0); }

void polyTrajOctomap::setSolution(int polyDegree, const std::vector<double>& xSol, const std::vector<double>& ySol,
                                  const std::vector<double>& zSol, const std::vector<double>& timeKnot) {
    extDegree_ = polyDegree;
    xSol_ = xSol; ySol_ = ySol; zSol_ = zSol;
    extKnots_ = timeKnot;
    trajSolver_.reset();
}

// PO.cpp:178-186
void polyTrajOctomap::insertWaypoint(const std::set<int>& seg) {
    for (auto rit = seg.rbegin(); rit != seg.rend(); ++rit) {
        const int idx = *rit;
        if (idx < 0 || idx + 1 >= (int)path_.size()) continue;
        const pose p1 = path_[idx], p2 = path_[idx + 1];
        path_.insert(path_.begin() + idx + 1, pose((p1.x + p2.x) / 2, (p1.y + p2.y) / 2, (p1.z + p2.z) / 2));
    }
}

const std::vector<double>& polyTrajOctomap::timeKnots() {
    if (trajSolver_) return trajSolver_->getTimeKnot();
    if (!extKnots_.empty()) return extKnots_;
    return pwlKnots_;
}

bool polyTrajOctomap::sweepPoints(const std::vector<pose>& pts, std::vector<uint8_t>& flags) {
    flags.assign(pts.size(), 1);
    if (pts.empty()) return true;
    if (!syncDevice()) return false;
    std::vector<double> xyz;
    vigo_host::appendXyz(pts, xyz);
    const bool ok = sweepXyz(xyz, flags);
    if (!ok) cout << "[Trajectory Planner INFO]: device box sweep failed: " << vigo_last_error(link_.handle()) << endl;
    return ok;
}

// ONE vigo_box_collision_points launch over xyz triples on the synced handle: flags[i] = 1 where the collision box at
// sample i meets an occupied voxel (all 1 if the launch or a copy fails)
bool polyTrajOctomap::sweepXyz(const std::vector<double>& xyz, std::vector<uint8_t>& flags) {
    const size_t n = xyz.size() / 3;
    flags.assign(n, 1);
    if (n == 0) return true;
    struct Stage {
        vigo_host::Staged<double> xyz;
        vigo_host::Staged<uint8_t> flags;
    };
    static thread_local Stage st;      // reused by every sweep of this thread
    const double box[3] = {collisionBox_[0], collisionBox_[1], collisionBox_[2]};
    const bool ok = st.xyz.upload(xyz) && st.flags.alloc(flags.size()) &&
                    vigo_box_collision_points(link_.handle(), (int64_t)n, st.xyz.get(), box, mapRes_, st.flags.get()) == VIGO_OK &&
                    st.flags.download(flags);
    // A pose at NaN or infinity: the reference's sweep makes no pass there (the lattice count is the conversion of a
    // NaN, INT_MIN on x86 — the device entry point follows that, include/vigo.h) and would publish the trajectory.  The
    // facade refuses such a pose instead: a degenerate min-snap solution (coincident waypoints) then falls back to the
    // piecewise-linear plan like any colliding one.
    for (size_t i = 0; i < n; ++i)
        if (!(std::isfinite(xyz[3 * i]) && std::isfinite(xyz[3 * i + 1]) && std::isfinite(xyz[3 * i + 2]))) flags[i] = 1;
    return ok;
}

bool polyTrajOctomap::checkCollision(const pose& p) {
    std::vector<uint8_t> f;
    sweepPoints({p}, f);
    return f[0] != 0;
}

// PO.cpp:571-589 on the dense map (host: a single lookup)
bool polyTrajOctomap::checkCollisionPoint(const pose& p, bool ignoreUnknown) {
    if (!link_.map()) return true;
    const unsigned v = mapAdapter::nodeBits(link_.map(), link_.region(), (float)p.x, (float)p.y, (float)p.z);   // pose2Octomap + search()
    if (v & mapAdapter::kOutside) return true;                  // beyond getMetricMin/Max
    if (v & mapAdapter::kUnknown) return !ignoreUnknown;        // no node there
    return (v & mapAdapter::kOccupied) != 0;                    // isNodeOccupied
}

// PO.cpp:619-632
bool polyTrajOctomap::checkCollisionTraj(const std::vector<pose>& trajectory, std::vector<int>& collisionIdx) {
    std::vector<uint8_t> f;
    sweepPoints(trajectory, f);
    bool has = false;
    for (size_t i = 0; i < f.size(); ++i)
        if (f[i]) { has = true; collisionIdx.push_back((int)i); }
    return has;
}

// PO.cpp:634-656
bool polyTrajOctomap::checkCollisionTraj(const std::vector<pose>& trajectory, double delT, std::set<int>& collisionSeg) {
    collisionSeg.clear();
    std::vector<uint8_t> f;
    sweepPoints(trajectory, f);
    return vigo_host::collisionSegments(f.data(), f.size(), timeKnots(), delT, collisionSeg);
}

// ---- the fallback of PO.cpp:308-318, :373-383, :528-541: a fresh pwlTraj over the waypoints (its own 1.0 m/s and
// 0.5 rad/s, piecewiseLinearTraj.h:20-21 — not the planner's desired velocity), sampled at delT; it replaces the
// min-snap polynomial as the plan ----
void polyTrajOctomap::pwlPlan(std::vector<pose>& trajectory, double delT) {
    trajSolver_.reset();
    pwlTrajSolver_.reset(new pwlTraj(nh_));
    trajectory.clear();
    pwlKnots_.clear();
    if (path_.empty()) return;
    pwlTrajSolver_->updatePath(path_);
    pwlTrajSolver_->makePlan(trajectory, delT);
    pwlKnots_ = pwlTrajSolver_->getTimeKnot();
}

// ---- the planning loop of PO.cpp:259-545: per round the QP (solveOnHost, or the device QP in makePlanBatch), the
// samples at delT, their box sweep, then advance(); the two callers keep their own time limits ----
polyTrajOctomap::PlanState polyTrajOctomap::begin(bool addingWaypoints) {
    setDefaultInit();
    trajSolver_.reset(new polyTrajSolver(polyDegree_, diffDegree_, continuityDegree_, desiredVel_));
    trajSolver_->updatePath(path_);
    trajSolver_->updateInitVel(initVel_[0], initVel_[1], initVel_[2]);
    trajSolver_->updateInitAcc(initAcc_[0], initAcc_[1], initAcc_[2]);
    PlanState s;
    s.addingWaypoints = addingWaypoints;
    if (!addingWaypoints) s.corridor.assign(path_.size() - 1, initR_);
    s.t0 = vigo_host::nowSec();
    findValidTraj_ = false;
    lastIterations_ = 0;
    return s;
}

// the round's corridor boxes (PO.cpp:421-424), the soft waypoint boxes (PO.cpp:290-292, :354-356, :426-428), the QP.
// An infeasible corridor keeps the previous polynomial, like the reference.
void polyTrajOctomap::solveOnHost(PlanState& s) {
    if (!s.addingWaypoints) trajSolver_->setCorridorConstraint(s.corridor, corridorRes_);
    if (softConstraint_) trajSolver_->setSoftConstraint(softConstraintRadius_, softConstraintRadius_, 0);
    trajSolver_->solve();
}

// this round's verdict (checkCollisionTraj, PO.cpp:634-656: does any sample collide, which segments are to blame): no
// collision ends the loop with a valid trajectory; otherwise insert waypoints in the colliding segments (PO.cpp:178-186;
// the solver's path is refreshed, which the reference omits) or shrink their corridors (PO.cpp:188-192).  False once the
// planner stops: valid, or past the iteration limit.
bool polyTrajOctomap::advance(PlanState& s, bool collides, const std::set<int>& collisionSeg) {
    if (collides && s.addingWaypoints) {
        insertWaypoint(collisionSeg);
        trajSolver_->updatePath(path_);
    } else if (collides) {
        adjustCorridorSize(collisionSeg, s.corridor);
    }
    lastIterations_ = ++s.iters;
    findValidTraj_ = !collides;
    return collides && s.iters <= maxIter_;
}

// PO.cpp:371-383, :531-542
void polyTrajOctomap::finish(std::vector<pose>& trajectory, double delT) {
    if (findValidTraj_) {
        cout << "[Trajectory Planner INFO]: Found valid trajectory!" << endl;
    } else {
        cout << "[Trajectory Planner INFO]: Not found. Return the best. Please consider piecewise linear trajectory!!" << endl;
        pwlPlan(trajectory, delT);
    }
}

// advance() on per-sample sweep flags of a host-sampled trajectory (collisionSegments, PO.cpp:634-656)
bool polyTrajOctomap::advanceOnFlags(PlanState& s, const std::vector<uint8_t>& flags, double delT) {
    std::set<int> collisionSeg;
    const bool collides = vigo_host::collisionSegments(flags.data(), flags.size(), trajSolver_->getTimeKnot(), delT, collisionSeg);
    return advance(s, collides, collisionSeg);
}

// makePlanAddingWaypoint / makePlanCorridorConstraint: PO.cpp:323-386, :472-545
void polyTrajOctomap::planOnHost(bool addingWaypoints, std::vector<pose>& trajectory, double delT) {
    findValidTraj_ = false;
    if (path_.empty()) return;
    if (path_.size() == 1) { trajectory = path_; findValidTraj_ = true; return; }
    PlanState s = begin(addingWaypoints);
    std::vector<uint8_t> flags;
    do {
        if (vigo_host::nowSec() - s.t0 >= timeout_) { cout << "[Trajectory Planner INFO]: Timeout." << endl; break; }
        solveOnHost(s);
        // with no polynomial to keep (the very first corridor was infeasible, and shrinking it cannot help; a degenerate
        // path such as coincident waypoints) there is nothing to sample: not found
        if (!trajSolver_->hasSolution()) break;
        trajSolver_->getTrajectory(trajectory, delT);
        sweepPoints(trajectory, flags);   // a failed sweep leaves every flag set: the loop goes on
    } while (advanceOnFlags(s, flags, delT));
    finish(trajectory, delT);
}

void polyTrajOctomap::makePlanAddingWaypoint(std::vector<pose>& trajectory, double delT) { planOnHost(true, trajectory, delT); }
void polyTrajOctomap::makePlanCorridorConstraint(std::vector<pose>& trajectory, double delT) { planOnHost(false, trajectory, delT); }

void polyTrajOctomap::makePlan(std::vector<pose>& trajectory, double delT) {
    const bool installed = !extKnots_.empty() && !trajSolver_;
    if (!installed || path_.size() < 2) {
        if (mode_) makePlanAddingWaypoint(trajectory, delT);
        else makePlanCorridorConstraint(trajectory, delT);
        return;
    }
    // an installed polynomial: one pass of the loop body (sample -> device sweep); one whose coefficients do not fit
    // its knots is no plan
    findValidTraj_ = false;
    trajectory.clear();
    if (!polyTrajSolver::coefficientsFit(extDegree_, extKnots_, xSol_, ySol_, zSol_)) return;
    polyTrajSolver::samplePiecewise(extDegree_, extKnots_, xSol_, ySol_, zSol_, delT, path_.back(), trajectory);
    std::set<int> collisionSeg;
    findValidTraj_ = !this->checkCollisionTraj(trajectory, delT, collisionSeg);
}

// makePlan() of many planners in lock-step: LockStepBatch (polyBatchLoop.h) with the rules below and the device steps —
// ONE vigo_minsnap launch per QP group, and every candidate trajectory checked whole (samples, box sweep and segment
// attribution of checkCollisionTraj, PO.cpp:634-656) by ONE vigo_traj_corridor_check launch with the lead's box and map
// resolution.  A failed device call ends the batch: every planner not yet valid falls back.
struct polyTrajOctomap::DeviceSteps {
    polyTrajOctomap* lead = nullptr;
    bool ready(polyTrajOctomap* l) { lead = l; return l->syncDevice(); }
    bool supported(int W, int diff, int cont) const { return vigo_minsnap_supported(W, 7, diff, cont) != 0; }
    bool solve(int diff, int cont, double vel, double corridorRes, std::vector<vigo_host::QpMember>& qp) {
        return vigo_host::minsnapGroupOnDevice(lead->link_.handle(), diff, cont, vel, corridorRes, qp);
    }
    bool check(std::vector<vigo_host::TrajCheck>& cand) {
        const polyTrajOctomap* l = lead;
        const double box[3] = {l->collisionBox_[0], l->collisionBox_[1], l->collisionBox_[2]};
        return vigo_host::checkTrajectoriesOnDevice(cand, [l, &box](int T, int S, const int32_t* segOff, const double* co, const double* kn,
                                                                    const double* dt, const double* ep, int32_t* status, int32_t* n,
                                                                    uint8_t* flag, int32_t* first, uint8_t* seg) {
            return vigo_traj_corridor_check(l->link_.handle(), T, S, 7, segOff, co, kn, dt, ep, box, l->mapRes_, VIGO_TRAJ_NONFINITE_COLLIDES,
                                            status, n, flag, first, nullptr, seg) == VIGO_OK;
        });
    }
    const char* lastError() const { return vigo_last_error(lead->link_.handle()); }
};

std::vector<bool> polyTrajOctomap::makePlanBatch(const std::vector<polyTrajOctomap*>& ps, std::vector<std::vector<pose>>& trajectories) {
    DeviceSteps steps;
    return vigo_host::LockStepBatch<polyTrajOctomap>::run(ps, false, trajectories, steps);   // (the mode is each planner's own)
}

// Who is batchable and who leads: everything is compared with the FIRST planner of the call (batchReference), the first
// batchable one leads.  The batch cannot take an installed polynomial, a single waypoint, another polynomial degree,
// another QP or sweep geometry, device, map or box than the first planner's, or soft waypoint constraints (the device QP
// takes the waypoints as equalities): those plan on their own.
bool polyTrajOctomap::batchable(const polyTrajOctomap* ref) const {
    return extKnots_.empty() && path_.size() >= 2 && polyDegree_ == 7 && diffDegree_ == ref->diffDegree_ &&
           continuityDegree_ == ref->continuityDegree_ && desiredVel_ == ref->desiredVel_ && corridorRes_ == ref->corridorRes_ &&
           link_.sameTarget(ref->link_) && collisionBox_ == ref->collisionBox_ && mapRes_ == ref->mapRes_ && !softConstraint_;
}
bool polyTrajOctomap::planAlone(std::vector<pose>& trajectory, bool, bool& toldSoft) {
    if (softConstraint_ && !toldSoft) {   // once per call
        cout << "[Trajectory Planner INFO]: soft waypoint constraints: planned on the host path, outside the device batch." << endl;
        toldSoft = true;
    }
    makePlan(trajectory, delT_);
    return findValidTraj_;
}

// Without a device the group is not planned: no trajectory, not valid (syncDevice has said why).
void polyTrajOctomap::planWithoutDevice(const std::vector<polyTrajOctomap*>& ps, const std::vector<size_t>& grp, bool,
                                        std::vector<std::vector<pose>>&, std::vector<bool>&) {
    for (size_t i : grp) ps[i]->findValidTraj_ = false;
}

// The time limit, timeout x (planners in the batch), is tested after a colliding round.
bool polyTrajOctomap::timedOutAfterRound(const PlanState& s, size_t G) const { return vigo_host::nowSec() - s.t0 >= timeout_ * (double)G; }

// The QP group key beside the waypoint count is the mode (sameQpGroup): corridor boxes for the corridor mode, none for the
// adding-waypoint mode.  No conditions are handed to the QP.
vigo_host::QpMember polyTrajOctomap::qpMember(size_t who, const PlanState& s) const {
    return {who, &path_, s.addingWaypoints ? nullptr : &s.corridor, {}, 0, {}};
}

// An infeasible corridor (-2) keeps the previous polynomial, like the reference; a numerical failure of the device QP
// (-1: more than 1024 corridor boxes, say) is solved by the host QP, which has no such limit.
void polyTrajOctomap::takeQpResult(PlanState& s, const vigo_host::QpMember& m) {
    if (m.status == 0) trajSolver_->installSolution(m.sol[0], m.sol[1], m.sol[2]);
    else if (m.status == -1) solveOnHost(s);
}

// A candidate the device check rejects is sampled on the host and swept on the lead's synced handle that round (a failed
// sweep leaves every flag set: the loop goes on); the blame as advanceOnFlags.
void polyTrajOctomap::checkOnHost(polyTrajOctomap& lead, vigo_host::TrajCheck& c) {
    std::vector<pose> traj;
    std::vector<uint8_t> flags;
    std::vector<double> pts;
    trajSolver_->getTrajectory(traj, delT_);
    vigo_host::appendXyz(traj, pts);
    lead.sweepXyz(pts, flags);
    c.segments.clear();
    c.collides = vigo_host::collisionSegments(flags.data(), flags.size(), trajSolver_->getTimeKnot(), delT_, c.segments);
}

// The ending: the polynomial that was found valid, sampled once; the PWL fallback otherwise.  (The loop's verdict is
// findValidTraj_, which advance() keeps.)
bool polyTrajOctomap::finishBatch(std::vector<pose>& trajectory, bool) {
    if (findValidTraj_) trajSolver_->getTrajectory(trajectory, delT_);
    else pwlPlan(trajectory, delT_);
    return findValidTraj_;
}

void polyTrajOctomap::makePlan() {
    std::vector<pose> trajectory;
    this->makePlan(trajectory, this->delT_);
}

void polyTrajOctomap::makePlan(nav_msgs::Path& trajectory, double delT) {
    std::vector<pose> tmp;
    this->makePlan(tmp, delT);
    this->trajMsgConverter(tmp, trajectory);
}

void polyTrajOctomap::trajMsgConverter(const std::vector<pose>& trajectoryTemp, nav_msgs::Path& trajectory) {
    vigo_host::posesToPathMsg(trajectoryTemp, trajectory);
}

// PO.cpp:658-677
geometry_msgs::PoseStamped polyTrajOctomap::getPose(double t) {
    if (t > this->getDuration()) t = this->getDuration();
    if (!trajSolver_ && extKnots_.empty()) {                     // PO.cpp:672-674: the fallback answers in its own words
        if (pwlTrajSolver_) return pwlTrajSolver_->getPose(t);
        geometry_msgs::PoseStamped none;
        none.header.frame_id = "map";
        return none;
    }
    pose p = trajSolver_ ? trajSolver_->getPose(t) : polyTrajSolver::evalPiecewise(extDegree_, extKnots_, xSol_, ySol_, zSol_, t);
    geometry_msgs::PoseStamped ps;
    ps.pose.position.x = p.x; ps.pose.position.y = p.y; ps.pose.position.z = p.z;
    ps.pose.orientation = quaternion_from_rpy(0, 0, p.yaw);
    ps.header.frame_id = "map";
    return ps;
}

// PO.cpp:679-689
double polyTrajOctomap::getDuration() {
    if (this->path_.size() == 1) return 0.0;
    const std::vector<double>& k = timeKnots();
    return k.empty() ? 0.0 : k.back();
}

}  // namespace trajPlanner
