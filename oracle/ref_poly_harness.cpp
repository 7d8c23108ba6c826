/*
 * ref_poly_harness.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Thin extern "C" surface around the VERBATIM reference sources
 *   include/trajectory_planner/polyTrajSolver.cpp, polyTrajOccMap.cpp, piecewiseLinearTraj.cpp (and their headers, utils.h),
 * included from where they lie (the Makefile passes -I$(REF)/include); no reference text is copied here.  Their other
 * includes resolve to oracle/ref_shim/: Eigen (ref_shim/Eigen/Eigen, rule R7 for SparseMatrix), ROS and the messages, the
 * map (this build's own voxel contract), and ref_shim/trajectory_planner/third_party/OsqpEigen/OsqpEigen.h, the stand-in
 * solver that records the QP the reference built and takes the solution from a hook (read that file for what it decides).
 * Output: oracle/_ref/libref_poly.so (git-ignored).
 *
 * tests/test_oracle_ref_poly.py holds tests/minsnap_ref.py, oracle/vigo_oracle.c and the host facades to what this
 * library computes, and tests/golden/make_poly_golden.py records its outputs in tests/golden/poly_ref.npz.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <iomanip>  // utils.h and <sstream> below it: before the access macro, which must not reach the standard library
#include <iostream>
#include <memory>
#include <mutex>    // polyTrajSolver.h includes <thread> and <mutex>: likewise
#include <set>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <Eigen/Eigen>
#include <ros/ros.h>
#include <map_manager/occupancyMap.h>
#include <trajectory_planner/third_party/OsqpEigen/OsqpEigen.h>

/* private members (xSol_, segToTimePose_, trajSolver_, ...) are reached by the access macro of ref_bspline_harness.cpp,
 * placed after every standard and shim header so that only the reference's own classes open up */
#define private public
#define protected public
#include <trajectory_planner/polyTrajSolver.cpp>
#include <trajectory_planner/piecewiseLinearTraj.cpp>
#include <trajectory_planner/polyTrajOccMap.cpp>
#undef private
#undef protected

namespace {
struct Quiet {
    std::ios_base::iostate was;
    Quiet() : was(std::cout.rdstate()) { std::cout.setstate(std::ios_base::failbit); }
    ~Quiet() { std::cout.clear(was); }
};
struct OccHandle {
    trajPlanner::polyTrajOccMap* pm;
    std::shared_ptr<mapManager::occMap> map;
    std::vector<std::vector<double>> rounds;                  // corridorSizeVec_ as each x solve saw it
    std::vector<std::vector<trajPlanner::pose>> roundTraj;    // what getTrajectory returned after each solve()
    int solves;
};
std::vector<trajPlanner::pose> toPath(int n, const double* wp, int stride) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n; ++i) {
        const double* p = wp + static_cast<size_t>(stride) * i;
        path.push_back(stride == 4 ? trajPlanner::pose(p[0], p[1], p[2], p[3]) : trajPlanner::pose(p[0], p[1], p[2]));
    }
    return path;
}
nav_msgs::Path toMsg(int n, const double* wp, int stride) {
    nav_msgs::Path path;
    for (int i = 0; i < n; ++i) {
        const double* p = wp + static_cast<size_t>(stride) * i;
        geometry_msgs::PoseStamped ps;
        ps.pose.position.x = p[0]; ps.pose.position.y = p[1]; ps.pose.position.z = p[2];
        if (stride == 4) ps.pose.orientation = trajPlanner::quaternion_from_rpy(0, 0, p[3]);
        path.poses.push_back(ps);
    }
    return path;
}
/* out[13]: getPose (x, y, z, yaw), getPos, getVel, getAcc */
void evalSolver(trajPlanner::polyTrajSolver* s, double t, double* o) {
    const trajPlanner::pose p = s->getPose(t);
    const Eigen::Vector3d x = s->getPos(t), v = s->getVel(t), a = s->getAcc(t);
    o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = p.yaw;
    for (int q = 0; q < 3; ++q) { o[4 + q] = x(q); o[7 + q] = v(q); o[10 + q] = a(q); }
}
void observeRound(void* user) {
    OccHandle* h = static_cast<OccHandle*>(user);
    if (h->solves++ % 3 != 0) return;
    if (!h->rounds.empty()) h->roundTraj.push_back(h->pm->trajSolver_->trajectory_);  // the round before this one
    h->rounds.push_back(h->pm->trajSolver_->corridorSizeVec_);
}
const int kUndefined = -99;  // a solver error before any solution exists: the reference would read an empty xSol_
const int kNotThreeAxes = -98;  // solve() did not ask the stand-in solver three times: observeRound's count would be off
}  // namespace

extern "C" {

void rps_set_hook(OsqpEigen::shim::Hook hook) { OsqpEigen::shim::hook() = hook; }
long rps_duplicate_inserts() { return Eigen::shim::duplicateInserts(); }

/* ---- the recorded QPs, in the order solveProblem() was called (x, y, z per solve()) ---- */
void rps_log_clear() { OsqpEigen::shim::log().clear(); }
int rps_log_count() { return static_cast<int>(OsqpEigen::shim::log().size()); }
/* shape[4] = n, m, tag (0 setUpProblem, 1 updateProblem), the hook's status */
void rps_log_shape(int i, int32_t* shape) {
    const OsqpEigen::shim::Record& r = OsqpEigen::shim::log()[i];
    shape[0] = r.n; shape[1] = r.m; shape[2] = r.tag; shape[3] = r.status;
}
/* P [n][n], q [n], A [m][n], l [m], u [m], x [n] (the hook's answer, before the reference rescales it); each may be NULL */
void rps_log_get(int i, double* P, double* q, double* A, double* l, double* u, double* x) {
    const OsqpEigen::shim::Record& r = OsqpEigen::shim::log()[i];
    if (P) std::memcpy(P, r.P.data(), sizeof(double) * r.P.size());
    if (q) std::memcpy(q, r.q.data(), sizeof(double) * r.q.size());
    if (A) std::memcpy(A, r.A.data(), sizeof(double) * r.A.size());
    if (l) std::memcpy(l, r.l.data(), sizeof(double) * r.l.size());
    if (u) std::memcpy(u, r.u.data(), sizeof(double) * r.u.size());
    if (x) std::memcpy(x, r.x.data(), sizeof(double) * r.x.size());
}

/* ---- trajPlanner::polyTrajSolver ---- */
void* rps_solver_create(int deg, int diff, int cont, double vel) { return new trajPlanner::polyTrajSolver(deg, diff, cont, vel); }
void rps_solver_destroy(void* vs) { delete static_cast<trajPlanner::polyTrajSolver*>(vs); }
void rps_solver_set_path(void* vs, int n, const double* wp) { static_cast<trajPlanner::polyTrajSolver*>(vs)->updatePath(toPath(n, wp, 3)); }
int rps_solver_continuity(void* vs) { return static_cast<trajPlanner::polyTrajSolver*>(vs)->continuityDegree_; }
int rps_solver_constraints(void* vs) { return static_cast<trajPlanner::polyTrajSolver*>(vs)->constraintNum_; }
/* conds [4][3]: initial velocity, final velocity, initial acceleration, final acceleration */
void rps_solver_set_conds(void* vs, const double* c) {
    trajPlanner::polyTrajSolver* s = static_cast<trajPlanner::polyTrajSolver*>(vs);
    s->updateInitVel(c[0], c[1], c[2]);
    s->updateEndVel(c[3], c[4], c[5]);
    s->updateInitAcc(c[6], c[7], c[8]);
    s->updateEndAcc(c[9], c[10], c[11]);
}
/* the overload with nargs arguments; nargs = -3: what polyTrajOccMap::makePlan passes, (bool, bool, int) = (true, true, 0) */
void rps_solver_set_soft(void* vs, int nargs, const double* r) {
    trajPlanner::polyTrajSolver* s = static_cast<trajPlanner::polyTrajSolver*>(vs);
    if (nargs == 1) s->setSoftConstraint(r[0]);
    else if (nargs == 2) s->setSoftConstraint(r[0], r[1]);
    else if (nargs == 3) s->setSoftConstraint(r[0], r[1], r[2]);
    else { const bool on = true; s->setSoftConstraint(on, on, 0); }
}
/* n > 0: the vector overload with sizes [n]; n == 0: the scalar overload with sizes[0] */
void rps_solver_set_corridor(void* vs, int n, const double* sizes, double res) {
    Quiet quiet;
    trajPlanner::polyTrajSolver* s = static_cast<trajPlanner::polyTrajSolver*>(vs);
    if (n > 0) s->setCorridorConstraint(std::vector<double>(sizes, sizes + n), res);
    else s->setCorridorConstraint(sizes[0], res);
}
/* the boxes in the order constructA and constructBound walk them (the unordered_map's own iteration order, taken from a
 * copy as both functions take it): seg [cap], t [cap], centre [cap][3]; returns how many */
int rps_solver_corridor_order(void* vs, int32_t* seg, double* t, double* centre, int cap) {
    trajPlanner::polyTrajSolver* s = static_cast<trajPlanner::polyTrajSolver*>(vs);
    int k = 0;
    if (!s->corridorConstraint_) return 0;
    for (size_t i = 0; i < s->path_.size() - 1; ++i) {
        if (s->corridorSizeVec_[i] == 0.0) continue;
        std::unordered_map<double, trajPlanner::pose> timeToPose = s->segToTimePose_[i];
        for (auto itr : timeToPose) {
            if (k < cap) {
                seg[k] = static_cast<int32_t>(i);
                t[k] = itr.first;
                centre[3 * k] = itr.second.x; centre[3 * k + 1] = itr.second.y; centre[3 * k + 2] = itr.second.z;
            }
            ++k;
        }
    }
    return k;
}
/* solve(): 0, or kUndefined when an axis failed before it ever had a solution */
int rps_solver_solve(void* vs) {
    Quiet quiet;
    try {
        static_cast<trajPlanner::polyTrajSolver*>(vs)->solve();
    } catch (const OsqpEigen::shim::UndefinedSolution&) {
        return kUndefined;
    }
    return 0;
}
int rps_solver_knots(void* vs, double* out, int cap) {
    const std::vector<double>& k = static_cast<trajPlanner::polyTrajSolver*>(vs)->getTimeKnot();
    for (size_t i = 0; i < k.size() && static_cast<int>(i) < cap; ++i) out[i] = k[i];
    return static_cast<int>(k.size());
}
/* the rescaled xSol_ / ySol_ / zSol_ (axis 0 / 1 / 2) */
int rps_solver_solution(void* vs, int axis, double* out, int cap) {
    trajPlanner::polyTrajSolver* s = static_cast<trajPlanner::polyTrajSolver*>(vs);
    const Eigen::VectorXd& x = axis == 0 ? s->xSol_ : axis == 1 ? s->ySol_ : s->zSol_;
    for (int i = 0; i < x.size() && i < cap; ++i) out[i] = x(i);
    return x.size();
}
/* getTrajectory(trajectory, delT): poses (x, y, z, yaw) into out [cap][4]; returns how many */
int rps_solver_trajectory(void* vs, double delT, double* out, int cap) {
    std::vector<trajPlanner::pose> tr;
    static_cast<trajPlanner::polyTrajSolver*>(vs)->getTrajectory(tr, delT);
    for (size_t i = 0; i < tr.size() && static_cast<int>(i) < cap; ++i) {
        out[4 * i] = tr[i].x; out[4 * i + 1] = tr[i].y; out[4 * i + 2] = tr[i].z; out[4 * i + 3] = tr[i].yaw;
    }
    return static_cast<int>(tr.size());
}
/* out [n_t][13]: getPose (x, y, z, yaw), getPos, getVel, getAcc.  Times outside [0, duration] leave the reference's
 * Vector3d uninitialised: the caller keeps t inside */
void rps_solver_eval(void* vs, int n_t, const double* t, double* out) {
    for (int k = 0; k < n_t; ++k) evalSolver(static_cast<trajPlanner::polyTrajSolver*>(vs), t[k], out + 13 * static_cast<size_t>(k));
}

/* ---- trajPlanner::polyTrajOccMap ---- */
/* cfg[14]: the poly_traj/ keys in initParam()'s order — polynomial_degree, differential_degree, continuity_degree,
 * desired_velocity, desired_acceleration, initial_radius, timeout, corridor_res, shrinking_factor, soft_constraint,
 * constraint_radius, sample_delta_time, maximum_iteration_num, use_pwl_failsafe; NaN: the key is not set */
void* rps_occ_create(const double* cfg) {
    Quiet quiet;
    static const char* keys[14] = {"polynomial_degree", "differential_degree", "continuity_degree", "desired_velocity",
                                   "desired_acceleration", "initial_radius", "timeout", "corridor_res", "shrinking_factor",
                                   "soft_constraint", "constraint_radius", "sample_delta_time", "maximum_iteration_num",
                                   "use_pwl_failsafe"};
    auto& table = ros::shim::params();
    table.clear();
    for (int i = 0; i < 14; ++i)
        if (!std::isnan(cfg[i])) table[std::string("poly_traj/") + keys[i]] = std::vector<double>{cfg[i]};
    OccHandle* h = new OccHandle;
    h->pm = new trajPlanner::polyTrajOccMap(ros::NodeHandle());
    h->solves = 0;
    return h;
}
void rps_occ_destroy(void* vh) {
    OccHandle* h = static_cast<OccHandle*>(vh);
    delete h->pm;
    delete h;
}
void rps_occ_set_map(void* vh, int nx, int ny, int nz, const double* origin, double res, const uint8_t* vox) {
    OccHandle* h = static_cast<OccHandle*>(vh);
    h->map = std::make_shared<mapManager::occMap>(nx, ny, nz, origin, res, vox);
    h->pm->setMap(h->map);
}
/* updatePath(nav_msgs::Path) or, with conds [4][3], updatePath(path, startEndCondition) */
void rps_occ_set_path(void* vh, int n, const double* wp, const double* conds) {
    OccHandle* h = static_cast<OccHandle*>(vh);
    const nav_msgs::Path path = toMsg(n, wp, 3);
    if (conds) {
        std::vector<Eigen::Vector3d> c;
        for (int k = 0; k < 4; ++k) c.push_back(Eigen::Vector3d(conds[3 * k], conds[3 * k + 1], conds[3 * k + 2]));
        h->pm->updatePath(path, c);
    } else {
        h->pm->updatePath(path);
    }
}
/* mode 1: makePlan(trajectory, true), 0: makePlan(trajectory, false), 2: makePlan(trajectory).  traj [cap][4]; *n_traj
 * poses.  Returns the verdict (0 / 1) or kUndefined.  The corridor sizes of every round are read with rps_occ_rounds. */
int rps_occ_make_plan(void* vh, int mode, double* traj, int cap, int32_t* n_traj) {
    Quiet quiet;
    OccHandle* h = static_cast<OccHandle*>(vh);
    h->rounds.clear();
    h->roundTraj.clear();
    h->solves = 0;
    OsqpEigen::shim::observer() = observeRound;
    OsqpEigen::shim::observerUser() = h;
    std::vector<trajPlanner::pose> tr;
    int verdict;
    try {
        verdict = (mode == 2 ? h->pm->makePlan(tr) : h->pm->makePlan(tr, mode != 0)) ? 1 : 0;
    } catch (const OsqpEigen::shim::UndefinedSolution&) {
        verdict = kUndefined;
    }
    OsqpEigen::shim::observer() = nullptr;
    if (verdict != kUndefined && h->solves % 3 != 0) return kNotThreeAxes;  // observeRound counts x, y, z per solve()
    if (!h->rounds.empty() && verdict != kUndefined) h->roundTraj.push_back(h->pm->trajSolver_->trajectory_);
    *n_traj = static_cast<int32_t>(tr.size());
    for (size_t i = 0; i < tr.size() && static_cast<int>(i) < cap; ++i) {
        traj[4 * i] = tr[i].x; traj[4 * i + 1] = tr[i].y; traj[4 * i + 2] = tr[i].z; traj[4 * i + 3] = tr[i].yaw;
    }
    return verdict;
}
/* rounds (= solve() calls) of the last makePlan; sizes [cap][n_seg] */
int rps_occ_rounds(void* vh, int n_seg, double* sizes, int cap) {
    OccHandle* h = static_cast<OccHandle*>(vh);
    for (size_t r = 0; r < h->rounds.size() && static_cast<int>(r) < cap; ++r)
        for (int s = 0; s < n_seg && s < static_cast<int>(h->rounds[r].size()); ++s) sizes[r * n_seg + s] = h->rounds[r][s];
    return static_cast<int>(h->rounds.size());
}
/* the polynomial's samples of round r (getTrajectory's list, before any PWL replacement): out [cap][3]; returns how many */
int rps_occ_round_traj(void* vh, int r, double* out, int cap) {
    OccHandle* h = static_cast<OccHandle*>(vh);
    if (r < 0 || r >= static_cast<int>(h->roundTraj.size())) return -1;
    const std::vector<trajPlanner::pose>& tr = h->roundTraj[r];
    for (size_t i = 0; i < tr.size() && static_cast<int>(i) < cap; ++i) { out[3 * i] = tr[i].x; out[3 * i + 1] = tr[i].y; out[3 * i + 2] = tr[i].z; }
    return static_cast<int>(tr.size());
}
double rps_occ_duration(void* vh) { return static_cast<OccHandle*>(vh)->pm->getDuration(); }
int rps_occ_valid(void* vh) { return static_cast<OccHandle*>(vh)->pm->findValidTraj_ ? 1 : 0; }
/* the inner solver's knots and rescaled solutions, for sampling by the code under test */
void* rps_occ_solver(void* vh) { return static_cast<OccHandle*>(vh)->pm->trajSolver_.get(); }
/* getTrajectory(dt): positions into out [cap][3]; returns how many */
int rps_occ_trajectory(void* vh, double dt, double* out, int cap) {
    const nav_msgs::Path p = static_cast<OccHandle*>(vh)->pm->getTrajectory(dt);
    for (size_t i = 0; i < p.poses.size() && static_cast<int>(i) < cap; ++i) {
        out[3 * i] = p.poses[i].pose.position.x; out[3 * i + 1] = p.poses[i].pose.position.y; out[3 * i + 2] = p.poses[i].pose.position.z;
    }
    return static_cast<int>(p.poses.size());
}
/* through polyTrajOccMap's clamp: out [n_t][16] = getPose position (3) and orientation (x, y, z, w), getPos, getVel, getAcc */
void rps_occ_eval(void* vh, int n_t, const double* t, double* out) {
    trajPlanner::polyTrajOccMap* pm = static_cast<OccHandle*>(vh)->pm;
    for (int k = 0; k < n_t; ++k) {
        double* o = out + 16 * static_cast<size_t>(k);
        const geometry_msgs::PoseStamped ps = pm->getPose(t[k]);
        o[0] = ps.pose.position.x; o[1] = ps.pose.position.y; o[2] = ps.pose.position.z;
        o[3] = ps.pose.orientation.x; o[4] = ps.pose.orientation.y; o[5] = ps.pose.orientation.z; o[6] = ps.pose.orientation.w;
        const Eigen::Vector3d x = pm->getPos(t[k]), v = pm->getVel(t[k]), a = pm->getAcc(t[k]);
        for (int q = 0; q < 3; ++q) { o[7 + q] = x(q); o[10 + q] = v(q); o[13 + q] = a(q); }
    }
}
/* checkCollisionTraj on traj [n][3] with the knots of the inner solver: the flag; seg [cap] gets the set, *n_seg its size */
int rps_occ_check(void* vh, int n, const double* traj, double delT, int32_t* seg, int cap, int32_t* n_seg) {
    std::set<int> cs;
    const bool hit = static_cast<OccHandle*>(vh)->pm->checkCollisionTraj(toPath(n, traj, 3), delT, cs);
    int k = 0;
    for (int s : cs) { if (k < cap) seg[k] = s; ++k; }
    *n_seg = k;
    return hit ? 1 : 0;
}

/* ---- trajPlanner::pwlTraj ---- */
/* wp [n][4] = (x, y, z, yaw).  overload: 0 updatePath(vector, useYaw), 1 updatePath(vector, vel, useYaw),
 * 2 updatePath(nav_msgs::Path, useYaw), 3 updatePath(nav_msgs::Path, vel, useYaw).  makePlan(vector, delT) into
 * traj [cap][4] (returns the count), getTimeKnot() into knots (*n_knots), *duration = getDuration(), and getPose at
 * t [n_t] into pose [n_t][7] = position, orientation (x, y, z, w) */
int rps_pwl(int n, const double* wp, int overload, int use_yaw, double vel, double delT, double* traj, int cap, double* knots,
            int32_t* n_knots, double* duration, int n_t, const double* t, double* pose) {
    Quiet quiet;
    trajPlanner::pwlTraj pw{ros::NodeHandle()};
    const bool yaw = use_yaw != 0;
    if (overload == 0) pw.updatePath(toPath(n, wp, 4), yaw);
    else if (overload == 1) pw.updatePath(toPath(n, wp, 4), vel, yaw);
    else if (overload == 2) pw.updatePath(toMsg(n, wp, 4), yaw);
    else pw.updatePath(toMsg(n, wp, 4), vel, yaw);
    std::vector<trajPlanner::pose> tr;
    pw.makePlan(tr, delT);
    for (size_t i = 0; i < tr.size() && static_cast<int>(i) < cap; ++i) {
        traj[4 * i] = tr[i].x; traj[4 * i + 1] = tr[i].y; traj[4 * i + 2] = tr[i].z; traj[4 * i + 3] = tr[i].yaw;
    }
    const std::vector<double> k = pw.getTimeKnot();
    *n_knots = static_cast<int32_t>(k.size());
    for (size_t i = 0; i < k.size(); ++i) knots[i] = k[i];
    *duration = pw.getDuration();
    for (int q = 0; q < n_t; ++q) {
        const geometry_msgs::PoseStamped ps = pw.getPose(t[q]);
        double* o = pose + 7 * static_cast<size_t>(q);
        o[0] = ps.pose.position.x; o[1] = ps.pose.position.y; o[2] = ps.pose.position.z;
        o[3] = ps.pose.orientation.x; o[4] = ps.pose.orientation.y; o[5] = ps.pose.orientation.z; o[6] = ps.pose.orientation.w;
    }
    return static_cast<int>(tr.size());
}

}  // extern "C"
