/*
 * ref_bspline_harness.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Thin extern "C" surface around the VERBATIM reference sources
 *   include/trajectory_planner/bspline.cpp, path_search/astarOcc.cpp, bsplineTraj.cpp (and their headers, utils.h,
 *   solver/lbfgs.hpp),
 * included from where they lie (the Makefile passes -I$(REF)/include); no reference text is copied here.  Their other
 * includes (Eigen, ROS, messages, tf2, map_manager, global_planner) resolve to oracle/ref_shim/, headers of this
 * project's own writing: read ref_shim/Eigen/Eigen for the rules that decide bits and for what stays unpinned (the order of
 * Eigen's three-element reductions: a run-time switch here; colPivHouseholderQr's pivot order), and
 * ref_shim/map_manager/occupancyMap.h for the map, which is this build's own voxel contract, not the reference's
 * external map_manager package.  Output: oracle/_ref/libref_bspline.so (git-ignored).
 *
 * tests/test_oracle_ref_bspline.py holds oracle/vigo_oracle.c to what this library computes, and
 * tests/golden/make_golden.py records its outputs in tests/golden/bspline_ref.npz.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <limits>
#include <memory>
#include <queue>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include <Eigen/Eigen>
#include <ros/ros.h>
#include <map_manager/occupancyMap.h>

/* private members (optData_, controlPointsTs_, notCheckRatio_, collisionSeg_, the inline gates) are reached by the usual
 * access macro, placed after every standard and shim header so that only the reference's own classes open up */
#define private public
#define protected public
#include <trajectory_planner/bspline.cpp>
#include <trajectory_planner/path_search/astarOcc.cpp>
#include <trajectory_planner/bsplineTraj.cpp>
#undef private
#undef protected

namespace {
struct Handle {
    trajPlanner::bsplineTraj* bt;
    std::shared_ptr<mapManager::occMap> map;
};
/* the reference narrates on std::cout: quiet for the length of one call into it, then as the process had it */
struct Quiet {
    std::ios_base::iostate was;
    Quiet() : was(std::cout.rdstate()) { std::cout.setstate(std::ios_base::failbit); }
    ~Quiet() { std::cout.clear(was); }
};
Eigen::MatrixXd toMatrix(int N, const double* ctrl) {
    Eigen::MatrixXd m(3, N);
    std::memcpy(m.data(), ctrl, sizeof(double) * 3 * N);
    return m;
}
}  // namespace

extern "C" {

/* 0: (x0 + x1) + x2, 1: x0 + (x1 + x2) — ref_shim/Eigen/Eigen rule R5 */
void rbs_set_reduction_order(int order) { Eigen::shim::reductionOrder() = order ? 1 : 0; }

/* p[20]: timestep, distance_threshold, max_vel, max_acc, weight_distance, weight_smoothness, weight_feasibility,
 * weight_dynamic_obstacle, plan_in_z_axis, min_height, max_height, uncertain_aware_factor, prediction_horizon,
 * distance_threshold_dynamic, max_path_length, max_obstacle_size[3] — the keys initParam() reads, through the shim's
 * parameter table — then the two members that have no key: controlPointsTs_, notCheckRatio_. */
void* rbs_create(const double* p) {
    Quiet quiet;
    static const char* keys[15] = {"timestep", "distance_threshold", "max_vel", "max_acc", "weight_distance",
                                   "weight_smoothness", "weight_feasibility", "weight_dynamic_obstacle", "plan_in_z_axis",
                                   "min_height", "max_height", "uncertain_aware_factor", "prediction_horizon",
                                   "distance_threshold_dynamic", "max_path_length"};
    auto& table = ros::shim::params();
    table.clear();
    for (int i = 0; i < 15; ++i) table[std::string("bspline_traj/") + keys[i]] = std::vector<double>{p[i]};
    table["bspline_traj/max_obstacle_size"] = std::vector<double>{p[15], p[16], p[17]};
    Handle* h = new Handle;
    h->bt = new trajPlanner::bsplineTraj(ros::NodeHandle());
    h->bt->controlPointsTs_ = p[18];
    h->bt->notCheckRatio_ = p[19];
    return h;
}

void rbs_destroy(void* vh) {
    Handle* h = static_cast<Handle*>(vh);
    delete h->bt;
    delete h;
}

void rbs_set_map(void* vh, int nx, int ny, int nz, const double* origin, double res, const uint8_t* vox) {
    Quiet quiet;
    Handle* h = static_cast<Handle*>(vh);
    h->map = std::make_shared<mapManager::occMap>(nx, ny, nz, origin, res, vox);
    h->bt->setMap(h->map);
}

/* control points [N][3]; clears the guide pairs */
void rbs_set_ctrl(void* vh, int N, const double* ctrl) {
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    bt->optData_.controlPoints = toMatrix(N, ctrl);
    bt->optData_.guidePoints.assign(N, std::vector<Eigen::Vector3d>());
    bt->optData_.guideDirections.assign(N, std::vector<Eigen::Vector3d>());
    bt->optData_.findGuidePoint.assign(N, false);
    bt->collisionSeg_.clear();
    bt->astarPaths_.clear();
    bt->init_ = true;
}

void rbs_get_ctrl(void* vh, double* out) {
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    std::memcpy(out, bt->optData_.controlPoints.data(), sizeof(double) * 3 * bt->optData_.controlPoints.cols());
}

/* CSR guide pairs of one trajectory: goff[N + 1], gpv[G][6] = (point, direction) */
void rbs_set_guides(void* vh, const int32_t* goff, const double* gpv) {
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    const int N = bt->optData_.controlPoints.cols();
    for (int i = 0; i < N; ++i) {
        bt->optData_.guidePoints[i].clear();
        bt->optData_.guideDirections[i].clear();
        for (int j = goff[i] - goff[0]; j < goff[i + 1] - goff[0]; ++j) {
            bt->optData_.guidePoints[i].push_back(Eigen::Vector3d(gpv[6 * j], gpv[6 * j + 1], gpv[6 * j + 2]));
            bt->optData_.guideDirections[i].push_back(Eigen::Vector3d(gpv[6 * j + 3], gpv[6 * j + 4], gpv[6 * j + 5]));
        }
    }
}

/* obs[n][9] = (pos, vel, size) */
void rbs_set_obstacles(void* vh, int n, const double* obs) {
    std::vector<Eigen::Vector3d> pos, vel, size;
    for (int i = 0; i < n; ++i) {
        pos.push_back(Eigen::Vector3d(obs[9 * i], obs[9 * i + 1], obs[9 * i + 2]));
        vel.push_back(Eigen::Vector3d(obs[9 * i + 3], obs[9 * i + 4], obs[9 * i + 5]));
        size.push_back(Eigen::Vector3d(obs[9 * i + 6], obs[9 * i + 7], obs[9 * i + 8]));
    }
    static_cast<Handle*>(vh)->bt->updateDynamicObstacles(pos, vel, size);
}

void rbs_set_weights(void* vh, const double* w) {
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    bt->weightDistance_ = w[0];
    bt->weightSmoothness_ = w[1];
    bt->weightFeasibility_ = w[2];
    bt->weightDynamicObstacle_ = w[3];
}

/* one cost term on the current control points: 0 distance, 1 smoothness, 2 feasibility, 3 dynamic obstacle;
 * grad [N][3], started from zero as costFunction() does */
double rbs_term(void* vh, int which, double* grad) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    const Eigen::MatrixXd& c = bt->optData_.controlPoints;
    Eigen::MatrixXd g = Eigen::MatrixXd::Zero(3, c.cols());
    double cost = 0;
    if (which == 0) bt->getDistanceCost(c, cost, g);
    else if (which == 1) bt->getSmoothnessCost(c, cost, g);
    else if (which == 2) bt->getFeasibilityCost(c, cost, g);
    else bt->getDynamicObstacleCost(c, cost, g);
    std::memcpy(grad, g.data(), sizeof(double) * 3 * c.cols());
    return cost;
}

/* costFunction through solverCostFunction: x, grad [n = 3 (N - 6)] */
double rbs_cost(void* vh, int n, const double* x, double* grad) {
    Quiet quiet;
    return trajPlanner::bsplineTraj::solverCostFunction(static_cast<Handle*>(vh)->bt, x, grad, n);
}

/* the reference's own optimize(): its status; the control points after it are read with rbs_get_ctrl */
int rbs_optimize(void* vh) {
    Quiet quiet;
    return static_cast<Handle*>(vh)->bt->optimize();
}

/* the driver call of optimize() with max_iterations as an argument (optimize() fixes 200), which also hands back what
 * optimize() keeps to itself: the final x [n] and cost */
int rbs_optimize_iters(void* vh, int max_iterations, double* x_out, double* fx_out) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    const int n = 3 * (bt->optData_.controlPoints.cols() - 2 * bsplineDegree);
    std::memcpy(x_out, bt->optData_.controlPoints.data() + 3 * bsplineDegree, sizeof(double) * n);
    lbfgs::lbfgs_parameter_t sp;
    lbfgs::lbfgs_load_default_parameters(&sp);
    sp.mem_size = 16;
    sp.max_iterations = max_iterations;
    sp.g_epsilon = 0.01;
    return lbfgs::lbfgs_optimize(n, x_out, fx_out, trajPlanner::bsplineTraj::solverCostFunction, NULL, NULL, bt, &sp);
}

/* bspline(3, ctrl, ts), getDerivative() deriv times, at(t) */
void rbs_bspline_at(int N, const double* ctrl, double ts, int deriv, double t, double* out) {
    trajPlanner::bspline s(bsplineDegree, toMatrix(N, ctrl), ts);
    for (int d = 0; d < deriv; ++d) s = s.getDerivative();
    Eigen::VectorXd p = s.at(t);
    for (int a = 0; a < 3; ++a) out[a] = p(a);
}

/* evalTraj(dt) (dt > 0) or evalTraj() (dt <= 0: the gates' own clock): number of samples; the first cap go to out [cap][3] */
int rbs_eval_traj(void* vh, double dt, double* out, int cap) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    std::vector<Eigen::Vector3d> tr = dt > 0 ? bt->evalTraj(dt) : bt->evalTraj();
    for (int i = 0; i < static_cast<int>(tr.size()) && i < cap; ++i)
        for (int a = 0; a < 3; ++a) out[3 * i + a] = tr[i](a);
    return static_cast<int>(tr.size());
}

/* parameterizeToBspline: points [K][3], cond [4][3] -> ctrl_out [K + 2][3]; A_out [(K + 4)(K + 2)] row-major and
 * b_out [3][K + 4] are the system the reference built.  Inputs on which the reference calls exit(0) return -1 unseen. */
int rbs_fit(int K, double ts, const double* points, const double* cond, double* ctrl_out, double* A_out, double* b_out) {
    Quiet quiet;
    if (!(ts > 0) || K <= 3) return -1;
    std::vector<Eigen::Vector3d> pts, cnd;
    for (int i = 0; i < K; ++i) pts.push_back(Eigen::Vector3d(points[3 * i], points[3 * i + 1], points[3 * i + 2]));
    for (int i = 0; i < 4; ++i) cnd.push_back(Eigen::Vector3d(cond[3 * i], cond[3 * i + 1], cond[3 * i + 2]));
    Eigen::MatrixXd cp;
    Eigen::shim::lastQrB().clear();
    trajPlanner::bspline::parameterizeToBspline(ts, pts, cnd, cp);
    std::memcpy(ctrl_out, cp.data(), sizeof(double) * 3 * (K + 2));
    if (A_out) std::memcpy(A_out, Eigen::shim::lastQrA().data(), sizeof(double) * (K + 4) * (K + 2));
    if (b_out)
        for (int a = 0; a < 3; ++a) std::memcpy(b_out + a * (K + 4), Eigen::shim::lastQrB()[a].data(), sizeof(double) * (K + 4));
    return 0;
}

int rbs_has_collision(void* vh) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    return bt->hasCollisionTrajectory(bt->optData_.controlPoints) ? 1 : 0;
}
int rbs_has_collision_pos(void* vh, double* pos) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    Eigen::Vector3d p(NAN, NAN, NAN);
    const bool hit = bt->hasCollisionTrajectory(bt->optData_.controlPoints, p);
    for (int a = 0; a < 3; ++a) pos[a] = p(a);
    return hit ? 1 : 0;
}
int rbs_has_dynamic_collision(void* vh) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    return bt->hasDynamicCollisionTrajectory(bt->optData_.controlPoints) ? 1 : 0;
}

/* findCollisionSeg on the current control points: pairs into seg [cap][2]; returns how many */
int rbs_find_collision_seg(void* vh, int32_t* seg, int cap) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    std::vector<std::pair<int, int>> s;
    bt->findCollisionSeg(bt->optData_.controlPoints, s);
    for (int i = 0; i < static_cast<int>(s.size()) && i < cap; ++i) { seg[2 * i] = s[i].first; seg[2 * i + 1] = s[i].second; }
    return static_cast<int>(s.size());
}

/* makePlan()'s steps 1-3: findCollisionSeg -> pathSearch -> assignGuidePointsSemiCircle.  Returns the number of
 * segments after pathSearch (which may merge them), or -1 when A* fails (makePlan() returns there); -2 when cap is too
 * small.  seg [cap][2]; path_off [nseg + 1] + path_pts [cap][3]: the A* paths; guide_off [N + 1] + guide_pv [cap][6]. */
int rbs_prologue(void* vh, int32_t* seg, int32_t* path_off, double* path_pts, int32_t* guide_off, double* guide_pv, int cap) {
    Quiet quiet;
    trajPlanner::bsplineTraj* bt = static_cast<Handle*>(vh)->bt;
    bt->findCollisionSeg(bt->optData_.controlPoints, bt->collisionSeg_);
    if (!bt->pathSearch(bt->collisionSeg_, bt->astarPaths_)) return -1;
    bt->assignGuidePointsSemiCircle(bt->astarPaths_, bt->collisionSeg_);
    const int nseg = static_cast<int>(bt->collisionSeg_.size());
    if (nseg > cap) return -2;
    for (int i = 0; i < nseg; ++i) { seg[2 * i] = bt->collisionSeg_[i].first; seg[2 * i + 1] = bt->collisionSeg_[i].second; }
    int k = 0;
    path_off[0] = 0;
    for (size_t i = 0; i < bt->astarPaths_.size(); ++i) {
        for (const Eigen::Vector3d& p : bt->astarPaths_[i]) {
            if (k >= cap) return -2;
            for (int a = 0; a < 3; ++a) path_pts[3 * k + a] = p(a);
            ++k;
        }
        path_off[i + 1] = k;
    }
    const int N = bt->optData_.controlPoints.cols();
    k = 0;
    guide_off[0] = 0;
    for (int i = 0; i < N; ++i) {
        for (size_t j = 0; j < bt->optData_.guidePoints[i].size(); ++j) {
            if (k >= cap) return -2;
            for (int a = 0; a < 3; ++a) {
                guide_pv[6 * k + a] = bt->optData_.guidePoints[i][j](a);
                guide_pv[6 * k + 3 + a] = bt->optData_.guideDirections[i][j](a);
            }
            ++k;
        }
        guide_off[i + 1] = k;
    }
    return nseg;
}

}  // extern "C"
