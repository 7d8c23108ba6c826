// cabi_host.cpp — small extern "C" entry points of libtrajectory_planner_vigo.so so the Python
// tests can exercise the host-side pieces that have no GPU part (the .bt reader and the min-snap
// QP) with ctypes.  Not part of include/vigo.h (that is the device ABI).
#ifdef VIGO_WITH_ROS
#error "tools of the in-tree dense map (standin/dense_occmap.h): not part of a build against map_manager"
#endif
#include <trajectory_planner/bsplineTraj.h>
#include <trajectory_planner/octomapBt.h>
#include <trajectory_planner/path_search/astarOcc.h>
#include <trajectory_planner/piecewiseLinearTraj.h>
#include <trajectory_planner/polyTrajOccMap.h>
#include <trajectory_planner/polyTrajOctomap.h>
#include <trajectory_planner/polyTrajSolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>

#include "../../../include/vigo.h"
#include "../../csrc/vigo_astar_core.hpp"
#include "../../csrc/vigo_guide_core.hpp"
#include "../../csrc/vigo_pathsearch_core.hpp"
#include "../../csrc/vigo_reguide_core.hpp"
#include "batchLayout.h"
#include "cabiPlanBatch.h"
#include "workerPool.h"

namespace {
using namespace cabi;

// cfg as vigo_host_poly_plan documents it; `mode`, the differential and the continuity degree are the caller's
std::unique_ptr<trajPlanner::polyTrajOctomap> makePolyPlanner(const std::shared_ptr<mapManager::occMap>& map, const double* cfg,
                                                               double mode, int diff, int cont, const std::vector<trajPlanner::pose>& path) {
    static const char* keys[7] = {"map_resolution", "sample_delta_time", "desired_velocity", "initial_radius", "shrinking_factor",
                                  "corridor_res", "maximum_iteration_num"};
    ros::NodeHandle nh;
    nh.setParam("collision_box", std::vector<double>{cfg[0], cfg[1], cfg[2]});
    for (int k = 0; k < 7; ++k) nh.setParam(keys[k], cfg[3 + k]);
    nh.setParam("traj_timeout", cfg[10]);
    nh.setParam("mode", mode);
    nh.setParam("polynomial_degree", 7.0);
    nh.setParam("differential_degree", (double)diff);
    nh.setParam("continuity_degree", (double)cont);
    std::unique_ptr<trajPlanner::polyTrajOctomap> p(new trajPlanner::polyTrajOctomap(nh));
    p->setMap(map);
    p->updatePath(path);
    return p;
}

std::vector<trajPlanner::pose> posesFromXyz(const double* q, int n) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n; ++i) path.push_back(trajPlanner::pose(q[3 * i], q[3 * i + 1], q[3 * i + 2]));
    return path;
}

// the first `cap` positions as xyz triples
void copyXyz(const std::vector<trajPlanner::pose>& traj, int cap, double* out) {
    const int n = (int)traj.size() < cap ? (int)traj.size() : cap;
    for (int k = 0; k < n; ++k) { out[3 * k] = traj[k].x; out[3 * k + 1] = traj[k].y; out[3 * k + 2] = traj[k].z; }
}
void copyXyz(const nav_msgs::Path& path, int cap, double* out) {
    const int n = (int)path.poses.size() < cap ? (int)path.poses.size() : cap;
    for (int k = 0; k < n; ++k) {
        const geometry_msgs::Point& q = path.poses[k].pose.position;
        out[3 * k] = q.x; out[3 * k + 1] = q.y; out[3 * k + 2] = q.z;
    }
}

double secondsSince(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The two makePlanBatch test entries of the min-snap planners: P planners from make(i), warm(planner) outside the timed
// region (the handle-creating device call, where the class has one), ONE timed batch(planners, trajectories, verdicts),
// report(planner, verdict, trajectory, i, false); then, when the caller wants them, P twins planned alone — each made,
// warmed, timed alone by solo(planner, trajectory) and reported with `true`.  secs_out[2] (may be NULL): seconds of the
// batch, of the P solo plans.
template <class Make, class Warm, class Batch, class Solo, class Report>
void batchThenSoloTwins(int P, bool twins, double* secs_out, Make make, Warm warm, Batch batch, Solo solo, Report report) {
    std::vector<decltype(make(0))> own;
    std::vector<decltype(make(0).get())> ps;
    for (int i = 0; i < P; ++i) { own.push_back(make(i)); ps.push_back(own.back().get()); }
    if (P > 0) warm(*ps[0]);
    std::vector<std::vector<trajPlanner::pose>> trajs;
    std::vector<bool> r;
    auto t0 = std::chrono::steady_clock::now();
    batch(ps, trajs, r);
    if (secs_out) secs_out[0] = secondsSince(t0);
    for (int i = 0; i < P; ++i) report(*ps[i], (bool)r[i], trajs[i], i, false);
    if (!twins) return;
    double solo_secs = 0.0;
    for (int i = 0; i < P; ++i) {
        auto p = make(i);
        std::vector<trajPlanner::pose> traj;
        warm(*p);
        t0 = std::chrono::steady_clock::now();
        const bool ri = solo(*p, traj);
        solo_secs += secondsSince(t0);
        report(*p, ri, traj, i, true);
    }
    if (secs_out) secs_out[1] = solo_secs;
}

// a dense byte grid as the kernels' twins read it (standin/dense_occmap.h byteAt): posToIndex is floor((p - origin) / res),
// the range test is made on the double, outside is 0xFF (occupied and unknown).  Called, it is the point predicate the
// core headers take.
struct DenseGrid {
    const unsigned char* vox;
    const int* dims;
    const double* origin;
    double res;
    unsigned byteAt(double x, double y, double z) const {
        const double f[3] = {std::floor((x - origin[0]) / res), std::floor((y - origin[1]) / res), std::floor((z - origin[2]) / res)};
        for (int a = 0; a < 3; ++a)
            if (!(f[a] >= 0.0 && f[a] < (double)dims[a])) return 0xFFu;
        return vox[((size_t)f[0] * dims[1] + (size_t)f[1]) * dims[2] + (size_t)f[2]];
    }
    bool occupied(double x, double y, double z) const { return byteAt(x, y, z) & 1u; }
    bool operator()(double x, double y, double z) const { return occupied(x, y, z); }
};

// occ(i) / line(i) of collision_segs and reguide_rules for the control points c[N][3]
auto ctrlFlags(const DenseGrid& g, const double* c) {
    return std::make_pair([&g, c](int i) { return g.occupied(c[3 * i], c[3 * i + 1], c[3 * i + 2]); },
                          [&g, c](int i) { return vigo::line_occupied(g, g.res, c + 3 * (i - 1), c + 3 * i); });
}

}  // namespace

extern "C" {

// returns 0 on success; info: nodes_header, nodes_parsed, bytes, occupied, free, nx, ny, nz; origin[3]; res
int vigo_host_bt_info(const char* path, long long* info, double* origin, double* res) {
    trajPlanner::BtInfo bi;
    const double inflate[3] = {0, 0, 0};
    auto m = trajPlanner::loadOctomapBt(path, inflate, 0, &bi);
    if (!m) return -1;
    info[0] = bi.nodes_header; info[1] = bi.nodes_parsed; info[2] = bi.bytes_consumed; info[3] = bi.occupied; info[4] = bi.free_;
    info[5] = m->nx(); info[6] = m->ny(); info[7] = m->nz();
    for (int a = 0; a < 3; ++a) origin[a] = m->origin()(a);
    *res = m->getRes();
    return 0;
}

// dense voxels of a .bt (caller allocates nx*ny*nz bytes as reported by vigo_host_bt_info with the same arguments)
int vigo_host_bt_load(const char* path, const double* inflate, int margin, unsigned char* out, long long cap, int* dims, double* origin) {
    auto m = trajPlanner::loadOctomapBt(path, inflate, margin, nullptr);
    if (!m) return -1;
    dims[0] = m->nx(); dims[1] = m->ny(); dims[2] = m->nz();
    for (int a = 0; a < 3; ++a) origin[a] = m->origin()(a);
    if ((long long)m->voxels().size() > cap) return -2;
    std::memcpy(out, m->voxels().data(), m->voxels().size());
    return 0;
}

// dense voxels of an ASCII .pcd at resolution res: first call with out == NULL to get dims/origin/points
int vigo_host_pcd_load(const char* path, double res, const double* inflate, int margin, unsigned char* out, long long cap, int* dims,
                       double* origin, long long* points) {
    auto m = trajPlanner::loadPcdAscii(path, res, inflate, margin, points);
    if (!m) return -1;
    dims[0] = m->nx(); dims[1] = m->ny(); dims[2] = m->nz();
    for (int a = 0; a < 3; ++a) origin[a] = m->origin()(a);
    if (!out) return 0;
    if ((long long)m->voxels().size() > cap) return -2;
    std::memcpy(out, m->voxels().data(), m->voxels().size());
    return 0;
}

// bsplineTraj's host prologue of makePlan() (BT.cpp:333-350: findCollisionSeg -> pathSearch -> assignGuidePointsSemiCircle)
// on a dense byte grid, after updatePath() over n_path poses (zero start / end conditions).  cfg: distance_threshold,
// min_height, max_height, max_obstacle_size[3].  Outputs (caller-sized, cap doubles / ints each):
//   ctrl_out  3 * N control points (column by column), returns N through *n_ctrl
//   seg_out   pairs of the collision segments AFTER pathSearch, *n_seg of them; -1 in *n_seg when A* failed
//   guide_off N + 1 offsets into guide_out, which holds (point, direction) 6-tuples per control point, in push order
//   path_off / path_out: the A* paths (with the segment ends put in, BT.cpp:455-457) as xyz triples
// Returns 0, -1 when updatePath refuses the path, -2 when a buffer is too small.
int vigo_host_bspline_prologue(const unsigned char* vox, const int* dims, const double* origin, double res, int n_path, const double* path_xyz,
                               const double* cfg, double* ctrl_out, int* n_ctrl, int* seg_out, int* n_seg, int* guide_off, double* guide_out,
                               int* path_off, double* path_out, int cap) {
    ros::NodeHandle nh;
    setBsplineParams(nh, cfg);
    nh.setParam("bspline_traj/max_path_length", 1000.0);
    trajPlanner::bsplineTraj bt(nh);
    bt.setMap(denseMap(dims[0], dims[1], dims[2], origin, res, vox));
    if (!bt.updatePath(pathFromXyz(path_xyz, n_path), std::vector<Eigen::Vector3d>(4, Eigen::Vector3d(0, 0, 0)))) return -1;
    const Eigen::MatrixXd c = bt.getControlPoints();
    const int N = (int)c.cols();
    if (3 * N > cap) return -2;
    *n_ctrl = N;
    for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) ctrl_out[3 * i + k] = c(k, i);
    std::vector<std::pair<int, int>> seg;
    std::vector<std::vector<Eigen::Vector3d>> paths;
    bt.findCollisionSeg(c, seg);
    if (!bt.pathSearch(seg, paths)) { *n_seg = -1; return 0; }
    bt.assignGuidePointsSemiCircle(paths, seg);
    if (2 * (int)seg.size() > cap) return -2;
    *n_seg = (int)seg.size();
    for (size_t i = 0; i < seg.size(); ++i) { seg_out[2 * i] = seg[i].first; seg_out[2 * i + 1] = seg[i].second; }
    std::vector<int32_t> off{0};
    std::vector<double> pv;
    vigo_host::appendGuides(bt.getOptData(), N, off, pv);
    if ((long long)pv.size() > cap) return -2;
    std::copy(off.begin(), off.end(), guide_off);
    std::copy(pv.begin(), pv.end(), guide_out);
    int q = 0;
    for (size_t i = 0; i < paths.size(); ++i) {
        path_off[i] = q;
        for (const auto& v : paths[i]) {
            if (3 * (q + 1) > cap) return -2;
            for (int k = 0; k < 3; ++k) path_out[3 * q + k] = v(k);
            ++q;
        }
    }
    path_off[paths.size()] = q;
    return 0;
}

// one AStar::AstarSearch on a dense byte grid (bit 0 = inflated-occupied): returns the number of path points written
// (xyz triples, start side first), -1 when no path is found, -2 when path_out is too small
int vigo_host_astar(const unsigned char* vox, const int* dims, const double* origin, double res, const int* pool, double min_height,
                    double max_height, double step, const double* start, const double* end, double* path_out, int cap) {
    auto m = denseMap(dims[0], dims[1], dims[2], origin, res, vox);
    AStar a;
    a.initGridMap(m, Eigen::Vector3i(pool[0], pool[1], pool[2]), min_height, max_height);
    if (!a.AstarSearch(step, Eigen::Vector3d(start[0], start[1], start[2]), Eigen::Vector3d(end[0], end[1], end[2]))) return -1;
    const std::vector<Eigen::Vector3d> path = a.getPath();
    if ((int)path.size() > cap) return -2;
    for (size_t i = 0; i < path.size(); ++i)
        for (int k = 0; k < 3; ++k) path_out[3 * i + k] = path[i](k);
    return (int)path.size();
}

// vigo_host_astar plus what the search did: stats[5] = nodes popped, nodes reached (blocked ones included), the open
// set's largest size, in-place score rewrites, nodes pushed (AStar::lastStats); filled whatever the outcome
int vigo_host_astar_stats(const unsigned char* vox, const int* dims, const double* origin, double res, const int* pool, double min_height,
                          double max_height, double step, const double* start, const double* end, double* path_out, int cap, int* stats) {
    auto m = denseMap(dims[0], dims[1], dims[2], origin, res, vox);
    AStar a;
    a.initGridMap(m, Eigen::Vector3i(pool[0], pool[1], pool[2]), min_height, max_height);
    const bool ok = a.AstarSearch(step, Eigen::Vector3d(start[0], start[1], start[2]), Eigen::Vector3d(end[0], end[1], end[2]));
    stats[0] = a.lastStats.pops; stats[1] = a.lastStats.nodes; stats[2] = a.lastStats.heapPeak; stats[3] = a.lastStats.rewrites;
    stats[4] = a.lastStats.pushed;
    if (!ok) return -1;
    const std::vector<Eigen::Vector3d> path = a.getPath();
    if ((int)path.size() > cap) return -2;
    for (size_t i = 0; i < path.size(); ++i)
        for (int k = 0; k < 3; ++k) path_out[3 * i + k] = path[i](k);
    return (int)path.size();
}

// the same search by the device's search core (csrc/vigo_astar_core.hpp) compiled for the host: a table of
// 1 << cap_log2 slots holding at most max_nodes nodes, a heap of heap_cap entries, max_expansions pops.  Returns the
// status (VIGO_ASTAR_*: 0 found, 1 not found, 2 deferred, 3 path longer than path_cap), -1 for an argument the device
// entry refuses; *len_out path points in path_out (written only when found), stats as vigo_host_astar_stats.
int vigo_host_astar_core(const unsigned char* vox, const int* dims, const double* origin, double res, const int* pool, double min_height,
                         double max_height, double step, const double* start, const double* end, int cap_log2, int max_nodes, int heap_cap,
                         int max_expansions, int path_cap, double* path_out, int* len_out, int* stats) {
    if (cap_log2 < 1 || cap_log2 > 30 || max_nodes < 1 || max_nodes >= (1 << cap_log2) || heap_cap < 1 || path_cap < 2 || !(step > 0)) return -1;
    for (int a = 0; a < 3; ++a)
        if (pool[a] < 3 || pool[a] > vigo::kAstarMaxPoolAxis) return -1;
    const size_t n = (size_t)1 << cap_log2;
    std::vector<int32_t> key(n, -1), heap((size_t)heap_cap);
    std::vector<double> g(n);
    std::vector<uint8_t> meta(n);
    vigo::AstarStore<int32_t> S{};
    S.key = key.data(); S.g = g.data(); S.meta = meta.data(); S.heap = heap.data();
    S.cap_log2 = cap_log2; S.max_nodes = max_nodes; S.heap_cap = heap_cap;
    const DenseGrid occ{vox, dims, origin, res};
    const int st = vigo::astar_search(S, occ, start, end, step, pool, min_height, max_height, max_expansions, path_cap, path_out, len_out);
    stats[0] = S.pops; stats[1] = S.n_nodes; stats[2] = S.heap_peak; stats[3] = S.rewrites;
    return st;
}

// The A* searches of makePlan()'s prologue for n sets of control points [n][N][3] on one dense byte grid: the first-choice
// search (segment start -> segment end) of every collision segment findCollisionSeg reports, run by the host A*.  cfg as
// in vigo_host_bspline_prologue.  Per search q < cap (the return value counts them all; -1 on a bad argument):
//   ends[q][6] start xyz, end xyz; owner[q] the planner; len[q] path points or -1; path[q][path_cap][3] (when it fits);
//   stats[q][5] as vigo_host_astar_stats.  pool_out[3]: the planners' node pool.
int vigo_host_prologue_searches(const unsigned char* vox, const int* dims, const double* origin, double res, int n, int N, const double* ctrl,
                                const double* cfg, int cap, int path_cap, double* ends, int* owner, int* len, double* path, int* stats,
                                int* pool_out) {
    if (n < 0 || N < 7 || !ctrl) return -1;
    auto m = denseMap(dims[0], dims[1], dims[2], origin, res, vox);
    ros::NodeHandle nh;
    setBsplineParams(nh, cfg);
    trajPlanner::bsplineTraj bt(nh);
    bt.setMap(m);
    nodePool(cfg, res, pool_out);
    const Eigen::Vector3i pool(pool_out[0], pool_out[1], pool_out[2]);
    AStar a;
    a.initGridMap(m, pool, cfg[1], cfg[2]);
    int q = 0;
    for (int t = 0; t < n; ++t) {
        Eigen::MatrixXd c(3, N);
        for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) c(k, i) = ctrl[((size_t)t * N + i) * 3 + k];
        std::vector<std::pair<int, int>> seg;
        bt.findCollisionSeg(c, seg);
        for (const auto& sg : seg) {
            if (q < cap) {
                const Eigen::Vector3d s = c.col(sg.first), e = c.col(sg.second);
                for (int k = 0; k < 3; ++k) { ends[6 * q + k] = s(k); ends[6 * q + 3 + k] = e(k); }
                owner[q] = t;
                const bool ok = a.AstarSearch(res, s, e);
                stats[5 * q] = a.lastStats.pops; stats[5 * q + 1] = a.lastStats.nodes; stats[5 * q + 2] = a.lastStats.heapPeak;
                stats[5 * q + 3] = a.lastStats.rewrites; stats[5 * q + 4] = a.lastStats.pushed;
                len[q] = -1;
                if (ok) {
                    const std::vector<Eigen::Vector3d> p = a.getPath();
                    len[q] = (int)p.size();
                    if (len[q] <= path_cap)
                        for (size_t i = 0; i < p.size(); ++i)
                            for (int k = 0; k < 3; ++k) path[((size_t)q * path_cap + i) * 3 + k] = p[i](k);
                }
            }
            ++q;
        }
    }
    return q;
}

// min-snap through n_wp waypoints (xyz triples); corridor == NULL: equality-constrained only.  conds: [4][3] initial
// velocity, final velocity, initial acceleration, final acceleration (normalised-time derivatives, vigo_minsnap's
// layout); NULL = zeros.  coeffs_out: 3 * (n_wp-1) * (deg+1) doubles (x block, y block, z block), knots_out: n_wp doubles.
int vigo_host_minsnap_conds(int n_wp, const double* wp, int deg, int diff, int cont, double vel, const double* corridor,
                            double corridor_res, const double* conds, double* coeffs_out, double* knots_out) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n_wp; ++i) path.push_back(trajPlanner::pose(wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]));
    trajPlanner::polyTrajSolver s(deg, diff, cont, vel);
    s.updatePath(path);
    if (conds) {
        s.updateInitVel(conds[0], conds[1], conds[2]);
        s.updateEndVel(conds[3], conds[4], conds[5]);
        s.updateInitAcc(conds[6], conds[7], conds[8]);
        s.updateEndAcc(conds[9], conds[10], conds[11]);
    }
    if (corridor) s.setCorridorConstraint(std::vector<double>(corridor, corridor + n_wp - 1), corridor_res);
    if (!s.solve()) return -1;
    const int n = (n_wp - 1) * (deg + 1);
    for (int a = 0; a < 3; ++a) std::memcpy(coeffs_out + (size_t)a * n, s.getSolution(a).data(), sizeof(double) * n);
    std::memcpy(knots_out, s.getTimeKnot().data(), sizeof(double) * n_wp);
    return 0;
}

int vigo_host_minsnap(int n_wp, const double* wp, int deg, int diff, int cont, double vel, const double* corridor,
                      double corridor_res, double* coeffs_out, double* knots_out) {
    return vigo_host_minsnap_conds(n_wp, wp, deg, diff, cont, vel, corridor, corridor_res, nullptr, coeffs_out, knots_out);
}

// trajPlanner::pwlTraj over n_wp poses (x, y, z, yaw): updatePath(path[, desired_vel], use_yaw), makePlan(traj, delT).
// desired_vel <= 0: the class default.  traj_out: up to cap poses (x, y, z, yaw); knots_out: up to 2 n_wp doubles.
// Returns the number of trajectory poses, *n_knots the number of time knots; -2 when traj_out is too small.
int vigo_host_pwl(int n_wp, const double* wp, int use_yaw, double desired_vel, double delT, double* traj_out, int cap, double* knots_out,
                  int* n_knots) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n_wp; ++i) path.push_back(trajPlanner::pose(wp[4 * i], wp[4 * i + 1], wp[4 * i + 2], wp[4 * i + 3]));
    ros::NodeHandle nh;
    trajPlanner::pwlTraj pw(nh);
    if (desired_vel > 0) pw.updatePath(path, desired_vel, use_yaw != 0);
    else pw.updatePath(path, use_yaw != 0);
    std::vector<trajPlanner::pose> traj;
    pw.makePlan(traj, delT);
    const std::vector<double> k = pw.getTimeKnot();
    *n_knots = (int)k.size();
    for (size_t i = 0; i < k.size(); ++i) knots_out[i] = k[i];
    if ((int)traj.size() > cap) return -2;
    for (size_t i = 0; i < traj.size(); ++i) { traj_out[4 * i] = traj[i].x; traj_out[4 * i + 1] = traj[i].y; traj_out[4 * i + 2] = traj[i].z; traj_out[4 * i + 3] = traj[i].yaw; }
    return (int)traj.size();
}

// min-snap with SOFT interior waypoints (polyTrajSolver::setSoftConstraint, PS.cpp:943-958): soft[3] = half sizes per axis
int vigo_host_minsnap_soft(int n_wp, const double* wp, int deg, int diff, int cont, double vel, const double* soft,
                           double* coeffs_out, double* knots_out) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n_wp; ++i) path.push_back(trajPlanner::pose(wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]));
    trajPlanner::polyTrajSolver s(deg, diff, cont, vel);
    s.updatePath(path);
    s.setSoftConstraint(soft[0], soft[1], soft[2]);
    if (!s.solve()) return -1;
    const int n = (n_wp - 1) * (deg + 1);
    for (int a = 0; a < 3; ++a) std::memcpy(coeffs_out + (size_t)a * n, s.getSolution(a).data(), sizeof(double) * n);
    std::memcpy(knots_out, s.getTimeKnot().data(), sizeof(double) * n_wp);
    return 0;
}

// corridors, soft waypoint boxes and end conditions together, in polyTrajOccMap's call order (setCorridorConstraint,
// then setSoftConstraint, PM.cpp:356-358): corridor / soft[3] / conds may each be NULL (not set); outputs as
// vigo_host_minsnap_conds, knots always, an axis's coefficients only when its QP was solved.  Returns the mask of the
// solved axes (bit a = axis a; 7 = all): solve() keeps the stale polynomial of an axis that fails, per axis.
int vigo_host_minsnap_full(int n_wp, const double* wp, int deg, int diff, int cont, double vel, const double* corridor,
                           double corridor_res, const double* soft, const double* conds, double* coeffs_out, double* knots_out) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n_wp; ++i) path.push_back(trajPlanner::pose(wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]));
    trajPlanner::polyTrajSolver s(deg, diff, cont, vel);
    s.updatePath(path);
    if (conds) {
        s.updateInitVel(conds[0], conds[1], conds[2]);
        s.updateEndVel(conds[3], conds[4], conds[5]);
        s.updateInitAcc(conds[6], conds[7], conds[8]);
        s.updateEndAcc(conds[9], conds[10], conds[11]);
    }
    if (corridor) s.setCorridorConstraint(std::vector<double>(corridor, corridor + n_wp - 1), corridor_res);
    if (soft) s.setSoftConstraint(soft[0], soft[1], soft[2]);
    std::memcpy(knots_out, s.getTimeKnot().data(), sizeof(double) * n_wp);
    s.solve();
    const size_t n = (size_t)(n_wp - 1) * (deg + 1);
    int mask = 0;
    for (int a = 0; a < 3; ++a)
        if (s.getSolution(a).size() == n) {
            std::memcpy(coeffs_out + a * n, s.getSolution(a).data(), sizeof(double) * n);
            mask |= 1 << a;
        }
    return mask;
}

// the same solve, then polyTrajSolver::getPose / getVel / getAcc at n_t times: out[n_t][9] = position, velocity, acceleration
int vigo_host_minsnap_eval(int n_wp, const double* wp, int deg, int diff, int cont, double vel, int n_t, const double* t,
                           double* out) {
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n_wp; ++i) path.push_back(trajPlanner::pose(wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]));
    trajPlanner::polyTrajSolver s(deg, diff, cont, vel);
    s.updatePath(path);
    if (!s.solve()) return -1;
    for (int k = 0; k < n_t; ++k) {
        const trajPlanner::pose p = s.getPose(t[k]);
        const Eigen::Vector3d v = s.getVel(t[k]), a = s.getAcc(t[k]);
        double* o = out + 9 * (size_t)k;
        o[0] = p.x; o[1] = p.y; o[2] = p.z;
        for (int q = 0; q < 3; ++q) { o[3 + q] = v(q); o[6 + q] = a(q); }
    }
    return 0;
}

// polyTrajSolver's accessors on GIVEN coefficients (no QP): updatePath(wp) at velocity vel gives the knots (knots_out,
// n_wp doubles), installSolution takes coeffs (3 blocks of (n_wp-1)(deg+1), un-normalised local time), then getPose /
// getPos / getVel / getAcc at n_t times: out[n_t][13] = pose x, y, z, yaw, position, velocity, acceleration, and
// getTrajectory(traj, delT) into traj_out (first cap poses x, y, z, yaw; delT <= 0: not sampled).  Returns the number of
// trajectory poses.
int vigo_host_poly_eval(int n_wp, const double* wp, int deg, double vel, const double* coeffs, int n_t, const double* t, double* out,
                        double* knots_out, double delT, double* traj_out, int cap) {
    if (n_wp < 2 || !wp || deg < 0 || !coeffs || n_t < 0 || (n_t > 0 && (!t || !out)) || !knots_out) return -1;
    std::vector<trajPlanner::pose> path;
    for (int i = 0; i < n_wp; ++i) path.push_back(trajPlanner::pose(wp[3 * i], wp[3 * i + 1], wp[3 * i + 2]));
    trajPlanner::polyTrajSolver s(deg, 4, 4, vel);
    s.updatePath(path);
    const size_t n = (size_t)(n_wp - 1) * (deg + 1);
    s.installSolution(std::vector<double>(coeffs, coeffs + n), std::vector<double>(coeffs + n, coeffs + 2 * n),
                      std::vector<double>(coeffs + 2 * n, coeffs + 3 * n));
    std::memcpy(knots_out, s.getTimeKnot().data(), sizeof(double) * n_wp);
    for (int k = 0; k < n_t; ++k) {
        const trajPlanner::pose p = s.getPose(t[k]);
        const Eigen::Vector3d x = s.getPos(t[k]), v = s.getVel(t[k]), a = s.getAcc(t[k]);
        double* o = out + 13 * (size_t)k;
        o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = p.yaw;
        for (int q = 0; q < 3; ++q) { o[4 + q] = x(q); o[7 + q] = v(q); o[10 + q] = a(q); }
    }
    if (!(delT > 0) || !traj_out) return 0;
    std::vector<trajPlanner::pose> traj;
    s.getTrajectory(traj, delT);
    for (size_t i = 0; i < traj.size() && (int)i < cap; ++i) {
        traj_out[4 * i] = traj[i].x; traj_out[4 * i + 1] = traj[i].y; traj_out[4 * i + 2] = traj[i].z; traj_out[4 * i + 3] = traj[i].yaw;
    }
    return (int)traj.size();
}

// BASELINE configs[0]: one polyTrajOctomap::makePlan() (cfg/planner_interactive.yaml values passed in
// `cfg`: box[3], map_resolution, sample_delta_time, desired_velocity, initial_radius, shrinking_factor,
// corridor_res, maximum_iteration_num, traj_timeout, mode) on a dense byte grid (vigo.h voxel
// contract).  traj_out: up to traj_cap xyz triples.  info_out: valid, iterations, samples, duration,
// seconds of makePlan.  Needs the GPU (the box sweep of every sample runs there); -1 on failure.
int vigo_host_poly_plan(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int n_wp,
                        const double* wp, const double* cfg, double* traj_out, int traj_cap, double* info_out) {
    auto p = makePolyPlanner(denseMap(nx, ny, nz, origin, res, voxels), cfg, cfg[11], 4, 4, posesFromXyz(wp, n_wp));
    trajPlanner::polyTrajOctomap& planner = *p;
    std::vector<trajPlanner::pose> traj;
    if (planner.checkCollision(planner.getPath().front())) { /* first device call: creates the handle, snapshots the map */ }
    const auto t0 = std::chrono::steady_clock::now();
    planner.makePlan(traj, cfg[4]);
    const double secs = secondsSince(t0);
    copyXyz(traj, traj_cap, traj_out);
    info_out[0] = planner.isValid() ? 1.0 : 0.0;
    info_out[1] = planner.getIterations();
    info_out[2] = (double)traj.size();
    info_out[3] = planner.getDuration();
    info_out[4] = secs;
    return 0;
}

// polyTrajOctomap::makePlanBatch of P planners on one map, and for comparison each planner's twin planned alone with
// makePlan(): cfg as vigo_host_poly_plan (its `mode` entry is replaced by mode[i]); path i is wp[wp_off[i] ..
// wp_off[i+1]) (xyz triples).  Per planner (batch, then solo): info[4] = valid, iterations, final path length (waypoints),
// samples; traj [P][traj_cap][3] (first traj_cap samples).  secs_out[2]: seconds of makePlanBatch, of the P solo plans.
// solo_traj / solo_info / secs_out may be NULL (no twins then).  diff / cont: differential_degree / continuity_degree of
// every planner.  -1 on bad arguments.
int vigo_host_poly_plan_batch_ex(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P,
                                 const int32_t* wp_off, const double* wp, const double* cfg, const int32_t* mode, int diff, int cont,
                                 int traj_cap, double* traj_out, double* info_out, double* solo_traj_out, double* solo_info_out,
                                 double* secs_out) {
    if (P < 0 || !wp_off || !wp || !cfg || !mode || traj_cap < 0 || !traj_out || !info_out) return -1;
    typedef trajPlanner::polyTrajOctomap Planner;
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    batchThenSoloTwins(
        P, solo_traj_out && solo_info_out, secs_out,
        [&](int i) { return makePolyPlanner(map, cfg, (double)mode[i], diff, cont, posesFromXyz(wp + 3 * (size_t)wp_off[i], wp_off[i + 1] - wp_off[i])); },
        [](Planner& p) { if (p.checkCollision(p.getPath().front())) { /* first device call: handle and map snapshot */ } },
        [](const std::vector<Planner*>& ps, std::vector<std::vector<trajPlanner::pose>>& trajs, std::vector<bool>& r) {
            r = Planner::makePlanBatch(ps, trajs);
        },
        [&](Planner& p, std::vector<trajPlanner::pose>& traj) { p.makePlan(traj, cfg[4]); return p.isValid(); },
        [&](Planner& p, bool, const std::vector<trajPlanner::pose>& traj, int i, bool solo) {
            double* info = (solo ? solo_info_out : info_out) + 4 * (size_t)i;
            copyXyz(traj, traj_cap, (solo ? solo_traj_out : traj_out) + (size_t)i * traj_cap * 3);
            info[0] = p.isValid() ? 1.0 : 0.0;
            info[1] = p.getIterations();
            info[2] = (double)p.getPath().size();
            info[3] = (double)traj.size();
        });
    return 0;
}

int vigo_host_poly_plan_batch(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P,
                              const int32_t* wp_off, const double* wp, const double* cfg, const int32_t* mode, int traj_cap,
                              double* traj_out, double* info_out, double* solo_traj_out, double* solo_info_out, double* secs_out) {
    return vigo_host_poly_plan_batch_ex(nx, ny, nz, origin, res, voxels, P, wp_off, wp, cfg, mode, 4, 4, traj_cap, traj_out, info_out,
                                        solo_traj_out, solo_info_out, secs_out);
}

// ---- trajPlanner::polyTrajOccMap (bspline_node's seed planner) ----
// cfg[16]: the poly_traj/ keys in PM.cpp's order — polynomial_degree, differential_degree, continuity_degree,
// desired_velocity, desired_acceleration, initial_radius, timeout, corridor_res, shrinking_factor, soft_constraint,
// constraint_radius, sample_delta_time, maximum_iteration_num, use_pwl_failsafe — then the arguments of
// updateDesiredVel and updateDesiredAcc calls made after construction.  NaN: the key is not set (PM.cpp's default) /
// the call is not made.  conds: [4][3] start vel, end vel, start acc, end acc through updatePath(path, conditions), or
// NULL (the defaults, zero).
static std::unique_ptr<trajPlanner::polyTrajOccMap> makeOccPlanner(const std::shared_ptr<mapManager::occMap>& map, const double* cfg,
                                                                    int n_wp, const double* wp, const double* conds) {
    static const char* keys[14] = {"polynomial_degree", "differential_degree", "continuity_degree", "desired_velocity",
                                   "desired_acceleration", "initial_radius", "timeout", "corridor_res", "shrinking_factor",
                                   "soft_constraint", "constraint_radius", "sample_delta_time", "maximum_iteration_num",
                                   "use_pwl_failsafe"};
    ros::NodeHandle nh;
    for (int k = 0; k < 14; ++k)
        if (!std::isnan(cfg[k])) nh.setParam(std::string("poly_traj/") + keys[k], cfg[k]);
    std::unique_ptr<trajPlanner::polyTrajOccMap> p(new trajPlanner::polyTrajOccMap(nh));
    p->setMap(map);
    if (!std::isnan(cfg[14])) p->updateDesiredVel(cfg[14]);
    if (!std::isnan(cfg[15])) p->updateDesiredAcc(cfg[15]);
    const nav_msgs::Path path = pathFromXyz(wp, n_wp);
    if (conds) {
        std::vector<Eigen::Vector3d> c;
        for (int k = 0; k < 4; ++k) c.push_back(Eigen::Vector3d(conds[3 * k], conds[3 * k + 1], conds[3 * k + 2]));
        p->updatePath(path, c);
    } else {
        p->updatePath(path);
    }
    return p;
}

// One polyTrajOccMap on a dense byte grid, planned alone on the host (no GPU).  mode 1: makePlan(trajectory, true),
// 0: makePlan(trajectory, false), 2: makePlan(trajectory) (no bool).  traj_out: the first traj_cap samples (xyz);
// gt_dt > 0: getTrajectory(gt_dt) afterwards into gt_out (first traj_cap poses).  info_out[8]: makePlan's result,
// iterations (QP solves), samples, getDuration(), seconds of makePlan, getTrajectory poses, getPos(getDuration()) x / y.
int vigo_host_occ_plan(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int n_wp,
                       const double* wp, const double* cfg, const double* conds, int mode, int traj_cap, double* traj_out,
                       double gt_dt, double* gt_out, double* info_out) {
    if (n_wp < 0 || (n_wp > 0 && !wp) || !cfg || traj_cap < 0 || (traj_cap > 0 && !traj_out) || !info_out) return -1;
    auto p = makeOccPlanner(denseMap(nx, ny, nz, origin, res, voxels), cfg, n_wp, wp, conds);
    std::vector<trajPlanner::pose> traj;
    const auto t0 = std::chrono::steady_clock::now();
    const bool r = mode == 2 ? p->makePlan(traj) : p->makePlan(traj, mode != 0);
    info_out[4] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    copyXyz(traj, traj_cap, traj_out);
    info_out[0] = r ? 1.0 : 0.0;
    info_out[1] = p->getIterations();
    info_out[2] = (double)traj.size();
    info_out[3] = p->getDuration();
    info_out[5] = 0.0;
    if (gt_dt > 0 && gt_out) {
        const nav_msgs::Path g = p->getTrajectory(gt_dt);
        info_out[5] = (double)g.poses.size();
        copyXyz(g, traj_cap, gt_out);
    }
    const Eigen::Vector3d e = p->getPos(p->getDuration());
    info_out[6] = e(0);
    info_out[7] = e(1);
    return 0;
}

// The same plan, then the planner's accessors at n_t times: out[n_t][16] = getPose's position (3) and orientation
// (x, y, z, w), getPos, getVel, getAcc — through polyTrajOccMap's clamp to getDuration() and its switch to the PWL when
// use_pwl_failsafe is set and no plan was valid.  Returns makePlan's result (0 / 1), -1 on bad arguments.
int vigo_host_occ_plan_eval(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int n_wp,
                            const double* wp, const double* cfg, const double* conds, int mode, int n_t, const double* t, double* out) {
    if (n_wp < 2 || !wp || !cfg || n_t < 0 || (n_t > 0 && (!t || !out))) return -1;
    auto p = makeOccPlanner(denseMap(nx, ny, nz, origin, res, voxels), cfg, n_wp, wp, conds);
    std::vector<trajPlanner::pose> traj;
    const bool r = mode == 2 ? p->makePlan(traj) : p->makePlan(traj, mode != 0);
    for (int k = 0; k < n_t; ++k) {
        double* o = out + 16 * (size_t)k;
        const geometry_msgs::PoseStamped ps = p->getPose(t[k]);
        o[0] = ps.pose.position.x; o[1] = ps.pose.position.y; o[2] = ps.pose.position.z;
        o[3] = ps.pose.orientation.x; o[4] = ps.pose.orientation.y; o[5] = ps.pose.orientation.z; o[6] = ps.pose.orientation.w;
        const Eigen::Vector3d x = p->getPos(t[k]), v = p->getVel(t[k]), a = p->getAcc(t[k]);
        for (int q = 0; q < 3; ++q) { o[7 + q] = x(q); o[10 + q] = v(q); o[13 + q] = a(q); }
    }
    return r ? 1 : 0;
}

// polyTrajOccMap::makePlanBatch of P planners on one map (path i = wp[wp_off[i] .. wp_off[i+1]), cfg [P][16] and conds
// [P][4][3] as vigo_host_occ_plan, conds may be NULL), and each planner's twin planned alone with makePlan(trajectory,
// corridor).  Per planner (batch, then solo): info[5] = verdict, iterations, samples, getDuration(), getPos(getDuration()).x;
// traj [P][traj_cap][3].  secs_out[2]: seconds of makePlanBatch, of the P solo plans.  solo_* / secs_out may be NULL.
int vigo_host_occ_plan_batch(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P,
                             const int32_t* wp_off, const double* wp, const double* cfg, const double* conds, int corridor,
                             int traj_cap, double* traj_out, double* info_out, double* solo_traj_out, double* solo_info_out,
                             double* secs_out) {
    if (P < 0 || !wp_off || !wp || !cfg || traj_cap < 0 || !traj_out || !info_out) return -1;
    typedef trajPlanner::polyTrajOccMap Planner;
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    batchThenSoloTwins(
        P, solo_traj_out && solo_info_out, secs_out,
        [&](int i) {
            return makeOccPlanner(map, cfg + 16 * (size_t)i, wp_off[i + 1] - wp_off[i], wp + 3 * (size_t)wp_off[i],
                                  conds ? conds + 12 * (size_t)i : nullptr);
        },
        [](Planner&) { /* the solo plan runs on the host, and the batch's handle is made inside its timed call */ },
        [&](const std::vector<Planner*>& ps, std::vector<std::vector<trajPlanner::pose>>& trajs, std::vector<bool>& r) {
            r = Planner::makePlanBatch(ps, corridor != 0, &trajs);
        },
        [&](Planner& p, std::vector<trajPlanner::pose>& traj) { return p.makePlan(traj, corridor != 0); },
        [&](Planner& p, bool r, const std::vector<trajPlanner::pose>& traj, int i, bool solo) {
            double* info = (solo ? solo_info_out : info_out) + 5 * (size_t)i;
            copyXyz(traj, traj_cap, (solo ? solo_traj_out : traj_out) + (size_t)i * traj_cap * 3);
            info[0] = r ? 1.0 : 0.0;
            info[1] = p.getIterations();
            info[2] = (double)traj.size();
            info[3] = p.getDuration();
            info[4] = p.getPos(p.getDuration())(0);
        });
    return 0;
}

// bspline_node's per-click sequence (src/bspline_node.cpp:317-378) for P start/goal pairs se[P][2][3] on one map: the
// polyTrajOccMap seeds (makePlanBatch(false), or each planner's makePlan(false) when solo), getTrajectory(dt) and the
// inputPathCheck search (dt from getInitTs(), x 0.8, at most 50 ms), then bsplineTraj::updatePathBatch and
// makePlanBatch (solo: updatePath and makePlan per planner).  poly_cfg[16] as vigo_host_occ_plan; bsp_cfg[6]:
// distance_threshold, min_height, max_height, max_obstacle_size[3] (bspline_traj/ keys), velocity and acceleration
// limits of both planners from poly_cfg's desired_velocity / desired_acceleration.  Outputs per pair: the seed
// (adjustedInputPolyTraj) seed_out[P][seed_cap][3] with seed_n[P] poses and seed_dt[P]; status[P] = 0 updatePath refused
// the seed, 1 updated but makePlan failed, 2 planned.
int vigo_host_occ_seed_chain(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P,
                             const double* se, const double* poly_cfg, const double* bsp_cfg, int solo, int seed_cap,
                             double* seed_out, int32_t* seed_n, double* seed_dt, int32_t* status) {
    if (P < 0 || !se || !poly_cfg || !bsp_cfg || seed_cap < 0 || !seed_out || !seed_n || !seed_dt || !status) return -1;
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    const double vel = std::isnan(poly_cfg[3]) ? 1.0 : poly_cfg[3], acc = std::isnan(poly_cfg[4]) ? 1.0 : poly_cfg[4];
    ros::NodeHandle bnh;
    setBsplineParams(bnh, bsp_cfg);
    bnh.setParam("bspline_traj/max_path_length", 1000.0);
    const std::vector<Eigen::Vector3d> cond(4, Eigen::Vector3d(0, 0, 0));
    std::vector<std::unique_ptr<trajPlanner::polyTrajOccMap>> polys;
    std::vector<std::unique_ptr<trajPlanner::bsplineTraj>> bsps;
    std::vector<trajPlanner::polyTrajOccMap*> pp;
    std::vector<trajPlanner::bsplineTraj*> bp;
    for (int i = 0; i < P; ++i) {
        double c[16];
        std::copy(poly_cfg, poly_cfg + 16, c);
        c[14] = vel;   // polyTraj->updateDesiredVel(desiredVel); updateDesiredAcc(desiredAcc) (bspline_node.cpp:223-224)
        c[15] = acc;
        const double zero[12] = {};
        polys.push_back(makeOccPlanner(map, c, 2, se + 6 * (size_t)i, zero));   // updatePath(waypointsMsg, startEndConditions)
        pp.push_back(polys.back().get());
        bsps.emplace_back(new trajPlanner::bsplineTraj(bnh));
        bsps.back()->setMap(map);
        bsps.back()->updateMaxVel(vel);
        bsps.back()->updateMaxAcc(acc);
        bp.push_back(bsps.back().get());
    }
    if (solo) for (auto* p : pp) p->makePlan(false);
    else trajPlanner::polyTrajOccMap::makePlanBatch(pp, false);
    std::vector<nav_msgs::Path> seeds(P);
    for (int i = 0; i < P; ++i) {
        double dt = bp[i]->getInitTs(), finalTime = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        while (ros::ok()) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= 0.05) break;
            const nav_msgs::Path input = pp[i]->getTrajectory(dt);
            if (bp[i]->inputPathCheck(input, seeds[i], dt, finalTime)) break;
            dt *= 0.8;
        }
        seed_dt[i] = dt;
        seed_n[i] = (int32_t)seeds[i].poses.size();
        copyXyz(seeds[i], seed_cap, seed_out + (size_t)i * seed_cap * 3);
    }
    std::vector<bool> up(P), planned(P, false);
    if (solo) {
        for (int i = 0; i < P; ++i) {
            up[i] = bp[i]->updatePath(seeds[i], cond);
            if (up[i]) planned[i] = bp[i]->makePlan();
        }
    } else {
        up = trajPlanner::bsplineTraj::updatePathBatch(bp, seeds, std::vector<std::vector<Eigen::Vector3d>>(P, cond));
        std::vector<trajPlanner::bsplineTraj*> ready;
        std::vector<int> idx;
        for (int i = 0; i < P; ++i) if (up[i]) { ready.push_back(bp[i]); idx.push_back(i); }
        const std::vector<bool> r = trajPlanner::bsplineTraj::makePlanBatch(ready);
        for (size_t k = 0; k < idx.size(); ++k) planned[idx[k]] = r[k];
    }
    for (int i = 0; i < P; ++i) status[i] = !up[i] ? 0 : planned[i] ? 2 : 1;
    return 0;
}

// The facade's own per-planner steps of the seed-path stage (bsplineTraj::seedSteps: getTrajectory(dt), the inputPathCheck
// search ending on max_tries, prepareFitPointsWith) for P waypoint paths (wp_off CSR over wp) on one dense byte grid, each
// polyTrajOccMap planned alone on the host with makePlan(false): no GPU.  poly_cfg[16] / bsp_cfg[6] as
// vigo_host_occ_seed_chain; dt0[i] <= 0: getInitTs().  Per planner the polynomial the steps sampled — out_K segments,
// out_knots[seg_cap + 1], out_coeffs[seg_cap][3][8] (vigo_traj_point_check's layout), out_duration, out_dt0 — and the
// steps' results: out_flags[4] = found, tries, prepareFitPointsWith's verdict, whether it reached adjustPathLengthDirect;
// out_vals[5] = dt, finalTime, previous path length after the search, after updatePath's head, control_point_distance;
// the seed and the curve-fit points ([point_cap][3] rows each).  Returns 0, -1 for a bad argument, -2 when a list does
// not fit its capacity.
int vigo_host_seed_steps(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P, const int32_t* wp_off,
                         const double* wp, const double* poly_cfg, const double* bsp_cfg, double max_path_length, const double* dt0,
                         const double* prev_seed, const double* prev_fit, int max_tries, int seg_cap, int32_t* out_K, double* out_knots,
                         double* out_coeffs, double* out_duration, double* out_dt0, int point_cap, int32_t* out_flags, double* out_vals,
                         int32_t* out_seed_n, double* out_seed, int32_t* out_fit_n, double* out_fit) {
    if (P < 0 || !wp_off || !wp || !poly_cfg || !bsp_cfg || !dt0 || !prev_seed || !prev_fit || max_tries < 1 || seg_cap < 1 || point_cap < 0 ||
        !out_K || !out_knots || !out_coeffs || !out_duration || !out_dt0 || !out_flags || !out_vals || !out_seed_n || !out_seed || !out_fit_n || !out_fit)
        return -1;
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    const double vel = std::isnan(poly_cfg[3]) ? 1.0 : poly_cfg[3], acc = std::isnan(poly_cfg[4]) ? 1.0 : poly_cfg[4];
    ros::NodeHandle bnh;
    setBsplineParams(bnh, bsp_cfg);
    bnh.setParam("bspline_traj/max_path_length", max_path_length);
    int rc = 0;
    for (int i = 0; i < P; ++i) {
        double c[16];
        std::copy(poly_cfg, poly_cfg + 16, c);
        c[14] = vel;
        c[15] = acc;
        const double zero[12] = {};
        auto poly = makeOccPlanner(map, c, wp_off[i + 1] - wp_off[i], wp + 3 * (size_t)wp_off[i], zero);
        poly->makePlan(false);
        trajPlanner::bsplineTraj bsp(bnh);
        bsp.setMap(map);
        bsp.updateMaxVel(vel);
        bsp.updateMaxAcc(acc);
        const trajPlanner::polyTrajSolver* sol = poly->getSolver();
        const int deg = sol ? sol->getPolyDegree() : 7;
        const int K = sol && sol->hasSolution() ? (int)sol->timeKnots().size() - 1 : 0;
        if (K > seg_cap || deg != 7) { rc = -2; out_K[i] = 0; continue; }
        out_K[i] = K;
        for (int k = 0; k <= K && K > 0; ++k) out_knots[(size_t)i * (seg_cap + 1) + k] = sol->timeKnots()[k];
        for (int sg = 0; sg < K; ++sg)
            for (int ax = 0; ax < 3; ++ax)
                for (int d = 0; d < 8; ++d) out_coeffs[(((size_t)i * seg_cap + sg) * 3 + ax) * 8 + d] = sol->getSolution(ax)[(size_t)sg * 8 + d];
        out_duration[i] = poly->getDuration();
        out_dt0[i] = dt0[i] > 0.0 ? dt0[i] : bsp.getInitTs();
        trajPlanner::bsplineTraj::SeedSteps st;
        bsp.seedSteps(*poly, out_dt0[i], max_tries, prev_seed[i], prev_fit[i], st);
        int32_t* f = out_flags + 4 * (size_t)i;
        double* v = out_vals + 5 * (size_t)i;
        f[0] = st.search.found ? 1 : 0; f[1] = st.search.tries; f[2] = st.fitOk ? 1 : 0; f[3] = st.fitWrote ? 1 : 0;
        v[0] = st.search.dt; v[1] = st.search.finalTime; v[2] = st.search.prevOut; v[3] = st.prevFitOut; v[4] = bsp.getControlPointDist();
        out_seed_n[i] = (int32_t)st.seed.poses.size();
        out_fit_n[i] = (int32_t)st.fitPoints.size();
        if (out_seed_n[i] > point_cap || out_fit_n[i] > point_cap) { rc = -2; continue; }
        copyXyz(st.seed, point_cap, out_seed + (size_t)i * point_cap * 3);
        for (int k = 0; k < out_fit_n[i]; ++k)
            for (int a = 0; a < 3; ++a) out_fit[((size_t)i * point_cap + k) * 3 + a] = st.fitPoints[k](a);
    }
    return rc;
}

// bspline_node's per-click sequence for P start/goal pairs as vigo_host_occ_seed_chain, through the batched stage:
// polyTrajOccMap::makePlanBatch(false), bsplineTraj::seedPathBatch under setDeviceSeed(device != 0) and makePlanBatch —
// or, serial != 0, one planner after another in the reference's order with the public steps (every planner's
// getTrajectory / inputPathCheck search ending on the try count, then every planner's updatePath and makePlan).
// max_len[P]: each bsplineTraj's max_path_length; kind[P] (may be NULL): 0 plain, 1 the bsplineTraj is bound to a HIP
// device that does not exist (no handle, no snapshot), 2 the polyTrajOccMap has use_pwl_failsafe set and is never
// planned (it flies the PWL fallback's duration).  prev0: the previous path length the batch starts from.  Outputs
// per pair: seed_out[seed_cap][3] with seed_n, seed_dt, seed_tries; status as vigo_host_occ_seed_chain; ctrl_n control
// points in ctrl_out[ctrl_cap][3] as updatePath left them (before makePlan); totals[2]: the planners the launch /
// the host steps decided; out_K / out_knots[seg_cap + 1] / out_coeffs[seg_cap][3][8] / out_duration (all four or none):
// the polynomial each seed was sampled from, as vigo_host_seed_steps returns it.
int vigo_host_seed_batch(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P, const double* se,
                         const double* poly_cfg, const double* bsp_cfg, const double* max_len, const int32_t* kind, double prev0, int device,
                         int serial, int max_tries, int seed_cap, double* seed_out, int32_t* seed_n, double* seed_dt, int32_t* seed_tries,
                         int32_t* status, int ctrl_cap, double* ctrl_out, int32_t* ctrl_n, long long* totals, int seg_cap, int32_t* out_K,
                         double* out_knots, double* out_coeffs, double* out_duration) {
    if (P < 0 || !se || !poly_cfg || !bsp_cfg || !max_len || seed_cap < 0 || !seed_out || !seed_n || !seed_dt || !seed_tries || !status ||
        ctrl_cap < 0 || !ctrl_out || !ctrl_n || max_tries < 1)
        return -1;
    using trajPlanner::bsplineTraj;
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    const double vel = std::isnan(poly_cfg[3]) ? 1.0 : poly_cfg[3], acc = std::isnan(poly_cfg[4]) ? 1.0 : poly_cfg[4];
    const std::vector<Eigen::Vector3d> cond(4, Eigen::Vector3d(0, 0, 0));
    std::vector<std::unique_ptr<trajPlanner::polyTrajOccMap>> polys;
    std::vector<std::unique_ptr<bsplineTraj>> bsps;
    std::vector<trajPlanner::polyTrajOccMap*> pp, planned_polys;
    std::vector<bsplineTraj*> bp;
    for (int i = 0; i < P; ++i) {
        const int k = kind ? kind[i] : 0;
        double c[16];
        std::copy(poly_cfg, poly_cfg + 16, c);
        c[14] = vel;
        c[15] = acc;
        if (k == 2) c[13] = 1.0;   // use_pwl_failsafe
        const double zero[12] = {};
        polys.push_back(makeOccPlanner(map, c, 2, se + 6 * (size_t)i, zero));
        pp.push_back(polys.back().get());
        if (k != 2) planned_polys.push_back(pp.back());
        ros::NodeHandle bnh;
        setBsplineParams(bnh, bsp_cfg);
        bnh.setParam("bspline_traj/max_path_length", max_len[i]);
        bsps.emplace_back(new bsplineTraj(bnh));
        bsps.back()->setMap(map);
        bsps.back()->updateMaxVel(vel);
        bsps.back()->updateMaxAcc(acc);
        if (k == 1) bsps.back()->setDevice(63);
        bp.push_back(bsps.back().get());
    }
    trajPlanner::polyTrajOccMap::makePlanBatch(planned_polys, false);
    if (out_K && out_knots && out_coeffs && out_duration)
        for (int i = 0; i < P; ++i) {
            const trajPlanner::polyTrajSolver* sol = pp[i]->getSolver();
            const int K = sol && sol->hasSolution() && sol->getPolyDegree() == 7 ? (int)sol->timeKnots().size() - 1 : 0;
            if (K > seg_cap) return -2;
            out_K[i] = K;
            out_duration[i] = pp[i]->getDuration();
            for (int k = 0; k <= K && K > 0; ++k) out_knots[(size_t)i * (seg_cap + 1) + k] = sol->timeKnots()[k];
            for (int sg = 0; sg < K; ++sg)
                for (int ax = 0; ax < 3; ++ax)
                    for (int d = 0; d < 8; ++d) out_coeffs[(((size_t)i * seg_cap + sg) * 3 + ax) * 8 + d] = sol->getSolution(ax)[(size_t)sg * 8 + d];
        }
    // the previous path length is process-wide: a one-point path through adjustPathLengthDirect leaves 0 there, a second
    // point prev0 away leaves prev0
    {
        std::vector<Eigen::Vector3d> two{Eigen::Vector3d(0, 0, 1), Eigen::Vector3d(prev0, 0, 1)}, out;
        if (P > 0) bp[0]->adjustPathLengthDirect(two, out);
    }
    std::vector<nav_msgs::Path> seeds(P);
    std::vector<bool> up(P, false), planned(P, false);
    bsplineTraj::BatchStats st;
    if (serial) {
        for (int i = 0; i < P; ++i) {
            double dt = bp[i]->getInitTs(), finalTime = 0.0;
            int tries = 0;
            while (tries < max_tries) {
                ++tries;
                const nav_msgs::Path input = pp[i]->getTrajectory(dt);
                if (bp[i]->inputPathCheck(input, seeds[i], dt, finalTime)) break;
                dt *= 0.8;
            }
            seed_dt[i] = dt;
            seed_tries[i] = tries;
        }
        for (int i = 0; i < P; ++i) up[i] = bp[i]->updatePath(seeds[i], cond);
    } else {
        // the process default (a test sets its mixedFit through vigo_host_set_mixed_fit) with this entry's own arguments
        bsplineTraj::BatchOptions o = bsplineTraj::defaultBatchOptions();
        o.deviceSeed = device != 0;
        o.seedMaxTries = max_tries;
        std::vector<bsplineTraj::SeedInfo> info;
        up = bsplineTraj::seedPathBatch(bp, pp, std::vector<std::vector<Eigen::Vector3d>>(P, cond), o, &st, &seeds, &info);
        for (int i = 0; i < P; ++i) { seed_dt[i] = info[i].dt; seed_tries[i] = info[i].tries; }
    }
    if (totals) { totals[0] = st.seedDecided; totals[1] = st.seedHost; }
    for (int i = 0; i < P; ++i) {
        seed_n[i] = (int32_t)seeds[i].poses.size();
        copyXyz(seeds[i], seed_cap, seed_out + (size_t)i * seed_cap * 3);
        ctrl_n[i] = 0;
        if (up[i]) {
            const Eigen::MatrixXd c = bp[i]->getControlPoints();
            ctrl_n[i] = (int32_t)c.cols();
            for (int q = 0; q < c.cols() && q < ctrl_cap; ++q)
                for (int a = 0; a < 3; ++a) ctrl_out[((size_t)i * ctrl_cap + q) * 3 + a] = c(a, q);
        }
    }
    std::vector<bsplineTraj*> ready;
    std::vector<int> idx;
    for (int i = 0; i < P; ++i) if (up[i]) { ready.push_back(bp[i]); idx.push_back(i); }
    const std::vector<bool> r = bsplineTraj::makePlanBatch(ready);
    for (size_t k = 0; k < idx.size(); ++k) planned[idx[k]] = r[k];
    for (int i = 0; i < P; ++i) status[i] = !up[i] ? 0 : planned[i] ? 2 : 1;
    return 0;
}

// bsplineTraj::setMixedFit, the process default, for the harness entries above and below (returns what it was): a test
// flips it around vigo_host_seed_batch, whose own arguments keep their meaning
int vigo_host_set_mixed_fit(int on) {
    const bool was = trajPlanner::bsplineTraj::mixedFit();
    trajPlanner::bsplineTraj::setMixedFit(on != 0);
    return was ? 1 : 0;
}

// Wall time of the seed-path stage up to installed control points for P start/goal pairs (planners built and the min-snap
// seeds planned once, before the clock): out_ms[reps][3], per repetition in this order
//   0  what existed before seedPathBatch: the searches as a serial loop on the calling thread, then updatePathBatch
//   1  seedPathBatch on the host workers (deviceSeed off)
//   2  seedPathBatch with the vigo_seed_paths launch (deviceSeed on)
// so that the three alternate.  totals[2]: the planners the launch / the host steps decided in the last repetition of 2.
int vigo_host_seed_timing(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, int P, const double* se,
                          const double* poly_cfg, const double* bsp_cfg, int max_tries, int reps, double* out_ms, long long* totals) {
    if (P < 0 || !se || !poly_cfg || !bsp_cfg || max_tries < 1 || reps < 1 || !out_ms) return -1;
    using trajPlanner::bsplineTraj;
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    const double vel = std::isnan(poly_cfg[3]) ? 1.0 : poly_cfg[3], acc = std::isnan(poly_cfg[4]) ? 1.0 : poly_cfg[4];
    ros::NodeHandle bnh;
    setBsplineParams(bnh, bsp_cfg);
    bnh.setParam("bspline_traj/max_path_length", 1000.0);
    const std::vector<std::vector<Eigen::Vector3d>> conds(P, std::vector<Eigen::Vector3d>(4, Eigen::Vector3d(0, 0, 0)));
    std::vector<std::unique_ptr<trajPlanner::polyTrajOccMap>> polys;
    std::vector<std::unique_ptr<bsplineTraj>> bsps;
    std::vector<trajPlanner::polyTrajOccMap*> pp;
    std::vector<bsplineTraj*> bp;
    for (int i = 0; i < P; ++i) {
        double c[16];
        std::copy(poly_cfg, poly_cfg + 16, c);
        c[14] = vel;
        c[15] = acc;
        const double zero[12] = {};
        polys.push_back(makeOccPlanner(map, c, 2, se + 6 * (size_t)i, zero));
        pp.push_back(polys.back().get());
        bsps.emplace_back(new bsplineTraj(bnh));
        bsps.back()->setMap(map);
        bsps.back()->updateMaxVel(vel);
        bsps.back()->updateMaxAcc(acc);
        bp.push_back(bsps.back().get());
    }
    trajPlanner::polyTrajOccMap::makePlanBatch(pp, false);
    bsplineTraj::BatchOptions o = bsplineTraj::defaultBatchOptions();     // (mixedFit as vigo_host_set_mixed_fit left it)
    o.seedMaxTries = max_tries;
    for (int r = 0; r < reps; ++r)
        for (int mode = 0; mode < 3; ++mode) {
            bsplineTraj::BatchStats st;
            const auto t0 = std::chrono::steady_clock::now();
            if (mode == 0) {
                std::vector<nav_msgs::Path> seeds(P);
                for (int i = 0; i < P; ++i) {
                    double dt = bp[i]->getInitTs(), finalTime = 0.0;
                    for (int k = 0; k < max_tries; ++k) {
                        const nav_msgs::Path input = pp[i]->getTrajectory(dt);
                        if (bp[i]->inputPathCheck(input, seeds[i], dt, finalTime)) break;
                        dt *= 0.8;
                    }
                }
                (void)bsplineTraj::updatePathBatch(bp, seeds, conds);
            } else {
                o.deviceSeed = mode == 2;
                (void)bsplineTraj::seedPathBatch(bp, pp, conds, o, &st);
            }
            out_ms[3 * (size_t)r + mode] = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (mode == 2 && totals) { totals[0] = st.seedDecided; totals[1] = st.seedHost; }
        }
    return 0;
}

}  // extern "C"

// ---- the same prologue for MANY paths on ONE map (the workload generator of bench.py / tests: product code, no oracle) ----
namespace {
// planners parked between jobs: each owns an A* node pool sized by max_obstacle_size, shares the map
struct PlannerPool {
    std::shared_ptr<mapManager::occMap> map;
    ros::NodeHandle nh;
    std::mutex m;
    std::vector<std::unique_ptr<trajPlanner::bsplineTraj>> idle;
    std::unique_ptr<trajPlanner::bsplineTraj> take() {
        {
            std::lock_guard<std::mutex> lk(m);
            if (!idle.empty()) { auto p = std::move(idle.back()); idle.pop_back(); return p; }
        }
        std::unique_ptr<trajPlanner::bsplineTraj> p(new trajPlanner::bsplineTraj(nh));
        p->setMap(map);
        return p;
    }
    void give(std::unique_ptr<trajPlanner::bsplineTraj> p) {
        std::lock_guard<std::mutex> lk(m);
        idle.push_back(std::move(p));
    }
};

void initPool(PlannerPool& pool, const unsigned char* vox, const int* dims, const double* origin, double res, const double* cfg) {
    pool.map = denseMap(dims[0], dims[1], dims[2], origin, res, vox);
    setBsplineParams(pool.nh, cfg);
    pool.nh.setParam("bspline_traj/max_path_length", 1000.0);
}
}  // namespace

extern "C" {

// n paths of n_pts poses each (xyz) on one dense byte grid -> per path: status (0 planned, -1 updatePath refused the path or
// the control-point count is not N, -2 A* failed: no guides), N control points, the number of collision segments after
// pathSearch, and the guide pairs of makePlan()'s prologue (BT.cpp:333-350) as CSR over n * N control points:
// guide_off[n * N + 1], guide_pv[6 per pair] (at most cap_pairs; -2 is returned when they do not fit).
// ctrl_in != NULL: SKIP updatePath and replay the host steps the rebound loop takes at failCount >= 4 (BT.cpp:640-648:
// findCollisionSeg -> pathSearch -> assignGuidePointsSemiCircle) on these CURRENT control points [n][N][3], starting from
// empty lists: the pairs returned are the ones that step would APPEND.  cfg as in vigo_host_bspline_prologue.
int vigo_host_bspline_guides_batch(const unsigned char* vox, const int* dims, const double* origin, double res, int n, int n_pts,
                                   const double* path_xyz, const double* ctrl_in, int N, const double* cfg, double* ctrl_out, int* status,
                                   int* n_seg, int* guide_off, double* guide_pv, long long cap_pairs) {
    if (n < 0 || N < 7 || (!path_xyz && !ctrl_in)) return -1;
    PlannerPool pool;
    initPool(pool, vox, dims, origin, res, cfg);
    std::vector<std::vector<int32_t>> off(n);     // per planner: N + 1 offsets of its own pairs
    std::vector<std::vector<double>> pv(n);
    vigo_host::parallelFor((size_t)n, [&](size_t t) {
        auto bt = pool.take();
        status[t] = 0;
        n_seg[t] = 0;
        off[t].assign(1, 0);
        bool have = true;
        if (ctrl_in) {
            Eigen::MatrixXd c(3, N);
            for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) c(k, i) = ctrl_in[((size_t)t * N + i) * 3 + k];
            bt->setControlPoints(c);
        } else {
            have = bt->updatePath(pathFromXyz(path_xyz + (size_t)t * n_pts * 3, n_pts), std::vector<Eigen::Vector3d>(4, Eigen::Vector3d(0, 0, 0))) && bt->getControlPoints().cols() == N;
        }
        if (!have) {
            status[t] = -1;
        } else {
            const Eigen::MatrixXd c = bt->getControlPoints();
            if (ctrl_out) for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) ctrl_out[((size_t)t * N + i) * 3 + k] = c(k, i);
            std::vector<std::pair<int, int>> seg;
            std::vector<std::vector<Eigen::Vector3d>> paths;
            bt->findCollisionSeg(c, seg);
            if (!bt->pathSearch(seg, paths)) {
                status[t] = -2;
            } else {
                bt->assignGuidePointsSemiCircle(paths, seg);
                n_seg[t] = (int)seg.size();
                vigo_host::appendGuides(bt->getOptData(), N, off[t], pv[t]);
            }
        }
        off[t].resize((size_t)N + 1, 0);              // (no pairs: the prologue did not get that far)
        pool.give(std::move(bt));
    });
    long long g = 0;
    for (int t = 0; t < n; ++t) {
        for (int i = 0; i < N; ++i) guide_off[(size_t)t * N + i] = (int)(g + off[t][i]);
        g += off[t][N];
    }
    guide_off[(size_t)n * N] = (int)g;
    if (g > cap_pairs) return -2;
    long long w = 0;
    for (int t = 0; t < n; ++t) { std::memcpy(guide_pv + 6 * w, pv[t].data(), pv[t].size() * sizeof(double)); w += (long long)pv[t].size() / 6; }
    return 0;
}

}  // extern "C"

// ---- guide assignment: the device's core on the host, the facade's own step, and the workloads of their tests ----------
namespace {
struct NudgedAtan2 {     // std::atan2 moved by `ulps` representable values (test-only neighbours of libm's result)
    int ulps;
    double operator()(double y, double x) const {
        double r = std::atan2(y, x);
        for (int k = 0; k < std::abs(ulps); ++k) r = std::nextafter(r, ulps > 0 ? HUGE_VAL : -HUGE_VAL);
        return r;
    }
};
}  // namespace

extern "C" {

// out[i] = vigo_atan2(y[i], x[i]) (csrc/vigo_guide_core.hpp)
int vigo_host_atan2(long long n, const double* y, const double* x, double* out) {
    if (n < 0 || (n > 0 && (!y || !x || !out))) return -1;
    for (long long i = 0; i < n; ++i) out[i] = vigo::vigo_atan2(y[i], x[i]);
    return 0;
}

// vigo_guide_assign on the host (csrc/vigo_guide_core.hpp) on a dense byte grid (bit 0 = inflated-occupied, bit 1 =
// unknown; outside the grid both), inputs and outputs as the device entry.  mode 0: std::atan2 (the facade's
// arithmetic); 1: vigo_atan2 (the device's twin); 2 / 3: std::atan2 nudged by +2 / -2 ulp (test-only neighbours).
// path_cap: a trajectory with a longer path is DEFERRED (the device's rule with vigo_guide_capacity's value).
// out_decision int32[pair_cap][3] or NULL: per pair the search's found flag, path segment and bisection step.
// Returns 0; -1 for what the device entry answers with VIGO_ERR_INVALID_ARG (nothing is written).
int vigo_host_guide_core(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                         const int* seg_off, const int* seg, const int* path_off, const double* path, int mode, int path_cap,
                         long long pair_cap, int* out_off, double* out_pv, unsigned char* out_unk, int* out_status, int* out_decision) {
    if (B < 0 || N < 1 || pair_cap < 0 || mode < 0 || mode > 3 || !(res > 0) ||
        (B > 0 && (!ctrl || !seg_off || !seg || !path_off || !path || !out_off || !out_pv || !out_status)))
        return -1;
    if (B == 0) return 0;
    if (seg_off[0] < 0) return -1;
    std::vector<uint8_t> deferred(B, 0);
    std::vector<long long> first_pair(B + 1, 0);
    size_t longest = 1;
    for (int b = 0; b < B; ++b) {
        if (seg_off[b + 1] < seg_off[b]) return -1;
        long long nb = 0;
        for (int k = seg_off[b]; k < seg_off[b + 1]; ++k) {
            const int len = path_off[k + 1] - path_off[k];
            if (path_off[k] < 0 || len < 0 || !vigo::guide_segment_ok(N, seg[2 * k], seg[2 * k + 1], len)) return -1;
            if (len > path_cap) deferred[b] = 1;
            longest = std::max(longest, (size_t)len);
            nb += vigo::guide_pushes_total(N, seg[2 * k], seg[2 * k + 1]);
        }
        first_pair[b + 1] = first_pair[b] + (deferred[b] ? 0 : nb);
    }
    if (first_pair[B] > pair_cap || first_pair[B] > 0x7fffffffLL) return -1;
    const DenseGrid occ{vox, dims, origin, res};
    vigo_host::parallelFor((size_t)B, [&](size_t b) {
        out_status[b] = deferred[b] ? vigo::kGuideDeferred : vigo::kGuideOk;
        const int s0 = seg_off[b], s1 = seg_off[b + 1];
        std::vector<int> cursor(N);
        long long at = first_pair[b];
        for (int i = 0; i < N; ++i) {
            out_off[b * (size_t)N + i] = (int)at;
            cursor[i] = (int)at;
            if (!deferred[b])
                for (int k = s0; k < s1; ++k) at += vigo::guide_pushes(N, seg[2 * k], seg[2 * k + 1], i);
        }
        if (deferred[b]) return;
        std::vector<vigo::G3> sc(longest);
        auto emit = [&](int idx, const vigo::G3& p, const vigo::G3& d, const int32_t* dec) {
            const int g = cursor[idx]++;
            for (int a = 0; a < 3; ++a) { out_pv[(size_t)g * 6 + a] = p.v[a]; out_pv[(size_t)g * 6 + 3 + a] = d.v[a]; }
            if (out_unk) out_unk[g] = (occ.byteAt(p.v[0], p.v[1], p.v[2]) >> 1) & 1u;
            if (out_decision) for (int a = 0; a < 3; ++a) out_decision[(size_t)g * 3 + a] = dec[a];
        };
        const double* c = ctrl + b * (size_t)N * 3;
        const int* sg = seg + 2 * (size_t)s0;
        const int* po = path_off + s0;
        // (the core indexes the paths from path_off[0] of the slice it is given: hand it the whole array and the slice's offsets)
        if (mode == 1) vigo::guide_assign(occ, vigo::GuideAtan2{}, res, N, c, s1 - s0, sg, po, path, sc.data(), emit);
        else if (mode == 0) vigo::guide_assign(occ, [](double y, double x) { return std::atan2(y, x); }, res, N, c, s1 - s0, sg, po, path, sc.data(), emit);
        else vigo::guide_assign(occ, NudgedAtan2{mode == 2 ? 2 : -2}, res, N, c, s1 - s0, sg, po, path, sc.data(), emit);
    });
    out_off[(size_t)B * N] = (int)first_pair[B];
    return 0;
}

// the FACADE's own step (bsplineTraj::assignGuidePointsSemiCircle) on the same inputs, one planner per trajectory with
// these control points and empty lists: offsets [B*N+1] and pairs as above.  Returns 0, -1 on a bad argument, -2 when
// the pairs do not fit pair_cap.
int vigo_host_guide_facade(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                           const int* seg_off, const int* seg, const int* path_off, const double* path, long long pair_cap, int* out_off,
                           double* out_pv) {
    if (B < 0 || N < 7 || !ctrl || !seg_off || !seg || !path_off || !path || !out_off || !out_pv) return -1;
    const double cfg[6] = {0.5, 0.7, 1.3, 5.0, 5.0, 3.0};      // (the step reads none of them)
    PlannerPool pool;
    initPool(pool, vox, dims, origin, res, cfg);
    std::vector<std::vector<int32_t>> off(B);
    std::vector<std::vector<double>> pv(B);
    vigo_host::parallelFor((size_t)B, [&](size_t b) {
        auto bt = pool.take();
        Eigen::MatrixXd c(3, N);
        for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) c(k, i) = ctrl[(b * N + i) * 3 + k];
        bt->setControlPoints(c);
        std::vector<std::pair<int, int>> sg;
        std::vector<std::vector<Eigen::Vector3d>> paths;
        for (int k = seg_off[b]; k < seg_off[b + 1]; ++k) {
            sg.push_back({seg[2 * k], seg[2 * k + 1]});
            paths.emplace_back();
            for (int q = path_off[k]; q < path_off[k + 1]; ++q) paths.back().push_back(Eigen::Vector3d(path[3 * (size_t)q], path[3 * (size_t)q + 1], path[3 * (size_t)q + 2]));
        }
        bt->assignGuidePointsSemiCircle(paths, sg);
        off[b].assign(1, 0);
        vigo_host::appendGuides(bt->getOptData(), N, off[b], pv[b]);
        pool.give(std::move(bt));
    });
    long long g = 0;
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < N; ++i) out_off[(size_t)b * N + i] = (int)(g + off[b][i]);
        g += off[b][N];
    }
    out_off[(size_t)B * N] = (int)g;
    if (g > pair_cap) return -2;
    long long w = 0;
    for (int b = 0; b < B; ++b) { std::memcpy(out_pv + 6 * w, pv[b].data(), pv[b].size() * sizeof(double)); w += (long long)pv[b].size() / 6; }
    return 0;
}

// What vigo_guide_assign is given in makePlan()'s prologue, by the host pipeline (findCollisionSeg -> pathSearch) for n
// sets of control points [n][N][3] on one dense byte grid: seg_off[n+1], seg[seg_cap][2] (after the merges, with the
// min(collisionSeg.size(), paths.size()) bound applied), path_off[seg_cap+1], path[pt_cap][3].  A trajectory whose A*
// fails has no segments (status[t] = -2, as vigo_host_bspline_guides_batch).  cfg as in vigo_host_bspline_prologue.
// Returns 0, -1 on a bad argument, -2 when a buffer is too small.
int vigo_host_prologue_paths(const unsigned char* vox, const int* dims, const double* origin, double res, int n, int N, const double* ctrl,
                             const double* cfg, int seg_cap, long long pt_cap, int* status, int* seg_off, int* seg, int* path_off,
                             double* path) {
    if (n < 0 || N < 7 || !ctrl || !cfg || !status || !seg_off || !seg || !path_off || !path) return -1;
    PlannerPool pool;
    initPool(pool, vox, dims, origin, res, cfg);
    std::vector<std::vector<std::pair<int, int>>> segs(n);
    std::vector<std::vector<std::vector<Eigen::Vector3d>>> paths(n);
    vigo_host::parallelFor((size_t)n, [&](size_t t) {
        auto bt = pool.take();
        Eigen::MatrixXd c(3, N);
        for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) c(k, i) = ctrl[(t * N + i) * 3 + k];
        bt->setControlPoints(c);
        status[t] = 0;
        bt->findCollisionSeg(c, segs[t]);
        if (!bt->pathSearch(segs[t], paths[t])) {
            status[t] = -2;
            segs[t].clear();
            paths[t].clear();
        }
        pool.give(std::move(bt));
    });
    long long s = 0, q = 0;
    seg_off[0] = 0;
    path_off[0] = 0;
    for (int t = 0; t < n; ++t) {
        const size_t m = std::min(segs[t].size(), paths[t].size());
        for (size_t k = 0; k < m; ++k) {
            if (s + 1 > seg_cap || q + (long long)paths[t][k].size() > pt_cap) return -2;
            seg[2 * s] = segs[t][k].first;
            seg[2 * s + 1] = segs[t][k].second;
            for (const auto& v : paths[t][k]) { for (int a = 0; a < 3; ++a) path[3 * q + a] = v(a); ++q; }
            ++s;
            path_off[s] = (int)q;
        }
        seg_off[t + 1] = (int)s;
    }
    return 0;
}

// vigo_collision_segs on the host (csrc/vigo_pathsearch_core.hpp) on a dense byte grid: outputs as the device entry.
// Returns 0; -1 for what the device entry answers with VIGO_ERR_INVALID_ARG (nothing is written).
int vigo_host_collision_segs_core(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                                  double not_check_ratio, long long seg_cap, int* out_seg_off, int* out_seg, int* out_status) {
    if (B < 0 || N < 7 || seg_cap < 0 || !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0) || !(res > 0) ||
        (B > 0 && (!ctrl || !out_seg_off || !out_seg || !out_status)))
        return -1;
    if (B == 0) return 0;
    const DenseGrid occ{vox, dims, origin, res};
    std::vector<std::vector<int32_t>> segs(B);
    vigo_host::parallelFor((size_t)B, [&](size_t b) {
        const double* c = ctrl + b * (size_t)N * 3;
        const auto [pt, ln] = ctrlFlags(occ, c);
        segs[b].resize(2 * vigo::kPathsMaxSegs);
        const int n = vigo::collision_segs(N, not_check_ratio, pt, ln, vigo::kPathsMaxSegs, segs[b].data());
        if (n > vigo::kPathsMaxSegs) segs[b].assign(1, -1);        // (marks the deferred ones)
        else segs[b].resize(2 * (size_t)n);
    });
    long long total = 0;
    for (int b = 0; b < B; ++b) total += segs[b].size() == 1 ? 0 : (long long)segs[b].size() / 2;
    if (total > seg_cap) return -1;
    long long s = 0;
    for (int b = 0; b < B; ++b) {
        out_seg_off[b] = (int)s;
        out_status[b] = segs[b].size() == 1 ? vigo::kPathsDeferred : vigo::kPathsOk;
        if (segs[b].size() == 1) continue;
        std::copy(segs[b].begin(), segs[b].end(), out_seg + 2 * s);
        s += (long long)segs[b].size() / 2;
    }
    out_seg_off[B] = (int)s;
    return 0;
}

// vigo_path_search on the host: csrc/vigo_pathsearch_core.hpp around vigo::astar_search (csrc/vigo_astar_core.hpp) with a
// table of 1 << cap_log2 slots holding at most max_nodes nodes and a heap of heap_cap entries (vigo_astar_capacity's
// values with cap_log2 = 13: the kernels' twin; large ones: no search is deferred for want of room).  Inputs and outputs
// as the device entry.  Returns 0; -1 for what the device entry answers with VIGO_ERR_INVALID_ARG or
// VIGO_ERR_UNSUPPORTED (nothing is written).
int vigo_host_path_search_core(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                               const int* seg_off, const int* seg, double not_check_ratio, double step, const int* pool, double min_height,
                               double max_height, int cap_log2, int max_nodes, int heap_cap, int max_expansions, int search_path_cap,
                               long long seg_cap, long long point_cap, int* out_status, int* out_seg_off, int* out_seg, int* out_path_off,
                               double* out_path, int* out_counts) {
    const bool scan = !seg_off && !seg;
    if (B < 0 || N < 7 || seg_cap < 0 || point_cap < 0 || (!scan && (!seg_off || !seg)) || (scan && !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0)) ||
        !pool || !(step > 0.0) || !(step < 1e300) || search_path_cap < 2 || max_expansions < 0 || !(res > 0) || cap_log2 < 1 || cap_log2 > 30 ||
        max_nodes < 1 || max_nodes >= (1 << cap_log2) || heap_cap < 1 ||
        (B > 0 && (!ctrl || !out_status || !out_seg_off || !out_seg || !out_path_off || !out_path)))
        return -1;
    for (int a = 0; a < 3; ++a)
        if (pool[a] < 3 || pool[a] > vigo::kAstarMaxPoolAxis) return -1;
    if (B == 0) return 0;
    if (!scan) {
        if (seg_off[0] < 0) return -1;
        for (int b = 0; b < B; ++b) {
            if (seg_off[b + 1] < seg_off[b]) return -1;
            if (seg_off[b + 1] - seg_off[b] > vigo::kPathsMaxSegs) continue;
            for (int k = seg_off[b]; k < seg_off[b + 1]; ++k)
                if (seg[2 * k] < 0 || seg[2 * k] >= N || seg[2 * k + 1] < 0 || seg[2 * k + 1] >= N) return -1;
        }
    }
    const DenseGrid occ{vox, dims, origin, res};
    struct Search { int status = vigo::kAstarDeferred, len = 0; std::vector<double> path; };
    struct Traj { int status = vigo::kPathsDeferred, run = 0, decided = 0; std::vector<int32_t> seg; std::vector<std::vector<double>> paths; };
    std::vector<Traj> out(B);
    const size_t slots = (size_t)1 << cap_log2;
    vigo_host::parallelFor((size_t)B, [&](size_t b) {
        static thread_local std::vector<int32_t> key, heap;
        static thread_local std::vector<double> g;
        static thread_local std::vector<uint8_t> meta;
        key.resize(slots); heap.resize((size_t)heap_cap); g.resize(slots); meta.resize(slots);
        const double* c = ctrl + b * (size_t)N * 3;
        Traj& T = out[b];
        std::vector<int32_t> in(2 * vigo::kPathsMaxSegs);
        int n;
        if (scan) {
            const auto [pt, ln] = ctrlFlags(occ, c);
            n = vigo::collision_segs(N, not_check_ratio, pt, ln, vigo::kPathsMaxSegs, in.data());
        } else {
            n = seg_off[b + 1] - seg_off[b];
            if (n <= vigo::kPathsMaxSegs) std::copy(seg + 2 * (size_t)seg_off[b], seg + 2 * (size_t)seg_off[b + 1], in.begin());
        }
        if (n > vigo::kPathsMaxSegs) return;                       // deferred, owns nothing
        auto search = [&](int first, int second) {
            Search r;
            r.path.resize((size_t)search_path_cap * 3);
            std::fill(key.begin(), key.end(), -1);
            vigo::AstarStore<int32_t> S{};
            S.key = key.data(); S.g = g.data(); S.meta = meta.data(); S.heap = heap.data();
            S.cap_log2 = cap_log2; S.max_nodes = max_nodes; S.heap_cap = heap_cap;
            r.status = vigo::astar_search(S, occ, c + 3 * (size_t)first, c + 3 * (size_t)second, step, pool, min_height, max_height, max_expansions,
                                          search_path_cap, r.path.data(), &r.len);
            ++T.run;
            T.decided += vigo::paths_search_decided(r.status) ? 1 : 0;
            return r;
        };
        std::vector<Search> s1(n), s2(n);
        for (int k = 0; k < n; ++k) s1[k] = search(in[2 * k], in[2 * k + 1]);
        vigo::retry_list(n, in.data(), [&](int k) { return s1[k].status; }, [&](int k) { s2[k] = search(in[2 * k], in[2 * (k + 1) + 1]); });
        std::vector<int32_t> mseg(2 * (size_t)n + 2), pick((size_t)n + 1);
        int n_out = 0;
        T.status = vigo::path_walk(n, in.data(), [&](int k) { return s1[k].status; }, [&](int k) { return s2[k].status; }, mseg.data(), pick.data(), &n_out);
        T.seg.assign(mseg.begin(), mseg.begin() + 2 * (size_t)n_out);
        for (int j = 0; j < n_out; ++j) {
            const int k = pick[j] & ~vigo::kPathsSecond;
            const bool second = (pick[j] & vigo::kPathsSecond) != 0;
            const Search& r = second ? s2[k] : s1[k];
            std::vector<double> p(r.path.begin(), r.path.begin() + 3 * (size_t)r.len);
            const double* first = c + 3 * (size_t)in[2 * k];
            const double* last = c + 3 * (size_t)in[2 * (second ? k + 1 : k) + 1];
            for (int a = 0; a < 3; ++a) p[a] = first[a];
            p.insert(p.end(), last, last + 3);
            T.paths.push_back(std::move(p));
        }
    });
    long long total_seg = 0, total_pts = 0;
    for (const Traj& T : out) {
        total_seg += (long long)T.seg.size() / 2;
        for (const auto& p : T.paths) total_pts += (long long)p.size() / 3;
    }
    if (total_seg > seg_cap || total_pts > point_cap || total_pts > 0x7fffffffLL) return -1;
    long long s = 0, q = 0;
    for (int b = 0; b < B; ++b) {
        const Traj& T = out[b];
        out_status[b] = T.status;
        out_seg_off[b] = (int)s;
        if (out_counts) { out_counts[2 * b] = T.run; out_counts[2 * b + 1] = T.decided; }
        for (size_t j = 0; j < T.paths.size(); ++j) {
            out_seg[2 * s] = T.seg[2 * j];
            out_seg[2 * s + 1] = T.seg[2 * j + 1];
            out_path_off[s] = (int)q;
            std::copy(T.paths[j].begin(), T.paths[j].end(), out_path + 3 * q);
            q += (long long)T.paths[j].size() / 3;
            ++s;
        }
    }
    out_seg_off[B] = (int)s;
    out_path_off[s] = (int)q;
    return 0;
}

}  // extern "C"

// ---- the re-guide step of the rebound loop: the device's rules on the host, and the facade's own step ---------------------
extern "C" {

// vigo_rebound_reguide on the host: csrc/vigo_reguide_core.hpp around vigo_host_path_search_core and
// vigo_host_guide_core on a dense byte grid, inputs and outputs as the device entry (dthresh: the handle's parameter
// there).  cap_log2 / max_nodes / heap_cap as vigo_host_path_search_core, guide_path_cap and mode as
// vigo_host_guide_core's path_cap and mode: with vigo_astar_capacity's and vigo_guide_capacity's values and mode 1 this
// is the kernels' bit-exact twin; with large ones and mode 0 it is the facade's arithmetic.  (More than
// VIGO_MAX_COLLISION_SEGS new segments are DEFERRED under every setting: the state does not hold them.)
// Returns 0; -1 for what the device entry answers with VIGO_ERR_INVALID_ARG / _UNSUPPORTED (nothing is written).
int vigo_host_rebound_reguide_core(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                                   const int* guide_off, const double* guide_pv, const unsigned char* guide_unk, double* weights,
                                   double not_check_ratio, double dthresh, double step, const int* pool, double min_height, double max_height,
                                   int cap_log2, int max_nodes, int heap_cap, int max_expansions, int search_path_cap, int guide_path_cap, int mode,
                                   vigo_rebound_state_t* state, long long pair_cap, int* out_guide_off, double* out_guide_pv,
                                   unsigned char* out_guide_unk, long long seg_cap, long long point_cap, int* out_path_seg_off, int* out_path_off,
                                   double* out_path, int* out_status) {
    const bool no_guides = !guide_off && !guide_pv && !guide_unk;
    const bool no_paths = !out_path_seg_off && !out_path_off && !out_path;
    if (B < 0 || N < 7 || N > VIGO_MAX_CTRL_POINTS || pair_cap < 0 || seg_cap < 0 || point_cap < 0 || !(not_check_ratio >= 0.0 && not_check_ratio <= 1.0) ||
        (!no_guides && (!guide_off || !guide_pv)) || (!no_paths && (!out_path_seg_off || !out_path_off || !out_path)) || !pool || !(step > 0.0) ||
        !(step < 1e300) || search_path_cap < 2 || max_expansions < 0 || !(res > 0) || mode < 0 || mode > 3 ||
        (B > 0 && (!ctrl || !weights || !state || !out_guide_off || !out_guide_pv || !out_status)))
        return -1;
    for (int a = 0; a < 3; ++a)
        if (pool[a] < 3 || pool[a] > vigo::kAstarMaxPoolAxis) return -1;
    if (B == 0) return 0;
    if (guide_off) {
        if (guide_off[0] < 0) return -1;
        for (size_t q = 0; q < (size_t)B * N; ++q)
            if (guide_off[q + 1] < guide_off[q]) return -1;
    }
    const DenseGrid occ{vox, dims, origin, res};
    constexpr int kSegs = VIGO_MAX_COLLISION_SEGS;
    // the rules: the new segments and the re-guide list of every trajectory that is worked on
    std::vector<int> kind(B), n_list(B, 0), n_new(B, 0);
    std::vector<int32_t> new_seg((size_t)B * 2 * kSegs), list((size_t)B * 2 * kSegs);
    vigo_host::parallelFor((size_t)B, [&](size_t b) {
        const vigo_rebound_state_t& st = state[b];
        if (!(st.status == VIGO_RB_NEEDS_HOST && st.gate_static != 0 && st.fail_count < 4)) { kind[b] = vigo::kReguideSkipped; return; }
        const double* c = ctrl + b * (size_t)N * 3;
        const auto [pt, ln] = ctrlFlags(occ, c);
        auto need_guide = [&](int i) {
            if (!guide_off || !guide_pv) return true;
            for (int j = guide_off[b * N + i]; j < guide_off[b * N + i + 1]; ++j)
                if (!vigo::reguide_guide_far(dthresh, c + 3 * i, guide_pv + 6 * (size_t)j)) return false;
            return true;
        };
        int32_t seg[2 * kSegs];
        uint8_t listed[kSegs];
        int m = 0;
        const int n_prev = std::min(std::max(st.n_seg, 0), kSegs);
        const int n = vigo::reguide_rules(N, not_check_ratio, pt, ln, n_prev, st.seg, need_guide, kSegs, seg, listed, &m);
        if (n > kSegs) { kind[b] = vigo::kReguideDeferred; return; }
        kind[b] = -1;
        n_new[b] = n;
        std::copy(seg, seg + 2 * n, new_seg.begin() + b * 2 * kSegs);
        int32_t* dst = list.data() + b * 2 * kSegs;
        for (int k = 0; k < n; ++k)
            if (listed[k]) { dst[2 * n_list[b]] = seg[2 * k]; dst[2 * n_list[b] + 1] = seg[2 * k + 1]; ++n_list[b]; }
    });
    // the path search on the lists, the guide step on its output
    std::vector<int> l_off(B + 1, 0), l_seg(2, 0);
    for (int b = 0; b < B; ++b) {
        l_off[b + 1] = l_off[b] + n_list[b];
        l_seg.insert(l_seg.end() - 2, list.begin() + (size_t)b * 2 * kSegs, list.begin() + (size_t)b * 2 * kSegs + 2 * n_list[b]);
    }
    const long long S = l_off[B], pts_room = S * ((long long)search_path_cap + 1);
    std::vector<int> ps_status(B), ps_seg_off(B + 1), ps_seg(2 * (size_t)S + 2), ps_path_off((size_t)S + 1), ps_counts(2 * (size_t)B);
    std::vector<double> ps_path(3 * (size_t)pts_room + 3);
    if (vigo_host_path_search_core(vox, dims, origin, res, B, N, ctrl, l_off.data(), l_seg.data(), not_check_ratio, step, pool, min_height, max_height,
                                   cap_log2, max_nodes, heap_cap, max_expansions, search_path_cap, S, pts_room, ps_status.data(), ps_seg_off.data(),
                                   ps_seg.data(), ps_path_off.data(), ps_path.data(), ps_counts.data()) != 0)
        return -1;
    const long long total_seg = ps_seg_off[B], total_pts = ps_path_off[total_seg];
    if (!no_paths && (total_seg > seg_cap || total_pts > point_cap)) return -1;
    long long pairs_room = 0;
    for (long long k = 0; k < total_seg; ++k) pairs_room += vigo::guide_pushes_total(N, ps_seg[2 * k], ps_seg[2 * k + 1]);
    std::vector<int> g_off((size_t)B * N + 1), g_status(B);
    std::vector<double> g_pv(6 * (size_t)pairs_room + 6);
    std::vector<unsigned char> g_unk((size_t)pairs_room + 1);
    if (vigo_host_guide_core(vox, dims, origin, res, B, N, ctrl, ps_seg_off.data(), ps_seg.data(), ps_path_off.data(), ps_path.data(), mode, guide_path_cap,
                             pairs_room, g_off.data(), g_pv.data(), g_unk.data(), g_status.data(), nullptr) != 0)
        return -1;
    // the outcomes and the merged offsets
    std::vector<int> outcome(B);
    long long total = 0;
    for (int b = 0; b < B; ++b) {
        const bool cut = ps_status[b] == vigo::kPathsOk && vigo::paths_cut_by_bound(ps_counts[2 * b], ps_seg_off[b + 1] - ps_seg_off[b]);
        outcome[b] = vigo::reguide_outcome(kind[b] != vigo::kReguideSkipped, kind[b] == vigo::kReguideDeferred, n_list[b], ps_status[b], cut,
                                           g_status[b] == vigo::kGuideDeferred);
        if (guide_off) total += guide_off[(size_t)(b + 1) * N] - guide_off[(size_t)b * N];
        if (outcome[b] == vigo::kReguideDone) total += g_off[(size_t)(b + 1) * N] - g_off[(size_t)b * N];
    }
    if (total > pair_cap || total > 0x7fffffffLL) return -1;
    long long at = 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < N; ++i) {
            const size_t q = (size_t)b * N + i;
            out_guide_off[q] = (int)at;
            auto put = [&](const double* src, unsigned unk) {
                std::copy(src, src + 6, out_guide_pv + 6 * at);
                if (out_guide_unk) out_guide_unk[at] = (unsigned char)unk;
                ++at;
            };
            if (guide_off)
                for (int j = guide_off[q]; j < guide_off[q + 1]; ++j) {
                    const double* src = guide_pv + 6 * (size_t)j;
                    put(src, guide_unk ? guide_unk[j] : ((occ.byteAt(src[0], src[1], src[2]) >> 1) & 1u));
                }
            if (outcome[b] == vigo::kReguideDone)
                for (int j = g_off[q]; j < g_off[q + 1]; ++j) put(g_pv.data() + 6 * (size_t)j, g_unk[j]);
        }
    out_guide_off[(size_t)B * N] = (int)at;
    if (!no_paths) {
        std::copy(ps_seg_off.begin(), ps_seg_off.end(), out_path_seg_off);
        std::copy(ps_path_off.begin(), ps_path_off.begin() + total_seg + 1, out_path_off);
        std::copy(ps_path.begin(), ps_path.begin() + 3 * total_pts, out_path);
    }
    for (int b = 0; b < B; ++b) {
        out_status[b] = outcome[b];
        if (outcome[b] == vigo::kReguideDeferred || outcome[b] == vigo::kReguideSkipped) continue;
        vigo_rebound_state_t& st = state[b];
        st.n_seg = n_new[b];
        std::copy(new_seg.begin() + (size_t)b * 2 * kSegs, new_seg.begin() + (size_t)b * 2 * kSegs + 2 * n_new[b], st.seg);
        vigo::reguide_commit(outcome[b], st.gate_dynamic != 0, weights + 4 * (size_t)b, &st.fail_count, &st.status, &st.solve_first);
    }
    return 0;
}

// the header's rules alone on flags: pt / ln uint8[N], prev int[n_prev][2], need uint8[N] (isControlPointRequireNewGuide
// per control point) -> the number of new segments, out_seg[cap][2], out_listed[cap], *out_n_list
int vigo_host_reguide_rules(int N, double not_check_ratio, const unsigned char* pt, const unsigned char* ln, int n_prev, const int* prev,
                            const unsigned char* need, int cap, int* out_seg, unsigned char* out_listed, int* out_n_list) {
    return vigo::reguide_rules(N, not_check_ratio, [&](int i) { return pt[i] != 0; }, [&](int i) { return ln[i] != 0; }, n_prev, prev,
                               [&](int i) { return need[i] != 0; }, cap, out_seg, out_listed, out_n_list);
}

// The FACADE's own step on the same inputs: one planner per trajectory on a dense byte grid with these control points,
// collisionSeg_ (state[b].n_seg, seg), guide pairs (guide_off / guide_pv, or NULL), the weights and failCount
// (state[b].fail_count), then bsplineTraj::reboundStep(r, true, state[b].gate_dynamic != 0, false) — the existing host
// code, unchanged.  Out: weights; state[b].fail_count, n_seg (the true count) and seg (the first
// VIGO_MAX_COLLISION_SEGS); the planner's guide pairs as CSR; astarPaths_ as CSR (path_seg_off[B+1], path_off, path);
// need_optimize[B].  cfg as in vigo_host_bspline_prologue.  Returns 0, -1 on a bad argument, -2 when a buffer is too small.
int vigo_host_reguide_facade(const unsigned char* vox, const int* dims, const double* origin, double res, int B, int N, const double* ctrl,
                             const int* guide_off, const double* guide_pv, double* weights, const double* cfg, vigo_rebound_state_t* state,
                             long long pair_cap, int* out_guide_off, double* out_guide_pv, long long seg_cap, long long point_cap,
                             int* out_path_seg_off, int* out_path_off, double* out_path, int* out_need_optimize) {
    if (B < 0 || N < 7 || !ctrl || !weights || !cfg || !state || !out_guide_off || !out_guide_pv || !out_path_seg_off || !out_path_off || !out_path ||
        !out_need_optimize || (!guide_off != !guide_pv))
        return -1;
    PlannerPool pool;
    initPool(pool, vox, dims, origin, res, cfg);
    std::vector<std::vector<int32_t>> off(B);
    std::vector<std::vector<double>> pv(B);
    std::vector<std::vector<std::vector<Eigen::Vector3d>>> paths(B);
    vigo_host::parallelFor((size_t)B, [&](size_t b) {
        auto bt = pool.take();
        bt->clear();
        Eigen::MatrixXd c(3, N);
        for (int i = 0; i < N; ++i) for (int k = 0; k < 3; ++k) c(k, i) = ctrl[(b * N + i) * 3 + k];
        bt->setControlPoints(c);
        vigo_rebound_state_t& st = state[b];
        std::vector<std::pair<int, int>> sg;
        for (int k = 0; k < st.n_seg && k < VIGO_MAX_COLLISION_SEGS; ++k) sg.push_back({st.seg[2 * k], st.seg[2 * k + 1]});
        std::vector<std::vector<Eigen::Vector3d>> gp(N), gd(N);
        if (guide_off)
            for (int i = 0; i < N; ++i)
                for (int j = guide_off[b * N + i]; j < guide_off[b * N + i + 1]; ++j) {
                    const double* q = guide_pv + 6 * (size_t)j;
                    gp[i].push_back(Eigen::Vector3d(q[0], q[1], q[2]));
                    gd[i].push_back(Eigen::Vector3d(q[3], q[4], q[5]));
                }
        double save_d, save_o;
        bt->getLoopWeights(save_d, save_o);
        bt->setLoopState(sg, gp, gd, weights[4 * b + 0], weights[4 * b + 3]);
        int failCount = st.fail_count;
        bool needOptimize = false, done = false;
        bt->runLoopBody(true, st.gate_dynamic != 0, failCount, needOptimize, done);
        bt->getLoopWeights(weights[4 * b + 0], weights[4 * b + 3]);
        st.fail_count = failCount;
        out_need_optimize[b] = needOptimize ? 1 : 0;
        const auto& ns = bt->getCollisionSeg();
        st.n_seg = (int32_t)ns.size();
        for (size_t k = 0; k < ns.size() && k < (size_t)VIGO_MAX_COLLISION_SEGS; ++k) { st.seg[2 * k] = ns[k].first; st.seg[2 * k + 1] = ns[k].second; }
        off[b].assign(1, 0);
        vigo_host::appendGuides(bt->getOptData(), N, off[b], pv[b]);
        paths[b] = bt->getAstarPaths();
        bt->setLoopState({}, {}, {}, save_d, save_o);
        pool.give(std::move(bt));
    });
    long long g = 0, s = 0, q = 0;
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < N; ++i) out_guide_off[(size_t)b * N + i] = (int)(g + off[b][i]);
        g += off[b][N];
        s += (long long)paths[b].size();
        for (const auto& p : paths[b]) q += (long long)p.size();
    }
    out_guide_off[(size_t)B * N] = (int)g;
    if (g > pair_cap || s > seg_cap || q > point_cap) return -2;
    long long w = 0;
    for (int b = 0; b < B; ++b) { std::memcpy(out_guide_pv + 6 * w, pv[b].data(), pv[b].size() * sizeof(double)); w += (long long)pv[b].size() / 6; }
    s = 0; q = 0;
    for (int b = 0; b < B; ++b) {
        out_path_seg_off[b] = (int)s;
        for (const auto& p : paths[b]) {
            out_path_off[s++] = (int)q;
            for (const auto& v : p) { for (int a = 0; a < 3; ++a) out_path[3 * q + a] = v(a); ++q; }
        }
    }
    out_path_seg_off[B] = (int)s;
    out_path_off[s] = (int)q;
    return 0;
}

}  // extern "C"

extern "C" {

// The epilogue stage alone (bsplineTraj::finishBatch: steps 5-6 and evalTrajToMsg) for n planners on one dense byte grid
// with the control points ctrl[n][Ns][3], n_pts[n] of them each: `reps` rounds, deviceEpilogue off then on in each,
// wall time in ms[reps][2].  *mismatch: planners whose linearFactor_, pose count, positions or quaternions of the last
// round differ between the two.  Returns 0, -1 on a bad argument.  Needs a GPU.
int vigo_host_finish_timing(const unsigned char* vox, const int* dims, const double* origin, double res, const double* cfg, int n, int Ns,
                            const int* n_pts, const double* ctrl, int reps, double* ms, long long* mismatch) {
    if (n < 1 || Ns < 7 || reps < 1 || !n_pts || !ctrl || !cfg || !ms || !mismatch) return -1;
    const std::shared_ptr<mapManager::occMap> map = denseMap(dims[0], dims[1], dims[2], origin, res, vox);
    ros::NodeHandle nh;
    setBsplineParams(nh, cfg);
    std::vector<std::unique_ptr<bsplineTraj>> owners;
    std::vector<bsplineTraj*> ps;
    for (int t = 0; t < n; ++t) {
        if (n_pts[t] < 7 || n_pts[t] > Ns) return -1;
        owners.emplace_back(new bsplineTraj(nh));
        owners.back()->setMap(map);
        owners.back()->updateMaxVel(2.0);
        owners.back()->updateMaxAcc(3.0);
        Eigen::MatrixXd c(3, n_pts[t]);
        for (int i = 0; i < n_pts[t]; ++i) for (int k = 0; k < 3; ++k) c(k, i) = ctrl[((size_t)t * Ns + i) * 3 + k];
        owners.back()->setControlPoints(c);
        ps.push_back(owners.back().get());
    }
    std::vector<nav_msgs::Path> traj[2];
    std::vector<double> factor[2];
    for (int rep = 0; rep < reps; ++rep)
        for (int slot = 0; slot < 2; ++slot) {
            bsplineTraj::BatchOptions o;
            o.deviceEpilogue = slot == 1;
            const auto t0 = std::chrono::steady_clock::now();
            bsplineTraj::finishBatch(ps, &traj[slot], true, o);
            ms[2 * rep + slot] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            factor[slot].clear();
            for (bsplineTraj* p : ps) factor[slot].push_back(p->getLinearFactor());
        }
    *mismatch = 0;
    for (int t = 0; t < n; ++t) {
        bool same = std::memcmp(&factor[0][t], &factor[1][t], sizeof(double)) == 0 && traj[0][t].poses.size() == traj[1][t].poses.size();
        for (size_t i = 0; same && i < traj[0][t].poses.size(); ++i) {
            const auto &a = traj[0][t].poses[i].pose, &b = traj[1][t].poses[i].pose;
            const double va[7] = {a.position.x, a.position.y, a.position.z, a.orientation.x, a.orientation.y, a.orientation.z, a.orientation.w};
            const double vb[7] = {b.position.x, b.position.y, b.position.z, b.orientation.x, b.orientation.y, b.orientation.z, b.orientation.w};
            same = std::memcmp(va, vb, sizeof(va)) == 0;
        }
        *mismatch += same ? 0 : 1;
    }
    return 0;
}

}  // extern "C"

// mapAdapter::rasterise (the generic route: four public map methods only) over the whole box of a dense map must give
// back that map's inflated-occupied and unknown bits.  Returns the number of differing voxels (0 = agreement), -1 on
// failure; dims_out receives the rasterised grid's extents.
extern "C" long long vigo_host_rasterise_check(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels,
                                               const double* box_min, const double* box_max, int* dims_out) {
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    trajPlanner::mapRegion region;
    region.set = true;
    region.boxMin = Eigen::Vector3d(box_min[0], box_min[1], box_min[2]);
    region.boxMax = Eigen::Vector3d(box_max[0], box_max[1], box_max[2]);
    std::vector<uint8_t> vox;
    int dims[3];
    double o[3];
    if (!trajPlanner::mapAdapter::rasterise(*map, region, vox, dims, o)) return -1;
    for (int a = 0; a < 3; ++a) dims_out[a] = dims[a];
    long long bad = 0;
    for (int ix = 0; ix < dims[0]; ++ix)
        for (int iy = 0; iy < dims[1]; ++iy)
            for (int iz = 0; iz < dims[2]; ++iz) {
                const Eigen::Vector3d c(o[0] + (ix + 0.5) * res, o[1] + (iy + 0.5) * res, o[2] + (iz + 0.5) * res);
                const unsigned want = map->byteAt(c);          // 0xFF outside the dense map: occupied and unknown
                const unsigned got = vox[((size_t)ix * dims[1] + iy) * dims[2] + iz];
                if ((got & 1u) != (want & 1u) || ((got >> 1) & 1u) != ((want >> 1) & 1u) || ((got >> 2) & 1u) != (got & 1u)) ++bad;
            }
    return bad;
}

// mapAdapter::rasteriseBox against a whole rasterisation, CPU only: the dense map is rasterised over the region
// [box_min, box_max] (grid A), the edit (edit_n bytes at voxel edit_lo of the dense map's own lattice) is written into the
// map, rasteriseBox runs over [sub_min, sub_max] and its bytes are patched into A (vigo_grid_region_apply_host, raw mode);
// the map is then rasterised whole again (grid B).  dims_out: the grids' extents, lo_out / n_out: what rasteriseBox
// returned, patched / whole: A and B, cap bytes each.  Returns 0, -1 when a step failed, -2 when cap is too small.
extern "C" int vigo_host_rasterise_box(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels, const double* box_min,
                                       const double* box_max, const int* edit_lo, const int* edit_n, const unsigned char* edit_bytes,
                                       const double* sub_min, const double* sub_max, long long cap, int* dims_out, int* lo_out, int* n_out,
                                       unsigned char* patched, unsigned char* whole) {
    auto map = denseMap(nx, ny, nz, origin, res, voxels);
    trajPlanner::mapRegion region;
    region.set = true;
    region.boxMin = Eigen::Vector3d(box_min[0], box_min[1], box_min[2]);
    region.boxMax = Eigen::Vector3d(box_max[0], box_max[1], box_max[2]);
    std::vector<uint8_t> a, b, bytes;
    int dims[3], lo[3], n[3];
    double o[3];
    if (!trajPlanner::mapAdapter::rasterise(*map, region, a, dims, o)) return -1;
    for (int k = 0; k < 3; ++k)
        if (edit_lo[k] < 0 || edit_n[k] < 0 || edit_lo[k] + edit_n[k] > (k == 0 ? nx : k == 1 ? ny : nz)) return -1;
    for (int ix = 0; ix < edit_n[0]; ++ix)
        for (int iy = 0; iy < edit_n[1]; ++iy)
            for (int iz = 0; iz < edit_n[2]; ++iz)
                map->at(edit_lo[0] + ix, edit_lo[1] + iy, edit_lo[2] + iz) = edit_bytes[((size_t)ix * edit_n[1] + iy) * edit_n[2] + iz];
    if (!trajPlanner::mapAdapter::rasteriseBox(*map, region, Eigen::Vector3d(sub_min[0], sub_min[1], sub_min[2]),
                                               Eigen::Vector3d(sub_max[0], sub_max[1], sub_max[2]), bytes, lo, n))
        return -1;
    if (bytes.size() != (size_t)n[0] * n[1] * n[2]) return -1;
    if (!bytes.empty() && vigo_grid_region_apply_host(dims[0], dims[1], dims[2], a.data(), lo, n, bytes.data(), nullptr) != VIGO_OK) return -1;
    if (!trajPlanner::mapAdapter::rasterise(*map, region, b, dims, o)) return -1;
    for (int k = 0; k < 3; ++k) { dims_out[k] = dims[k]; lo_out[k] = lo[k]; n_out[k] = n[k]; }
    if ((long long)a.size() > cap) return -2;
    std::memcpy(patched, a.data(), a.size());
    std::memcpy(whole, b.data(), b.size());
    return 0;
}

// trajPlanner::DirtyJournal on its own, CPU only: n_rec entries (version[k], a box whose every lo is version[k] and every n
// is k) are recorded in turn, then changesSince(since, now) is asked.  Returns -1 when it is false, else the number of
// entries, with versions_out / n_out (cap values each) the entries' version and n[0].
extern "C" int vigo_host_dirty_journal(int n_rec, const unsigned long long* version, unsigned long long since, unsigned long long now, int cap,
                                       unsigned long long* versions_out, int* n_out) {
    trajPlanner::DirtyJournal j;
    for (int k = 0; k < n_rec; ++k) {
        const int lo[3] = {(int)version[k], (int)version[k], (int)version[k]}, n[3] = {k, k, k};
        j.record(version[k], lo, n);
    }
    std::vector<trajPlanner::DirtyBox> out;
    if (!j.changesSince(since, now, out)) return -1;
    if ((int)out.size() > cap) return -2;
    for (size_t k = 0; k < out.size(); ++k) {
        if (out[k].lo[0] != (int)out[k].version || out[k].lo[2] != (int)out[k].version || out[k].n[0] != out[k].n[1]) return -3;
        versions_out[k] = out[k].version;
        n_out[k] = out[k].n[0];
    }
    return (int)out.size();
}

// A map that changes under planners that share it: n planners with a pose list each (as vigo_host_plan_batch) on
// ONE dense map plan by makePlanBatch(planners) under the options of `mask`, after the first upload (round 0) and after
// each of E edits (round e + 1): edit e writes the bytes edit_bytes[edit_off[e] ..) as the box edit_n[e] at voxel
// edit_lo[e] into the map and then tells the planners by mode 0: a bare ++version, mode 1: markChanged(lo, n).  The
// planners (and their handles) live through all rounds; every round starts from updatePathBatch on the same paths.
// Outputs per round r as slot r of dumpSlot: ok, solver, ncp [E+1][n], ctrl [E+1][n][ncp_cap][3] (zero padded by the
// caller); totals[3]: what mapAdapter::snapshotTotals moved by over the call (full snapshots, region updates, region
// voxels); round_ms[E+1]: the wall time of the round's makePlanBatch, the snapshot refresh included.  Returns 0, -1 on a
// bad argument, -2 when ncp_cap is too small, -3 when a call threw.  Needs a GPU.
extern "C" int vigo_host_map_update_replan(const unsigned char* vox, const int* dims, const double* origin, double res, int n, const int* path_off,
                                           const double* path_xyz, const double* cfg, int mask, int E, const int* edit_lo, const int* edit_n,
                                           const long long* edit_off, const unsigned char* edit_bytes, int mode, int ncp_cap, int* ok,
                                           int* solver, int* ncp, double* ctrl, long long* totals, double* round_ms) {
    if (n < 1 || !path_off || !path_xyz || !cfg || mask < 0 || E < 0 || (mode != 0 && mode != 1)) return -1;
    for (int t = 0; t < n; ++t)
        if (path_off[t + 1] - path_off[t] < 2) return -1;
    for (int e = 0; e < E; ++e)
        for (int a = 0; a < 3; ++a)
            if (edit_lo[3 * e + a] < 0 || edit_n[3 * e + a] < 0 || edit_lo[3 * e + a] + edit_n[3 * e + a] > dims[a]) return -1;
    try {
        BatchFixture fx(vox, dims, origin, res, cfg, n, path_off, path_xyz);
        const trajPlanner::mapAdapter::SnapshotTotals before = trajPlanner::mapAdapter::snapshotTotals();   // (the planners' first fit uploads)
        FreshPlanners fp = freshPlanners(fx);
        mapManager::occMap& map = *fx.maps[0];
        const bsplineTraj::BatchOptions o = optionsOfMask(mask, 16384);
        vigo_host_plan_batch_job_t out{};
        out.ncp_cap = ncp_cap; out.ok = ok; out.solver = solver; out.ncp = ncp; out.ctrl = ctrl;
        for (int r = 0; r <= E; ++r) {
            if (r > 0) {
                const int e = r - 1;
                const int *lo = edit_lo + 3 * e, *en = edit_n + 3 * e;
                const unsigned char* src = edit_bytes + edit_off[e];
                for (int ix = 0; ix < en[0]; ++ix)
                    for (int iy = 0; iy < en[1]; ++iy)
                        for (int iz = 0; iz < en[2]; ++iz) map.at(lo[0] + ix, lo[1] + iy, lo[2] + iz) = src[((size_t)ix * en[1] + iy) * en[2] + iz];
                if (mode == 1) map.markChanged(lo, en);
                else ++map.version;
                bsplineTraj::updatePathBatch(fp.ps, fx.in, fx.cond);
            }
            bsplineTraj::BatchStats st;
            const std::vector<bool> planned = timedPlan(fp.ps, o, round_ms[r], st);
            const int rc = dumpSlot(fp.ps, planned, r, out);
            if (rc != 0) return rc;
        }
        const trajPlanner::mapAdapter::SnapshotTotals after = trajPlanner::mapAdapter::snapshotTotals();
        totals[0] = after.fullSnapshots - before.fullSnapshots;
        totals[1] = after.regionUpdates - before.regionUpdates;
        totals[2] = after.regionVoxels - before.regionVoxels;
    } catch (...) {
        return -3;
    }
    return 0;
}

// The facade's snapshot refresh alone, timed: a DeviceLink on a dense map is synced once (the first upload), then `reps`
// times the owner announces a change of the box [lo, lo + n) — mode 0: ++version, mode 1: markChanged(lo, n) — and the
// next sync() is timed into ms[rep] (wall clock; sync() returns when the snapshot is on the device).  totals[3]: what
// mapAdapter::snapshotTotals moved by over the reps.  Returns 0, -1 when a sync failed.  Needs a GPU.
extern "C" int vigo_host_snapshot_refresh(const unsigned char* vox, const int* dims, const double* origin, double res, const int* lo, const int* n,
                                          int mode, int reps, double* ms, long long* totals) {
    auto map = denseMap(dims[0], dims[1], dims[2], origin, res, vox);
    trajPlanner::DeviceLink link;
    link.setMap(map);
    if (link.sync(true) != trajPlanner::DeviceLink::kSynced) return -1;
    const trajPlanner::mapAdapter::SnapshotTotals before = trajPlanner::mapAdapter::snapshotTotals();
    for (int rep = 0; rep < reps; ++rep) {
        if (mode == 1) map->markChanged(lo, n);
        else ++map->version;
        const auto t0 = std::chrono::steady_clock::now();
        if (link.sync(true) != trajPlanner::DeviceLink::kSynced) return -1;
        ms[rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const trajPlanner::mapAdapter::SnapshotTotals after = trajPlanner::mapAdapter::snapshotTotals();
    totals[0] = after.fullSnapshots - before.fullSnapshots;
    totals[1] = after.regionUpdates - before.regionUpdates;
    totals[2] = after.regionVoxels - before.regionVoxels;
    return 0;
}

namespace {
// n planners on the fixture's one map, each fitted to its pose list by updatePath (held plans: nothing is planned); planner
// `no_device` is bound to a card that does not exist, planner `not_init` never gets a path (either -1: none); planner t's
// dynamic obstacles are rows obs_off[t] .. obs_off[t + 1] - 1 of obs[][9] (position, velocity, size), obs_off NULL: none
FreshPlanners heldPlanners(const BatchFixture& fx, int no_device, int not_init, const int* obs_off, const double* obs) {
    FreshPlanners fp;
    for (size_t t = 0; t < fx.in.size(); ++t) {
        fp.owners.emplace_back(new bsplineTraj(fx.nh));
        bsplineTraj& p = *fp.owners.back();
        p.setMap(fx.maps[0]);
        p.updateMaxVel(2.0);
        p.updateMaxAcc(3.0);
        if ((int)t == no_device) p.setDevice(63);
        if ((int)t != not_init) p.updatePath(fx.in[t], fx.cond[t]);
        if (obs_off && obs_off[t + 1] > obs_off[t]) {
            std::vector<Eigen::Vector3d> pos, vel, size;
            for (int j = obs_off[t]; j < obs_off[t + 1]; ++j) {
                const double* o = obs + 9 * (size_t)j;
                pos.push_back(Eigen::Vector3d(o[0], o[1], o[2]));
                vel.push_back(Eigen::Vector3d(o[3], o[4], o[5]));
                size.push_back(Eigen::Vector3d(o[6], o[7], o[8]));
            }
            p.updateDynamicObstacles(pos, vel, size);
        }
        fp.ps.push_back(&p);
    }
    return fp;
}

// both routes on the planners as they stand, into slot 0 (isCurrTrajValidBatch) and slot 1 (the per-planner loop:
// isCurrTrajValid(pos), hasDynamicCollisionTrajectory) of valid[2][n], pos[2][n][3] (an entry is written only where the
// route writes it), dyn[2][n]; stats[3]: the batch call's validateDecided, validateHost, validateGroups
void validateBothRoutes(const std::vector<bsplineTraj*>& ps, int* valid, double* pos, int* dyn, long long* stats) {
    const size_t n = ps.size();
    std::vector<Eigen::Vector3d> hit(n);
    for (size_t t = 0; t < n; ++t) hit[t] = Eigen::Vector3d(pos[3 * t], pos[3 * t + 1], pos[3 * t + 2]);
    std::vector<bool> dynamic;
    bsplineTraj::BatchStats st;
    const std::vector<bool> ok = bsplineTraj::isCurrTrajValidBatch(ps, &hit, &dynamic, &st);
    for (size_t t = 0; t < n; ++t) {
        valid[t] = ok[t] ? 1 : 0;
        dyn[t] = dynamic[t] ? 1 : 0;
        for (int a = 0; a < 3; ++a) pos[3 * t + a] = hit[t](a);
        Eigen::Vector3d one(pos[3 * (n + t)], pos[3 * (n + t) + 1], pos[3 * (n + t) + 2]);
        valid[n + t] = ps[t]->isCurrTrajValid(one) ? 1 : 0;
        dyn[n + t] = ps[t]->hasDynamicCollisionTrajectory(ps[t]->getControlPoints()) ? 1 : 0;
        for (int a = 0; a < 3; ++a) pos[3 * (n + t) + a] = one(a);
    }
    stats[0] = st.validateDecided;
    stats[1] = st.validateHost;
    stats[2] = st.validateGroups;
}
}  // namespace

// Held plans validated in one call: n planners with a pose list each (as vigo_host_plan_batch) on ONE dense map,
// made by heldPlanners (no_device, not_init, obs_off / obs as there).  Outputs: validateBothRoutes' valid, pos, dyn (pos
// prefilled by the caller) and stats; ncp[n] the planners' control-point counts; totals[3]: what the same three fields of
// bsplineTraj::batchTotals() moved by over the batch call; ms[reps][2] (reps may be 0): the wall time of the batch form and
// of the per-planner loop, run again in turn.  Returns 0, -1 on a bad argument, -3 when a call threw.  Needs a GPU.
extern "C" int vigo_host_validate_batch(const unsigned char* vox, const int* dims, const double* origin, double res, int n, const int* path_off,
                                        const double* path_xyz, const double* cfg, int no_device, int not_init, const int* obs_off, const double* obs,
                                        int* valid, double* pos, int* dyn, int* ncp, long long* stats, long long* totals, int reps, double* ms) {
    if (n < 1 || !path_off || !path_xyz || !cfg || !valid || !pos || !dyn || !ncp || !stats || !totals || reps < 0 || (reps > 0 && !ms)) return -1;
    for (int t = 0; t < n; ++t)
        if (path_off[t + 1] - path_off[t] < 2) return -1;
    try {
        BatchFixture fx(vox, dims, origin, res, cfg, n, path_off, path_xyz);
        FreshPlanners fp = heldPlanners(fx, no_device, not_init, obs_off, obs);
        for (int t = 0; t < n; ++t) ncp[t] = (int)fp.ps[t]->getControlPoints().cols();
        const bsplineTraj::BatchStats before = bsplineTraj::batchTotals();
        validateBothRoutes(fp.ps, valid, pos, dyn, stats);
        const bsplineTraj::BatchStats after = bsplineTraj::batchTotals();
        totals[0] = after.validateDecided - before.validateDecided;
        totals[1] = after.validateHost - before.validateHost;
        totals[2] = after.validateGroups - before.validateGroups;
        // (workload tools) the two routes again, alternating, wall clock per route: the answers above stand
        for (int rep = 0; rep < reps; ++rep) {
            std::vector<Eigen::Vector3d> hit(fp.ps.size());
            std::vector<bool> dynamic;
            auto t0 = std::chrono::steady_clock::now();
            (void)bsplineTraj::isCurrTrajValidBatch(fp.ps, &hit, &dynamic);
            ms[2 * rep] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            t0 = std::chrono::steady_clock::now();
            for (bsplineTraj* p : fp.ps) {
                Eigen::Vector3d one;
                (void)p->isCurrTrajValid(one);
                (void)p->hasDynamicCollisionTrajectory(p->getControlPoints());
            }
            ms[2 * rep + 1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
    } catch (...) {
        return -3;
    }
    return 0;
}

// A map that changes under held plans: the planners of vigo_host_validate_batch (all with a device, all initialised, no
// obstacles) are validated by both routes after the first upload (round 0) and after each of E edits (round e + 1), edit e
// written and announced as in vigo_host_map_update_replan (mode 0: ++version, mode 1: markChanged(lo, n)).  Outputs per
// round r: valid[E+1][2][n], pos[E+1][2][n][3] (prefilled by the caller), dyn[E+1][2][n], stats[E+1][3]; totals[3]: what
// mapAdapter::snapshotTotals moved by over the call.  Returns 0, -1 on a bad argument, -3 when a call threw.  Needs a GPU.
extern "C" int vigo_host_map_update_validate(const unsigned char* vox, const int* dims, const double* origin, double res, int n, const int* path_off,
                                             const double* path_xyz, const double* cfg, int E, const int* edit_lo, const int* edit_n,
                                             const long long* edit_off, const unsigned char* edit_bytes, int mode, int* valid, double* pos, int* dyn,
                                             long long* stats, long long* totals) {
    if (n < 1 || !path_off || !path_xyz || !cfg || E < 0 || (mode != 0 && mode != 1) || !valid || !pos || !dyn || !stats || !totals) return -1;
    for (int t = 0; t < n; ++t)
        if (path_off[t + 1] - path_off[t] < 2) return -1;
    for (int e = 0; e < E; ++e)
        for (int a = 0; a < 3; ++a)
            if (edit_lo[3 * e + a] < 0 || edit_n[3 * e + a] < 0 || edit_lo[3 * e + a] + edit_n[3 * e + a] > dims[a]) return -1;
    try {
        BatchFixture fx(vox, dims, origin, res, cfg, n, path_off, path_xyz);
        const trajPlanner::mapAdapter::SnapshotTotals before = trajPlanner::mapAdapter::snapshotTotals();
        FreshPlanners fp = heldPlanners(fx, -1, -1, nullptr, nullptr);
        mapManager::occMap& map = *fx.maps[0];
        for (int r = 0; r <= E; ++r) {
            if (r > 0) {
                const int e = r - 1;
                const int *lo = edit_lo + 3 * e, *en = edit_n + 3 * e;
                const unsigned char* src = edit_bytes + edit_off[e];
                for (int ix = 0; ix < en[0]; ++ix)
                    for (int iy = 0; iy < en[1]; ++iy)
                        for (int iz = 0; iz < en[2]; ++iz) map.at(lo[0] + ix, lo[1] + iy, lo[2] + iz) = src[((size_t)ix * en[1] + iy) * en[2] + iz];
                if (mode == 1) map.markChanged(lo, en);
                else ++map.version;
            }
            validateBothRoutes(fp.ps, valid + (size_t)r * 2 * n, pos + (size_t)r * 6 * n, dyn + (size_t)r * 2 * n, stats + 3 * r);
        }
        const trajPlanner::mapAdapter::SnapshotTotals after = trajPlanner::mapAdapter::snapshotTotals();
        totals[0] = after.fullSnapshots - before.fullSnapshots;
        totals[1] = after.regionUpdates - before.regionUpdates;
        totals[2] = after.regionVoxels - before.regionVoxels;
    } catch (...) {
        return -3;
    }
    return 0;
}
