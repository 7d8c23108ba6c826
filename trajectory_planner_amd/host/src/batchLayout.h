// batchLayout.h — internal to the host facades: bsplineTraj's optData flattened into the batch layouts of include/vigo.h
// (control points column by column; guide pairs and dynamic obstacles as CSR lists, offsets + flat list), what comes
// back in those layouts installed into a planner, and the order in which planners are grouped into device batches.
#ifndef VIGO_HOST_BATCH_LAYOUT_H
#define VIGO_HOST_BATCH_LAYOUT_H
#include <trajectory_planner/bsplineTraj.h>

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace vigo_host {

// The guide pairs (point, direction: 6 doubles) of control points 0 .. N-1 in push order, appended to pv; after each
// control point the running pair count is appended to off (N offsets).  A control point without a guide list (guidePoints
// shorter than N, as clear() leaves it) has no pairs.
inline void appendGuides(const trajPlanner::optData& od, int N, std::vector<int32_t>& off, std::vector<double>& pv) {
    for (int i = 0; i < N; ++i) {
        const size_t cnt = i < (int)od.guidePoints.size() ? od.guidePoints[i].size() : 0;
        for (size_t j = 0; j < cnt; ++j) {
            for (int q = 0; q < 3; ++q) pv.push_back(od.guidePoints[i][j](q));
            for (int q = 0; q < 3; ++q) pv.push_back(od.guideDirections[i][j](q));
        }
        off.push_back((int32_t)(pv.size() / 6));
    }
}

// appendGuides' inverse for one planner: of the pairs off[i] .. off[i + 1] of control point i (off: the planner's N + 1
// offsets into pv) those after the first skip_i are appended to its lists.  skip_i is 0, or with skipHeld the number of
// pairs the control point holds already (a CSR that repeats the held pairs before the new ones).
inline void installGuides(trajPlanner::optData& od, int N, const int32_t* off, const double* pv, bool skipHeld = false) {
    for (int i = 0; i < N; ++i)
        for (int g = off[i] + (skipHeld ? (int)od.guidePoints[i].size() : 0); g < off[i + 1]; ++g) {
            const double* q = pv + (size_t)g * 6;
            od.guidePoints[i].push_back(Eigen::Vector3d(q[0], q[1], q[2]));
            od.guideDirections[i].push_back(Eigen::Vector3d(q[3], q[4], q[5]));
        }
}

// the paths of the segments s0 .. s1-1 of a CSR (pathOff: offsets into path's xyz triples) in place of a planner's paths
inline void installPaths(std::vector<std::vector<Eigen::Vector3d>>& paths, int s0, int s1, const int32_t* pathOff, const double* path) {
    paths.clear();
    for (int k = s0; k < s1; ++k) {
        paths.emplace_back();
        for (int q = pathOff[k]; q < pathOff[k + 1]; ++q)
            paths.back().push_back(Eigen::Vector3d(path[3 * (size_t)q], path[3 * (size_t)q + 1], path[3 * (size_t)q + 2]));
    }
}

// a planner's control points (3 x N, column by column) appended to ctrl as [N][3]
inline void appendCtrl(const Eigen::MatrixXd& controlPoints, std::vector<double>& ctrl) {
    ctrl.insert(ctrl.end(), controlPoints.data(), controlPoints.data() + 3 * (size_t)controlPoints.cols());
}

// the dynamic obstacles (position, velocity, size: 9 doubles each) appended to obs
inline void appendObstacles(const trajPlanner::optData& od, std::vector<double>& obs) {
    for (size_t j = 0; j < od.dynamicObstaclesPos.size(); ++j) {
        for (int q = 0; q < 3; ++q) obs.push_back(od.dynamicObstaclesPos[j](q));
        for (int q = 0; q < 3; ++q) obs.push_back(od.dynamicObstaclesVel[j](q));
        for (int q = 0; q < 3; ++q) obs.push_back(od.dynamicObstaclesSize[j](q));
    }
}

// B trajectories in rows of N control points each, added one planner at a time.  A planner of n < N control points (the
// layout of the vigo_*_mixed entries, include/vigo.h) owns the first n points of its row: the rest is zeros, the padded
// points have empty guide lists — control point i of trajectory b is entry b * N + i of goff either way — and npts holds n.
struct HostBatch {
    int B = 0, N;
    std::vector<double> ctrl, gpv, obs, weights;
    std::vector<int32_t> goff{0}, ooff{0}, npts;
    explicit HostBatch(int stride) : N(stride) {}
    // controlPoints: 3 x n column by column, n <= N; w: (distance, smoothness, feasibility, dynamic)
    void add(const double* controlPoints, int n, const trajPlanner::optData& od, const std::array<double, 4>& w) {
        addRow(controlPoints, n);
        appendGuides(od, n, goff, gpv);
        goff.resize(goff.size() + (size_t)(N - n), goff.back());
        appendObstacles(od, obs);
        ooff.push_back((int32_t)(obs.size() / 9));
        weights.insert(weights.end(), w.begin(), w.end());
    }
    // the row and its count alone, for a stage that reads neither lists nor weights (the finish stage)
    void addRow(const double* controlPoints, int n) {
        ctrl.insert(ctrl.end(), controlPoints, controlPoints + 3 * n);
        ctrl.resize(ctrl.size() + 3 * (size_t)(N - n), 0.0);
        npts.push_back(n);
        ++B;
    }
    void add(const double* controlPoints, const trajPlanner::optData& od, const std::array<double, 4>& w) { add(controlPoints, N, od, w); }
    size_t guides() const { return gpv.size() / 6; }
    bool uniform() const {                       // every trajectory fills its row: the batch of the uniform entries
        for (int32_t n : npts)
            if (n != N) return false;
        return true;
    }
    const double* row(int b) const { return ctrl.data() + (size_t)b * 3 * N; }
};

// fn(members) for every group of the indices [0, n): the lead is the first index not in a group yet, the members are
// every index from the lead on that is not in a group yet and for which same(lead, index) holds, in increasing order.
// This order decides what goes into each device batch.  An index for which same(index, index) fails is in no group.
template <typename Same, typename Fn>
void forEachGroup(size_t n, Same same, Fn fn) {
    std::vector<bool> grouped(n, false);
    std::vector<size_t> members;
    for (size_t a = 0; a < n; ++a) {
        if (grouped[a]) continue;
        members.clear();
        for (size_t b = a; b < n; ++b)
            if (!grouped[b] && same(a, b)) {
                members.push_back(b);
                grouped[b] = true;
            }
        if (!members.empty()) fn(members);
    }
}

}  // namespace vigo_host
#endif  /* VIGO_HOST_BATCH_LAYOUT_H */
