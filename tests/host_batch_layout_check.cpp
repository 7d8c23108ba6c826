// host_batch_layout_check.cpp — HostBatch (host/src/batchLayout.h), the facade's packing of planners into the padded layout
// of the vigo_*_mixed entries, printed for tests/test_solver_plan_mixed.py to compare with synth.pad_batches.  No device.
// stdin: the row stride, then one planner per line: "n n_obs c_0 .. c_{n-1}" (control points, obstacles, guide pairs per
// control point).  Planner t's values are fixed functions of (t, point, pair, component), the same the test uses.
// stdout: one line each — "B N", npts, ctrl, goff, gpv, ooff, obs, weights, uniform().
#include <cstdio>
#include <vector>

#include "../trajectory_planner_amd/host/src/batchLayout.h"

template <class V>
static void print(const V& v, const char* fmt) {
    for (size_t i = 0; i < v.size(); ++i) { if (i) printf(" "); printf(fmt, v[i]); }
    printf("\n");
}

int main() {
    int stride;
    if (scanf("%d", &stride) != 1) return 1;
    vigo_host::HostBatch hb(stride);
    int n, n_obs;
    for (int t = 0; scanf("%d %d", &n, &n_obs) == 2; ++t) {
        trajPlanner::optData od;
        od.controlPoints = Eigen::MatrixXd(3, n);
        od.guidePoints.resize(n);
        od.guideDirections.resize(n);
        for (int i = 0; i < n; ++i) {
            int c;
            if (scanf("%d", &c) != 1) return 1;
            for (int k = 0; k < 3; ++k) od.controlPoints(k, i) = t * 100 + i + k * 0.25;
            for (int j = 0; j < c; ++j) {
                const double base = t * 1000 + i * 10 + j;
                od.guidePoints[i].push_back(Eigen::Vector3d(base, base + 0.125, base + 0.25));
                od.guideDirections[i].push_back(Eigen::Vector3d(base + 0.375, base + 0.5, base + 0.625));
            }
        }
        for (int j = 0; j < n_obs; ++j) {
            const double base = t * 7 + j;
            od.dynamicObstaclesPos.push_back(Eigen::Vector3d(base, base + 0.5, base + 1.0));
            od.dynamicObstaclesVel.push_back(Eigen::Vector3d(base + 1.5, base + 2.0, base + 2.5));
            od.dynamicObstaclesSize.push_back(Eigen::Vector3d(base + 3.0, base + 3.5, base + 4.0));
        }
        hb.add(od.controlPoints.data(), n, od, {1.0 + t, 2.0 + t, 3.0 + t, 4.0 + t});
    }
    printf("%d %d\n", hb.B, hb.N);
    print(hb.npts, "%d");
    print(hb.ctrl, "%.17g");
    print(hb.goff, "%d");
    print(hb.gpv, "%.17g");
    print(hb.ooff, "%d");
    print(hb.obs, "%.17g");
    print(hb.weights, "%.17g");
    printf("%d\n", (int)hb.uniform());
    return 0;
}
