// polyBatch.h — internal to the host facades: the packing both min-snap planners (polyTrajOctomap, polyTrajOccMap) use
// around vigo_minsnap in their makePlanBatch.
#ifndef VIGO_HOST_POLY_BATCH_H
#define VIGO_HOST_POLY_BATCH_H
#include <trajectory_planner/polyTrajSolver.h>

#include <vector>

namespace vigo_host {

inline void appendXyz(const std::vector<trajPlanner::pose>& pts, std::vector<double>& xyz) {
    for (const trajPlanner::pose& q : pts) { xyz.push_back(q.x); xyz.push_back(q.y); xyz.push_back(q.z); }
}

// one planner's block [K][3][8] of vigo_minsnap's coefficients, installed as the solver's per-axis solution
inline void installDeviceSolution(trajPlanner::polyTrajSolver& solver, const double* co, int K) {
    const int D = 8;
    std::vector<double> axis[3];
    for (int c = 0; c < 3; ++c) {
        axis[c].resize((size_t)K * D);
        for (int sgm = 0; sgm < K; ++sgm)
            for (int d = 0; d < D; ++d) axis[c][sgm * D + d] = co[((size_t)sgm * 3 + c) * D + d];
    }
    solver.installSolution(axis[0], axis[1], axis[2]);
}

}  // namespace vigo_host
#endif  /* VIGO_HOST_POLY_BATCH_H */
