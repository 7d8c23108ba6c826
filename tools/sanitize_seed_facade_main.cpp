// The facade's host steps of the seed-path stage under AddressSanitizer + UBSan, stand-alone (tools/sanitize_host.sh):
// bsplineTraj::seedSteps — getTrajectory(dt), the inputPathCheck search (inputPathCheckWith, seedSearchWith),
// prepareFitPointsWith — on min-snap plans made on the host through random box worlds, short paths for the fillPath
// branches, previous path lengths above and below max_path_length, one try and sixteen, a dt that is not positive.
// bsplineTraj.cpp links the HIP runtime and libvigo_hip.so; none of these steps calls into either, and no GPU is needed.
#include <trajectory_planner/bsplineTraj.h>
#include <trajectory_planner/polyTrajOccMap.h>
#include <cstdio>
#include <random>
int main() {
    using namespace trajPlanner;
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(-1, 1);
    int fails = 0; long ok = 0, ran = 0;
    for (int trial = 0; trial < 60; ++trial) {
        auto m = std::make_shared<mapManager::occMap>(80, 80, 24, Eigen::Vector3d(-4.0, -4.0, 0.0), 0.1);
        for (int b = 0; b < trial % 6; ++b) {
            const int cx = 10 + (int)(30 * (U(rng) + 1)), cy = 10 + (int)(30 * (U(rng) + 1)), h = 1 + (int)(4 * std::fabs(U(rng)));
            for (int x = std::max(0, cx - h); x < std::min(80, cx + h); ++x)
                for (int y = std::max(0, cy - h); y < std::min(80, cy + h); ++y)
                    for (int z = 0; z < 24; ++z) m->at(x, y, z) |= 1;
        }
        ros::NodeHandle nh;
        nh.setParam("bspline_traj/max_path_length", trial % 3 ? 1000.0 : 2.0);
        polyTrajOccMap poly(nh);
        poly.setMap(m);
        nav_msgs::Path path;
        const int W = 2 + trial % 3;
        for (int i = 0; i < W; ++i) {
            geometry_msgs::PoseStamped ps;
            ps.pose.position.x = -3.5 + 7.0 * i / (W - 1) * (trial % 5 == 4 ? 0.03 : 1.0); ps.pose.position.y = 3.0 * U(rng); ps.pose.position.z = 1.0 + 0.3 * U(rng);
            path.poses.push_back(ps);
        }
        poly.updatePath(path, std::vector<Eigen::Vector3d>(4, Eigen::Vector3d(0, 0, 0)));
        poly.makePlan(false);
        bsplineTraj bsp(nh);
        bsp.setMap(m);
        for (int v = 0; v < 4; ++v) {
            bsplineTraj::SeedSteps st;
            bsp.seedSteps(poly, v == 3 ? -1.0 : bsp.getInitTs(), v == 2 ? 1 : 16, v & 1 ? 3.0 : 0.0, v & 1 ? 2.5 : 0.0, st);
            ++ran;
            if (st.fitOk) { ++ok; if (st.fitPoints.size() < 4 || st.seed.poses.size() < 2) ++fails; }
            if (st.search.tries < 1 || st.search.tries > 16) ++fails;
        }
        nav_msgs::Path seed; double ft = 0;
        (void)bsp.inputPathCheck(poly.getTrajectory(bsp.getInitTs()), seed, bsp.getInitTs(), ft);
    }
    std::printf("seed facade steps: %ld runs, %ld fitted, %s\n", ran, ok, fails ? "FAILED" : "no failures");
    return fails || ok == 0;
}
