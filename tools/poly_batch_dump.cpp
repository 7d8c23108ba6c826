// poly_batch_dump.cpp — before/after evidence for polyTrajOctomap::makePlanBatch: calls only the public facade API, so
// the same source links against any build of libtrajectory_planner_vigo.so.  Writes, for every planner of every
// scenario, validity, iterations, the final waypoint path and the returned trajectory as raw bytes to argv[1] (compare
// two libraries' files with cmp), then times makePlanBatch of 32 and 1024 planners (median of argv[2] repetitions,
// default 3) and prints one JSON line.  Build (GPU box, after `make -C trajectory_planner_amd/host`):
//   hipcc -O2 -std=c++17 -Itrajectory_planner_amd/host/include tools/poly_batch_dump.cpp \
//         -Ltrajectory_planner_amd/lib -ltrajectory_planner_vigo -lvigo_hip -Wl,-rpath,<lib dir> -o poly_batch_dump
#include <trajectory_planner/polyTrajOctomap.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

using trajPlanner::polyTrajOctomap;
using trajPlanner::pose;

static std::shared_ptr<mapManager::occMap> pillarWorld(unsigned seed, int pillars) {
    auto m = std::make_shared<mapManager::occMap>(128, 128, 40, Eigen::Vector3d(-6.4, -6.4, -0.5), 0.1);
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> cx(10, 117), w(1, 3);
    for (int p = 0; p < pillars; ++p) {
        const int x = cx(rng), y = cx(rng), a = w(rng), b = w(rng);
        for (int i = x - a; i <= x + a; ++i)
            for (int j = y - b; j <= y + b; ++j)
                for (int k = 0; k < 40; ++k) m->at(i, j, k) |= 5;   // occupied (and inflated)
    }
    return m;
}

static std::unique_ptr<polyTrajOctomap> planner(const std::shared_ptr<mapManager::occMap>& map, bool adding, const std::vector<pose>& path) {
    ros::NodeHandle nh;
    nh.setParam("collision_box", std::vector<double>{0.4, 0.4, 0.2});
    nh.setParam("map_resolution", 0.2);
    nh.setParam("sample_delta_time", 0.1);
    nh.setParam("mode", adding ? 1.0 : 0.0);
    nh.setParam("initial_radius", 0.5);
    nh.setParam("shrinking_factor", 0.8);
    nh.setParam("corridor_res", 8.0);
    nh.setParam("maximum_iteration_num", 8.0);
    nh.setParam("traj_timeout", 0.5);
    std::unique_ptr<polyTrajOctomap> p(new polyTrajOctomap(nh));
    p->setMap(map);
    p->updatePath(path);
    return p;
}

// P seeded paths of 4-8 waypoints across the world (every 16th one 13 waypoints: the host QP), modes alternating
static std::vector<std::vector<pose>> paths(unsigned seed, int P) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(-5.0, 5.0), z(0.8, 1.6);
    std::uniform_int_distribution<int> nw(4, 8);
    std::vector<std::vector<pose>> out;
    for (int i = 0; i < P; ++i) {
        const int W = i % 16 == 5 ? 13 : nw(rng);
        const double x0 = u(rng), y0 = u(rng), x1 = u(rng), y1 = u(rng);
        std::vector<pose> p;
        for (int k = 0; k < W; ++k) {
            const double f = (double)k / (W - 1);
            p.push_back(pose(x0 + f * (x1 - x0) + 0.2 * (k % 2), y0 + f * (y1 - y0), z(rng)));
        }
        out.push_back(p);
    }
    return out;
}

struct Batch {
    std::vector<std::unique_ptr<polyTrajOctomap>> own;
    std::vector<polyTrajOctomap*> ps;
};

static Batch make(const std::shared_ptr<mapManager::occMap>& map, const std::vector<std::vector<pose>>& pp) {
    Batch b;
    for (size_t i = 0; i < pp.size(); ++i) {
        b.own.push_back(planner(map, i % 2 == 1, pp[i]));
        b.ps.push_back(b.own.back().get());
    }
    return b;
}

static void put(FILE* f, const void* p, size_t n) { std::fwrite(p, 1, n, f); }
static void putPoses(FILE* f, const std::vector<pose>& v) {
    const long long n = (long long)v.size();
    put(f, &n, sizeof n);
    for (const pose& q : v) { put(f, &q.x, 8); put(f, &q.y, 8); put(f, &q.z, 8); }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s dump_file [reps]\n", argv[0]); return 2; }
    const int reps = argc > 2 ? std::atoi(argv[2]) : 3;
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    // scenarios: the test_facade pillar geometry (paths beside / through one pillar, both modes) and seeded worlds
    std::vector<std::pair<std::shared_ptr<mapManager::occMap>, std::vector<std::vector<pose>>>> sc;
    {
        auto m = std::make_shared<mapManager::occMap>(128, 128, 40, Eigen::Vector3d(-6.4, -6.4, -0.5), 0.1);
        for (int i = 61; i < 67; ++i)
            for (int j = 56; j < 72; ++j)
                for (int k = 0; k < 40; ++k) m->at(i, j, k) |= 5;   // occupied (and inflated)
        std::vector<std::vector<pose>> pp;
        for (int i = 0; i < 32; ++i) {
            const double y = -1.6 + 0.12 * i;
            pp.push_back({{-3, y, 1}, {-1, y + 0.3, 1}, {1, y + 0.3, 1}, {3, y, 1}});
        }
        sc.push_back({m, pp});
    }
    for (unsigned s = 1; s <= 3; ++s) sc.push_back({pillarWorld(100 + s, 25), paths(200 + s, 32)});
    int planners = 0, valid = 0;
    for (auto& c : sc) {
        Batch b = make(c.first, c.second);
        std::vector<std::vector<pose>> trajs;
        std::vector<bool> r = polyTrajOctomap::makePlanBatch(b.ps, trajs);
        for (size_t i = 0; i < b.ps.size(); ++i) {
            const int v = r[i] ? 1 : 0, it = b.ps[i]->getIterations();
            put(f, &v, 4);
            put(f, &it, 4);
            putPoses(f, b.ps[i]->getPath());
            putPoses(f, trajs[i]);
            ++planners;
            valid += v;
        }
    }
    std::fclose(f);
    // timing: makePlanBatch of 32 and 1024 planners (fresh planners every repetition) on the pillar geometry of the
    // first scenario, its 32 paths repeated
    auto world = sc[0].first;
    double med[2];
    const int sizes[2] = {32, 1024};
    for (int k = 0; k < 2; ++k) {
        std::vector<std::vector<pose>> pp;
        for (int i = 0; i < sizes[k]; ++i) pp.push_back(sc[0].second[i % 32]);
        std::vector<double> t;
        for (int r = 0; r < reps + 1; ++r) {
            Batch b = make(world, pp);
            std::vector<std::vector<pose>> trajs;
            const auto t0 = std::chrono::steady_clock::now();
            polyTrajOctomap::makePlanBatch(b.ps, trajs);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r > 0) t.push_back(ms);              // the first one warms the handle and the map snapshot up
        }
        std::sort(t.begin(), t.end());
        med[k] = t[t.size() / 2];
    }
    std::printf("{\"planners_dumped\": %d, \"valid\": %d, \"makePlanBatch_32_ms\": %.3f, \"makePlanBatch_1024_ms\": %.3f, \"reps\": %d}\n",
                planners, valid, med[0], med[1], reps);
    return 0;
}
