// poly_batch_dump.cpp — before/after evidence for polyTrajOctomap::makePlanBatch and polyTrajOccMap::makePlanBatch: calls
// only the public facade API, so the same source links against any build of libtrajectory_planner_vigo.so.  Writes, for
// every planner of every scenario, validity, iterations, the final waypoint path (polyTrajOctomap) or the duration
// (polyTrajOccMap) and the returned trajectory as raw bytes to argv[1] (compare two libraries' files with cmp), then times
// makePlanBatch of 32 and 1024 planners of each class (median of argv[2] repetitions, default 3; 0: dump only) and prints
// one JSON line.  Every planner's time limit is far above what a plan takes (both batches allow timeout x planners), so
// no plan ends on the clock and the dump is deterministic: the planners' "Timeout" lines on stdout must count 0.
// Build (GPU box, after `make -C trajectory_planner_amd/host`):
//   hipcc -O2 -std=c++17 -Itrajectory_planner_amd/host/include tools/poly_batch_dump.cpp \
//         -Ltrajectory_planner_amd/lib -ltrajectory_planner_vigo -lvigo_hip -Wl,-rpath,<lib dir> -o poly_batch_dump
#include <trajectory_planner/polyTrajOccMap.h>
#include <trajectory_planner/polyTrajOctomap.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <vector>

using trajPlanner::polyTrajOccMap;
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

// ---- polyTrajOccMap: a sample collides where the map says inflated-occupied AND unknown, so two pillars in three carry
// both bits (the others only the first: no obstacle to this planner) and unknown blocks overlap some of the rest ----
static std::shared_ptr<mapManager::occMap> occWorld(unsigned seed) {
    auto m = std::make_shared<mapManager::occMap>(60, 60, 20, Eigen::Vector3d(-3.0, -3.0, 0.0), 0.1);
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> c(4, 55), w(1, 3), kind(0, 2), cz(0, 19);
    for (int p = 0; p < 25; ++p) {
        const int x = c(rng), y = c(rng), a = w(rng), b = w(rng), bits = kind(rng) == 0 ? 1 : 3;
        for (int i = x - a; i < x + a; ++i)
            for (int j = y - b; j < y + b; ++j)
                for (int k = 0; k < 20; ++k) m->at(i, j, k) |= bits;
    }
    for (int q = 0; q < 6; ++q) {
        const int x = c(rng), y = c(rng), z = cz(rng);
        for (int i = x - 4; i < x + 4; ++i)
            for (int j = y - 4; j < y + 4; ++j)
                for (int k = std::max(z - 4, 0); k < std::min(z + 4, 20); ++k) m->at(i, j, k) |= 2;
    }
    return m;
}

struct OccJob {
    std::vector<pose> path;
    bool soft;          // soft_constraint: the host QP inside the batch
    double cond[12];    // start vel, end vel, start acc, end acc
};

// P seeded jobs of 2-8 waypoints across the world; `mixed`: every 16th one 13 waypoints (beyond the device QP), every 7th
// one with soft constraints, two in three with non-zero end conditions
static std::vector<OccJob> occJobs(unsigned seed, int P, bool mixed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> y(-2.6, 2.6), z(0.4, 1.6), cnd(-0.4, 0.4);
    std::uniform_int_distribution<int> nw(2, 8), side(0, 1);
    std::vector<OccJob> out;
    for (int i = 0; i < P; ++i) {
        OccJob j;
        const int W = mixed && i % 16 == 5 ? 13 : nw(rng);
        const double sgn = side(rng) ? 1.0 : -1.0;
        for (int k = 0; k < W; ++k) {
            const double px = sgn * (-2.6 + 5.2 * k / (W - 1)), py = y(rng), pz = z(rng);
            j.path.push_back(pose(px, py, pz));
        }
        j.soft = mixed && i % 7 == 3;
        for (double& c : j.cond) c = mixed && i % 3 != 0 ? cnd(rng) : 0.0;
        out.push_back(j);
    }
    return out;
}

struct OccBatch {
    std::vector<std::unique_ptr<polyTrajOccMap>> own;
    std::vector<polyTrajOccMap*> ps;
};

// timeout 100 s: the loops end on the iteration limit, never on the clock
static OccBatch makeOcc(const std::shared_ptr<mapManager::occMap>& map, const std::vector<OccJob>& jobs) {
    OccBatch b;
    for (const OccJob& j : jobs) {
        ros::NodeHandle nh;
        nh.setParam("poly_traj/timeout", 100.0);
        nh.setParam("poly_traj/maximum_iteration_num", 8.0);
        nh.setParam("poly_traj/shrinking_factor", 0.75);
        nh.setParam("poly_traj/soft_constraint", j.soft ? 1.0 : 0.0);
        std::unique_ptr<polyTrajOccMap> p(new polyTrajOccMap(nh));
        p->setMap(map);
        nav_msgs::Path msg;
        for (const pose& q : j.path) {
            geometry_msgs::PoseStamped ps;
            ps.pose.position.x = q.x; ps.pose.position.y = q.y; ps.pose.position.z = q.z;
            msg.poses.push_back(ps);
        }
        std::vector<Eigen::Vector3d> c;
        for (int k = 0; k < 4; ++k) c.push_back(Eigen::Vector3d(j.cond[3 * k], j.cond[3 * k + 1], j.cond[3 * k + 2]));
        p->updatePath(msg, c);
        b.own.push_back(std::move(p));
        b.ps.push_back(b.own.back().get());
    }
    return b;
}

// median of `reps` timed runs after one that warms the handle and the map snapshot up; `run` returns its milliseconds
static double medianMs(int reps, const std::function<double()>& run) {
    std::vector<double> t;
    for (int r = 0; r < reps + 1; ++r) {
        const double ms = run();
        if (r > 0) t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
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
    // polyTrajOccMap: three seeded worlds of 32 mixed jobs, with corridors (the plans iterate) and without
    int occPlanners = 0, occValid = 0, occIterated = 0;
    for (unsigned s = 1; s <= 3; ++s)
        for (int corridor = 1; corridor >= 0; --corridor) {
            OccBatch b = makeOcc(occWorld(300 + s), occJobs(400 + s, 32, true));
            std::vector<std::vector<pose>> trajs;
            std::vector<bool> r = polyTrajOccMap::makePlanBatch(b.ps, corridor != 0, &trajs);
            for (size_t i = 0; i < b.ps.size(); ++i) {
                const int v = r[i] ? 1 : 0, it = b.ps[i]->getIterations();
                const double dur = b.ps[i]->getDuration();
                put(f, &v, 4);
                put(f, &it, 4);
                put(f, &dur, 8);
                putPoses(f, trajs[i]);
                ++occPlanners;
                occValid += v;
                occIterated += it > 1;
            }
        }
    std::fclose(f);
    // the JSON line is printed in one piece at the end: the planners write their own messages to stdout meanwhile
    char buf[256];
    std::snprintf(buf, sizeof buf, "{\"planners_dumped\": %d, \"valid\": %d, \"occ_planners_dumped\": %d, \"occ_valid\": %d, \"occ_iterated\": %d",
                  planners, valid, occPlanners, occValid, occIterated);
    std::string json = buf;
    // timing: makePlanBatch of 32 and 1024 planners (fresh planners every repetition).  polyTrajOctomap: the pillar geometry
    // of the first scenario, its 32 paths repeated; polyTrajOccMap: a seeded world, 32 device-QP jobs repeated, corridors on
    if (reps > 0) {
        const auto occMapT = occWorld(301);
        const std::vector<OccJob> occ32 = occJobs(501, 32, false);
        for (int n : {32, 1024}) {
            std::vector<std::vector<pose>> pp;
            std::vector<OccJob> jj;
            for (int i = 0; i < n; ++i) { pp.push_back(sc[0].second[i % 32]); jj.push_back(occ32[i % 32]); }
            const double ms = medianMs(reps, [&] {
                Batch b = make(sc[0].first, pp);
                std::vector<std::vector<pose>> trajs;
                const auto t0 = std::chrono::steady_clock::now();
                polyTrajOctomap::makePlanBatch(b.ps, trajs);
                return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            });
            const double occMs = medianMs(reps, [&] {
                OccBatch b = makeOcc(occMapT, jj);
                std::vector<std::vector<pose>> trajs;
                const auto t0 = std::chrono::steady_clock::now();
                polyTrajOccMap::makePlanBatch(b.ps, true, &trajs);
                return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            });
            std::snprintf(buf, sizeof buf, ", \"makePlanBatch_%d_ms\": %.3f, \"occ_makePlanBatch_%d_ms\": %.3f", n, ms, n, occMs);
            json += buf;
        }
    }
    std::printf("%s, \"reps\": %d}\n", json.c_str(), reps);
    return 0;
}
