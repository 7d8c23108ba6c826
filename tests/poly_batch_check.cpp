// poly_batch_check.cpp — a program of its own (built by test_poly_batch_loop.py with the address and undefined-behaviour
// sanitizers; no GPU, no device library): the lock-step loop of the min-snap planners' makePlanBatch
// (host/src/polyBatchLoop.h) driven for polyTrajOccMap with SCRIPTED steps in place of the two device steps, so that the
// branches a healthy device never takes are run: a QP status of -1 or -2, a candidate the check rejects, a check call that
// fails mid-batch, the time limit.  The QP step solves every member with the host QP (a scratch polyTrajSolver); the check
// step is the planner's own host rule (checkCollisionTraj: isInflatedOccupied && isUnknown per sample, then
// collisionSegments).  Expected values: each planner's twin planned alone by makePlan(trajectory, corridor), the
// reference loop on the host.  Compared bit for bit per planner: verdict, getIterations(), the trajectory, getDuration().
// Exit status 0 and a last line "ok: ..." when every scenario holds.
#include <trajectory_planner/polyTrajOccMap.h>

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../include/vigo.h"
#include "../trajectory_planner_amd/host/src/polyBatchLoop.h"

using trajPlanner::polyTrajOccMap;
using trajPlanner::pose;

// ---- the device and HIP entry points the planner sources name: this program must never reach one ----
[[noreturn]] static void deviceCall(const char* what) {
    std::fprintf(stderr, "poly_batch_check: %s was called: the scripted steps must keep the loop off the device\n", what);
    std::abort();
}
extern "C" {
int vigo_create(vigo_handle_t*, int) { deviceCall("vigo_create"); }
int vigo_destroy(vigo_handle_t) { deviceCall("vigo_destroy"); }
int vigo_set_stream(vigo_handle_t, void*) { deviceCall("vigo_set_stream"); }
int vigo_set_params(vigo_handle_t, const vigo_params_t*) { deviceCall("vigo_set_params"); }
int vigo_set_grid_host(vigo_handle_t, int, int, int, const double*, double, const uint8_t*) { deviceCall("vigo_set_grid_host"); }
const char* vigo_last_error(vigo_handle_t) { deviceCall("vigo_last_error"); }
int vigo_minsnap_supported(int, int, int, int) { deviceCall("vigo_minsnap_supported"); }
int vigo_minsnap(vigo_handle_t, int, int, int, int, int, double, double, const double*, const double*, const double*, double*, double*,
                 int32_t*) { deviceCall("vigo_minsnap"); }
int vigo_traj_point_check(vigo_handle_t, int, int, int, const int32_t*, const double*, const double*, const double*, const double*,
                          int32_t*, int32_t*, uint8_t*, int32_t*, int32_t*, uint8_t*) { deviceCall("vigo_traj_point_check"); }
hipError_t hipSetDevice(int) { deviceCall("hipSetDevice"); }
hipError_t hipGetDevice(int*) { deviceCall("hipGetDevice"); }
hipError_t hipMalloc(void**, size_t) { deviceCall("hipMalloc"); }
hipError_t hipFree(void*) { deviceCall("hipFree"); }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { deviceCall("hipMemcpyAsync"); }
hipError_t hipStreamCreateWithFlags(hipStream_t*, unsigned int) { deviceCall("hipStreamCreateWithFlags"); }
hipError_t hipStreamSynchronize(hipStream_t) { deviceCall("hipStreamSynchronize"); }
}

ros::Time ros::Time::now() { return ros::Time(); }   // (the in-tree stand-in's clock lives in bsplineTraj.cpp, which is not part of this program)

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            ++g_failures;                                  \
            std::printf("FAILED %s: ", #cond);             \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
        }                                                  \
    } while (0)

// ---- the world: 16^3 voxels of 0.5 m, a few boxes that are inflated-occupied AND unknown (the planner's collision rule) ----
std::shared_ptr<mapManager::occMap> makeMap() {
    auto map = std::make_shared<mapManager::occMap>(16, 16, 16, Eigen::Vector3d(0, 0, 0), 0.5);
    const int boxes[3][6] = {{7, 9, 0, 9, 0, 16}, {3, 5, 11, 13, 0, 16}, {11, 13, 6, 8, 0, 16}};   // x0 x1 y0 y1 z0 z1 (voxels)
    for (const auto& b : boxes)
        for (int x = b[0]; x < b[1]; ++x)
            for (int y = b[2]; y < b[3]; ++y)
                for (int z = b[4]; z < b[5]; ++z) map->at(x, y, z) = 1u | 2u | 4u;
    return map;
}

struct Spec {
    std::vector<pose> path;
    int degree;
    bool soft;
};

struct Knobs {   // what a scenario sets for every planner
    double timeout = 1e9;
    int maxIter = 6;
    bool pwl = true;
};

std::unique_ptr<polyTrajOccMap> makePlanner(const std::shared_ptr<mapManager::occMap>& map, const Spec& s, const Knobs& k) {
    ros::NodeHandle nh;
    nh.setParam("poly_traj/polynomial_degree", (double)s.degree);
    nh.setParam("poly_traj/soft_constraint", s.soft ? 1.0 : 0.0);
    nh.setParam("poly_traj/timeout", k.timeout);
    nh.setParam("poly_traj/maximum_iteration_num", (double)k.maxIter);
    nh.setParam("poly_traj/use_pwl_failsafe", k.pwl ? 1.0 : 0.0);
    std::unique_ptr<polyTrajOccMap> p(new polyTrajOccMap(nh));
    p->setMap(map);
    p->updatePath(s.path);
    return p;
}

struct Outcome {
    bool verdict = false;
    int iterations = 0;
    std::vector<pose> traj;
    double duration = 0;
};

bool sameBits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }
bool sameTraj(const std::vector<pose>& a, const std::vector<pose>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!sameBits(a[i].x, b[i].x) || !sameBits(a[i].y, b[i].y) || !sameBits(a[i].z, b[i].z) || !sameBits(a[i].yaw, b[i].yaw)) return false;
    return true;
}

Outcome solo(const std::shared_ptr<mapManager::occMap>& map, const Spec& s, const Knobs& k, bool corridor) {
    auto p = makePlanner(map, s, k);
    Outcome o;
    o.verdict = p->makePlan(o.traj, corridor);
    o.iterations = p->getIterations();
    o.duration = p->getDuration();
    return o;
}

// ---- the scripted steps.  Positions are (planner index in the call, round counted from 1) ----
typedef std::pair<int, int> At;
struct Script {
    std::map<At, int> qpStatus;   // the QP step answers this status (-1, -2) instead of solving
    std::set<At> rejected;        // the check step answers VIGO_TRAJ_STALL instead of a verdict
    int failedCheckRound = 0;     // the whole check step fails in this round
};

struct ScriptedSteps {
    const Script& script;
    const std::vector<polyTrajOccMap*>& planners;   // of the call
    const std::vector<int>& group;                  // group member g -> its index in the call
    int round = 1, groups = 0, hits = 0;
    std::set<int> groupSizes;                       // waypoint counts that formed a QP group in round 1
    ScriptedSteps(const Script& s, const std::vector<polyTrajOccMap*>& ps, const std::vector<int>& g) : script(s), planners(ps), group(g) {}

    bool ready(polyTrajOccMap*) { return true; }
    bool supported(int W, int, int) const { return W >= 2 && W <= 11; }
    bool solve(int diff, int cont, double vel, double corridorRes, std::vector<vigo_host::QpMember>& qp) {
        ++groups;
        if (round == 1) groupSizes.insert((int)qp[0].path->size());
        for (vigo_host::QpMember& m : qp) {
            const auto scripted = script.qpStatus.find(At(group.at(m.who), round));
            if (scripted != script.qpStatus.end()) {
                m.status = scripted->second;
                ++hits;
                continue;
            }
            trajPlanner::polyTrajSolver s(7, diff, cont, vel);
            s.updatePath(*m.path);
            if (m.conds[0]) {
                s.updateInitVel(m.conds[0]->linear.x, m.conds[0]->linear.y, m.conds[0]->linear.z);
                s.updateEndVel(m.conds[1]->linear.x, m.conds[1]->linear.y, m.conds[1]->linear.z);
                s.updateInitAcc(m.conds[2]->linear.x, m.conds[2]->linear.y, m.conds[2]->linear.z);
                s.updateEndAcc(m.conds[3]->linear.x, m.conds[3]->linear.y, m.conds[3]->linear.z);
            }
            if (m.corridor) s.setCorridorConstraint(*m.corridor, corridorRes);
            s.solve();
            m.status = s.hasSolution() ? 0 : -2;
            for (int ax = 0; ax < 3 && m.status == 0; ++ax) m.sol[ax] = s.getSolution(ax);
        }
        return true;
    }
    bool check(std::vector<vigo_host::TrajCheck>& cand) {
        const int r = round++;
        if (r == script.failedCheckRound) { ++hits; return false; }
        for (vigo_host::TrajCheck& c : cand) {
            const int who = group.at(c.who);
            if (script.rejected.count(At(who, r))) {
                c.status = VIGO_TRAJ_STALL;
                ++hits;
                continue;
            }
            std::vector<pose> traj;
            c.solver->getTrajectory(traj, c.delT);
            c.status = VIGO_TRAJ_OK;
            c.collides = planners[who]->checkCollisionTraj(traj, c.delT, c.segments);
        }
        return true;
    }
    const char* lastError() const { return "scripted failure of the check step"; }
};

struct Run {
    std::vector<Outcome> got;
    int groupsRound1 = 0;
};

// the batch of one scenario; `inBatch[i]`: the loop is expected to take planner i (two or more waypoints, degree 7)
Run batch(const std::shared_ptr<mapManager::occMap>& map, const std::vector<Spec>& specs, const Knobs& k, bool corridor, const Script& script,
          const char* name) {
    std::vector<std::unique_ptr<polyTrajOccMap>> own;
    std::vector<polyTrajOccMap*> ps;
    std::vector<int> group;
    for (size_t i = 0; i < specs.size(); ++i) {
        own.push_back(makePlanner(map, specs[i], k));
        ps.push_back(own.back().get());
        if (specs[i].path.size() >= 2 && specs[i].degree == 7) group.push_back((int)i);
    }
    ScriptedSteps steps(script, ps, group);
    std::vector<std::vector<pose>> out;
    const std::vector<bool> verdicts = vigo_host::LockStepBatch<polyTrajOccMap>::run(ps, corridor, out, steps);
    const int scripted = (int)script.qpStatus.size() + (int)script.rejected.size() + (script.failedCheckRound ? 1 : 0);
    CHECK(steps.hits == scripted, "%s: %d of %d scripted positions were reached", name, steps.hits, scripted);
    Run r;
    r.groupsRound1 = (int)steps.groupSizes.size();
    for (size_t i = 0; i < specs.size(); ++i) {
        Outcome o;
        o.verdict = verdicts[i];
        CHECK(ps[i]->isValid() == o.verdict, "%s: planner %zu isValid() against the returned verdict", name, i);
        o.iterations = ps[i]->getIterations();
        o.traj = out[i];
        o.duration = ps[i]->getDuration();
        r.got.push_back(o);
    }
    return r;
}

void expectEqual(const char* name, size_t i, const Outcome& got, const Outcome& want) {
    CHECK(got.verdict == want.verdict, "%s: planner %zu verdict %d, alone %d", name, i, (int)got.verdict, (int)want.verdict);
    CHECK(got.iterations == want.iterations, "%s: planner %zu iterations %d, alone %d", name, i, got.iterations, want.iterations);
    CHECK(sameTraj(got.traj, want.traj), "%s: planner %zu trajectory (%zu samples, alone %zu)", name, i, got.traj.size(), want.traj.size());
    CHECK(sameBits(got.duration, want.duration), "%s: planner %zu duration %.17g, alone %.17g", name, i, got.duration, want.duration);
}

}  // namespace

int main() {
    const auto map = makeMap();
    // planners 0-5: paths of 2, 3 and 4 waypoints; 6: a soft constraint (in the batch, but every round on the host QP);
    // 7: one waypoint, 8: another polynomial degree — both outside the batch
    const std::vector<Spec> specs = {
        {{pose(1, 1, 2), pose(6.5, 1.5, 2)}, 7, false},                                      // straight through a box: never valid
        {{pose(1, 6, 2), pose(3, 7.2, 2.5)}, 7, false},                                      // free
        {{pose(1, 2, 2), pose(2.8, 5.2, 2), pose(6, 5.5, 2)}, 7, false},
        {{pose(5, 7, 1), pose(6.2, 4.6, 1.5), pose(7.4, 6.8, 2)}, 7, false},
        {{pose(1, 1, 3), pose(3.2, 2.2, 3), pose(3.1, 5.0, 3), pose(6.5, 5.6, 3)}, 7, false},
        {{pose(6.5, 1, 1), pose(6.2, 2.6, 1), pose(4.6, 3.0, 1.5), pose(5.0, 5.5, 2)}, 7, false},
        {{pose(2.5, 7.5, 2), pose(2.9, 5.0, 2), pose(6, 4.8, 2)}, 7, true},
        {{pose(2, 2, 2)}, 7, false},
        {{pose(1, 6.5, 1), pose(3, 7.0, 1), pose(3.5, 7.5, 1.5)}, 5, false},
    };
    const size_t P = specs.size();
    const Knobs usual;
    std::vector<Outcome> alone[2];   // [corridor]
    for (int c = 0; c < 2; ++c)
        for (const Spec& s : specs) alone[c].push_back(solo(map, s, usual, c != 0));

    // what the inputs must show before anything is concluded from them: with corridors, a planner that needs two or more
    // rounds and ends valid, one valid in the first round, one that never is
    int later = -1, first = -1, never = -1;
    for (int i = 0; i < 6; ++i) {
        const Outcome& o = alone[1][i];
        if (o.verdict && o.iterations >= 2 && later < 0) later = i;
        if (o.verdict && o.iterations == 1 && first < 0) first = i;
        if (!o.verdict && o.iterations >= 2 && never < 0) never = i;
    }
    for (size_t i = 0; i < P; ++i)
        std::printf("alone, corridors: planner %zu verdict %d after %d solves, %zu samples\n", i, (int)alone[1][i].verdict,
                    alone[1][i].iterations, alone[1][i].traj.size());
    CHECK(later >= 0 && first >= 0 && never >= 0, "the inputs show no planner valid at once / valid later / never valid (%d %d %d)", first, later, never);
    if (g_failures) return 1;
    const int laterRound = alone[1][later].iterations;

    struct Scenario {
        const char* name;
        bool corridor;
        Script script;
    };
    std::vector<Scenario> scenarios;
    scenarios.push_back({"no script, corridors", true, {}});
    scenarios.push_back({"no script, no corridors", false, {}});
    for (int status : {-1, -2}) {
        Script a, b, c;
        a.qpStatus[At(later, 1)] = status;
        a.qpStatus[At(first, 1)] = status;
        b.qpStatus[At(later, laterRound)] = status;
        b.qpStatus[At(never, 2)] = status;
        c.qpStatus[At(first, 1)] = status;
        scenarios.push_back({status == -1 ? "QP status -1 in round 1" : "QP status -2 in round 1", true, a});
        scenarios.push_back({status == -1 ? "QP status -1 in a later round" : "QP status -2 in a later round", true, b});
        scenarios.push_back({status == -1 ? "QP status -1, no corridors" : "QP status -2, no corridors", false, c});
    }
    {
        Script a, b;
        a.rejected.insert(At(later, 1));
        a.rejected.insert(At(first, 1));
        b.rejected.insert(At(later, laterRound));
        b.rejected.insert(At(never, 3));
        scenarios.push_back({"rejected candidates in round 1", true, a});
        scenarios.push_back({"rejected candidates in later rounds", true, b});
    }
    for (const Scenario& sc : scenarios) {
        const Run r = batch(map, specs, usual, sc.corridor, sc.script, sc.name);
        CHECK(r.groupsRound1 >= 2, "%s: %d QP groups formed in round 1", sc.name, r.groupsRound1);
        for (size_t i = 0; i < P; ++i) expectEqual(sc.name, i, r.got[i], alone[sc.corridor][i]);
    }

    {   // the time limit: nobody solves anything
        const char* name = "timeout 0";
        Knobs k;
        k.timeout = 0.0;
        for (int c = 0; c < 2; ++c) {
            const Run r = batch(map, specs, k, c != 0, Script(), name);
            for (size_t i = 0; i < P; ++i) {
                const Outcome want = solo(map, specs[i], k, c != 0);
                expectEqual(name, i, r.got[i], want);
                const bool single = specs[i].path.size() == 1;
                CHECK(r.got[i].verdict == single && r.got[i].iterations == 0, "%s: planner %zu verdict %d after %d solves", name, i,
                      (int)r.got[i].verdict, r.got[i].iterations);
            }
        }
    }

    {   // the check step fails in round 2.  Planners valid in round 1, and those outside the batch, keep what they plan
        // alone; the others report not found after one counted round, with the trajectory of their last polynomial — the
        // second round's, which a twin limited to maximum_iteration_num = 1 samples as well (its second solve is its last)
        const char* name = "failed check step in round 2";
        Knobs k, twin;
        k.pwl = twin.pwl = false;
        twin.maxIter = 1;
        Script s;
        s.failedCheckRound = 2;
        const Run r = batch(map, specs, k, true, s, name);
        int kept = 0, cut = 0;
        for (size_t i = 0; i < P; ++i) {
            const Outcome whole = solo(map, specs[i], k, true);
            const bool outside = specs[i].path.size() < 2 || specs[i].degree != 7;
            if (outside || whole.iterations <= 1) {
                expectEqual(name, i, r.got[i], whole);
                ++kept;
                continue;
            }
            const Outcome two = solo(map, specs[i], twin, true);
            CHECK(two.iterations == 2, "%s: planner %zu's limited twin solved %d times", name, i, two.iterations);
            CHECK(!r.got[i].verdict && r.got[i].iterations == 1, "%s: planner %zu verdict %d after %d counted rounds", name, i,
                  (int)r.got[i].verdict, r.got[i].iterations);
            CHECK(!r.got[i].traj.empty() && sameTraj(r.got[i].traj, two.traj), "%s: planner %zu trajectory (%zu samples, twin %zu)", name, i,
                  r.got[i].traj.size(), two.traj.size());
            CHECK(sameBits(r.got[i].duration, two.duration), "%s: planner %zu duration", name, i);
            ++cut;
        }
        CHECK(kept >= 3 && cut >= 2, "%s: %d planners kept their plan, %d were cut off", name, kept, cut);
    }

    if (g_failures) {
        std::printf("%d checks FAILED\n", g_failures);
        return 1;
    }
    std::printf("ok: %zu scripted scenarios + the time limit + a failed check step, %zu planners each\n", scenarios.size(), P);
    return 0;
}
