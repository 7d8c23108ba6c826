// bsplineTrajBatch.h — internal to bsplineTraj's three sources (bsplineTraj.cpp: the reference port and the single-planner
// device seam; bsplineTrajSeed.cpp: updatePathBatch / seedPathBatch; bsplineTrajBatch.cpp: makePlanBatch and its device
// stages): what they share.
#ifndef VIGO_HOST_BSPLINE_TRAJ_BATCH_H
#define VIGO_HOST_BSPLINE_TRAJ_BATCH_H
#include <trajectory_planner/bsplineTraj.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <iostream>
#include <mutex>

#include "../../../include/vigo.h"
#include "../../../include/vigo_validate.h"
#include "batchLayout.h"
#include "devbuf.h"
#include "workerPool.h"

namespace trajPlanner {

using vigo_host::HostBatch;
using vigo_host::Staged;
using vigo_host::parallelFor;

// The reference keeps the length of the previous call's path in a function-static shared by all instances (BT.cpp:755):
// kept here as one process-wide value, read and written through adjustPathLengthWith so that updatePathBatch can run
// the planners' prologues on several host threads and still hand every planner the value its predecessor left.
// (atomic only so that two host threads planning two batches do not race on it formally; WHICH value a planner of one
// batch sees when another batch runs at the same time is as unspecified as it is for the reference's static)
extern std::atomic<double> g_prevPathLength;

inline double wallSeconds() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the result of a C ABI call of a device stage: VIGO_OK, or the entry's failure on the console
inline bool deviceCallOk(int rc, const char* entry, vigo_handle_t h) {
    if (rc != VIGO_OK) std::cout << "[BsplineTraj]: " << entry << " failed: " << vigo_last_error(h) << std::endl;
    return rc == VIGO_OK;
}

// the end of every batch call: its stats to the caller, when asked for, and onto the process totals (bsplineTraj::batchTotals)
void reportBatchStats(const bsplineTraj::BatchStats& st, bsplineTraj::BatchStats* out);

// BT.cpp:497-511: the segments after the merges of pathSearch
void applyMerges(std::vector<std::pair<int, int>>& collisionSeg, const std::vector<int>& mergeIndices);

#ifdef VIGO_WITH_ROS
// The snapshot of this map type covers the planner's region only, and the device takes everything outside it for occupied
// while the host asks the map itself: what a device stage may read has to lie inside the region.  This is the test:
// the axis-aligned box of the n points xyz (triples), grown by half[k] along axis k, lies inside R, bounds included.
// (No region set, or a NaN coordinate: it does not.  No points: it does.)
inline bool boxInRegion(const mapRegion& R, const double* xyz, size_t n, const double half[3]) {
    if (!R.set) return false;
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (size_t q = 0; q < 3 * n; ++q) {
        const double v = xyz[q];
        if (v < lo[q % 3] || std::isnan(v)) lo[q % 3] = v;       // (a NaN stays: nothing compares below or above it)
        if (v > hi[q % 3] || std::isnan(v)) hi[q % 3] = v;
    }
    for (int k = 0; k < 3; ++k)
        if (!(lo[k] - half[k] >= R.boxMin(k) && hi[k] + half[k] <= R.boxMax(k))) return false;
    return true;
}
#endif

// What the device searches of a group of planners share, from the group's lead: the map's resolution, the A* node pool
// setMap sizes from maxObstacleSize_ (BT.cpp:187-195), the control-point count (the row stride: under mixedPrologue the
// largest count of the planners the group takes).
struct bsplineTraj::SearchGroup {
    double res;
    int32_t pool[3];
    double half[3];        // reach of a search's node pool around the midpoint of its ends: pool / 2 + 1 nodes
    int N;
    bool uniform = true;   // every planner of the group has N control points: the uniform entries apply
    double notCheckRatio;
    explicit SearchGroup(const bsplineTraj& lead)
        : res(lead.link_.map()->getRes()), N(lead.optData_.controlPoints.cols()), notCheckRatio(lead.notCheckRatio_) {
        for (int k = 0; k < 3; ++k) {
            pool[k] = 2 * int(lead.maxObstacleSize_(k) / res);
            half[k] = (pool[k] / 2 + 1) * res;
        }
    }
    // the ranges the device entries take: the pool's always, with `scan` vigo_path_search's for the segment scan too
    bool valid(bool scan) const {
        for (int k = 0; k < 3; ++k)
            if (pool[k] < 3 || pool[k] > VIGO_ASTAR_MAX_POOL_AXIS) return false;
        return !scan || (N >= 7 && notCheckRatio >= 0.0 && notCheckRatio <= 1.0);
    }
    // x and y may share such a group: a device batch and a node pool; `mixed` (BatchOptions::mixedPrologue): whatever
    // their counts inside a shape class, as the mixed solves group them
    static bool same(const bsplineTraj& x, const bsplineTraj& y, bool mixed = false) {
        return x.sameSolveGroup(y, mixed) && x.maxObstacleSize_(0) == y.maxObstacleSize_(0) && x.maxObstacleSize_(1) == y.maxObstacleSize_(1) &&
               x.maxObstacleSize_(2) == y.maxObstacleSize_(2);
    }
    // May the device search for p among the n points xyz?  Every node pool around a midpoint of two of them, and with it
    // every path point, lies in the points' box grown by the pool's reach: a map type whose snapshot covers p's region
    // only (boxInRegion) must hold that box; the in-tree dense map is snapshotted whole.
    bool inReach(const bsplineTraj& p, const double* xyz, size_t n) const {
#ifdef VIGO_WITH_ROS
        return boxInRegion(p.link_.region(), xyz, n, half);
#else
        (void)p; (void)xyz; (void)n;
        return true;
#endif
    }
    // The opening of a device stage over ps[owners[..]]: fn(lead, g, who) per group (`same`) whose lead syncs its device
    // and whose ranges are valid(scan), who = the group's entries of owners in order — with `scan` (the stage reads the
    // planners' control points) those with their control points inReach.  A group that fails any of this, or is left
    // empty, is skipped: its planners stay with the host steps.  `mixed`: groups of mixed counts (same); g.N is then the
    // largest count of `who` and g.uniform says whether the counts differ at all.
    template <class Fn>
    static void forEach(const std::vector<bsplineTraj*>& ps, const std::vector<size_t>& owners, bool scan, bool mixed, Fn fn) {
        auto sameGroup = [&](size_t a, size_t b) { return same(*ps[owners[a]], *ps[owners[b]], mixed); };
        vigo_host::forEachGroup(owners.size(), sameGroup, [&](const std::vector<size_t>& members) {
            bsplineTraj* lead = ps[owners[members[0]]];
            if (!lead->syncDevice()) return;
            SearchGroup g(*lead);
            if (!g.valid(scan)) return;
            std::vector<size_t> who;
            for (size_t m : members) {
                const Eigen::MatrixXd& c = ps[owners[m]]->optData_.controlPoints;
                if (!scan || g.inReach(*ps[owners[m]], c.data(), (size_t)c.cols())) who.push_back(owners[m]);
            }
            if (who.empty()) return;
            for (size_t i : who) {
                const int n = (int)ps[i]->optData_.controlPoints.cols();
                g.uniform = g.uniform && n == (int)ps[who[0]]->optData_.controlPoints.cols();
                g.N = i == who[0] ? n : std::max(g.N, n);
            }
            fn(lead, g, who);
        });
    }
};

// the calling thread's staging buffers of a HostBatch's lists, one set for every stage that stages one (costGrad,
// solveBatch, deviceRounds, reguideOnDevice): the thread's next upload overwrites them
struct BatchStage {
    Staged<double> ctrl, gpv, obs, weights;
    Staged<int32_t> goff, ooff, npts;
    Staged<uint8_t> gunk;
};
BatchStage& batchStage();

// device pointers to a HostBatch's lists; an empty guide or obstacle list is null (vigo.h: "no guides" / "no obstacles")
struct DeviceBatch {
    double* ctrl;
    const int32_t* goff;
    const double* gpv;
    const uint8_t* gunk;
    const int32_t* ooff;
    const double* obs;
    double* weights;
    const int32_t* npts;     // null: every trajectory fills its row (HostBatch::uniform), the uniform entries apply
};

// hb into the calling thread's staging buffers, then map_->isUnknown(guidePoint) (BT.cpp:841) for its guides, hoisted
// out of the solve.  The buffers live across calls (hipMalloc/hipFree per rebound round cost more than the round's
// kernels): the thread's next upload overwrites them, so what a call reads back is read back before that.
bool uploadBatch(vigo_handle_t h, const HostBatch& hb, DeviceBatch& d);

// one unsplit makePlanBatch call: its options, what its stages did so far (written by the calling thread only), per planner
// (index into the call's planners) its loop state and result; the planners still in the loop, in call order, with their indices
struct bsplineTraj::PlanBatch {
    const BatchOptions o;
    BatchStats stats;
    std::mutex logMutex;                                       // o.reguideStepLog: the workers append
    std::vector<Rebound> rb;
    std::vector<bool> result;
    std::vector<bsplineTraj*> active;
    std::vector<size_t> activeIdx;
    std::atomic<long long> nsSeg{0}, nsAstar{0}, nsGuide{0};   // prologue CPU time summed over the worker threads
    std::atomic<long long> nsChain{0};                         // devicePrologue: wall time of the device chains (all three steps)
    PlanBatch(size_t P, const BatchOptions& options) : o(options), rb(P), result(P, false) {}
    // step 1 of planner p and, with `search`, step 2 on the calling worker, timed; false: its A* failed
    bool hostSteps(bsplineTraj* p, bool search) {
        const double t0 = wallSeconds();
        p->findCollisionSeg(p->optData_.controlPoints, p->collisionSeg_);           // step 1
        const double t1 = wallSeconds();
        nsSeg += (long long)((t1 - t0) * 1e9);
        if (!search) return true;
        const bool found = p->pathSearch(p->collisionSeg_, p->astarPaths_);         // step 2
        nsAstar += (long long)((wallSeconds() - t1) * 1e9);
        return found;
    }
};

// one AstarSearch(res, pStart, pEnd) of planner `planner`: from the start of segment `seg` to the end of segment `endSeg`
struct bsplineTraj::AstarJob {
    size_t planner;
    int seg, endSeg;
    Eigen::Vector3d s, e;
    bool ok = false;                       // AstarSearch's return value
    std::vector<Eigen::Vector3d> path;     // getPath()
};

}  // namespace trajPlanner
#endif  /* VIGO_HOST_BSPLINE_TRAJ_BATCH_H */
