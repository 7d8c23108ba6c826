/*
 * bsplineTraj.h — trajPlanner::bsplineTraj with the reference's public interface
 * (include/trajectory_planner/bsplineTraj.h:87-158) over the MI355X back-end (include/vigo.h).
 *
 * Host side (this class): path conditioning, B-spline fit, collision-segment bookkeeping, A*,
 * guide assignment, the rebound loop's decisions, time re-parameterisation, getters.
 * Device side (libvigo_hip.so): optimize() = vigo_optimize, the rebound-loop gates
 * (vigo_traj_collision / vigo_traj_dynamic_collision), isUnknown(guide) = vigo_guides_unknown.
 *
 * makePlan() runs one planner (B = 1, link compatibility); makePlanBatch() runs the rebound loops
 * of many planners in lock-step so that every optimize() of the batch is ONE kernel launch —
 * that is the configuration the device is built for.
 */
#ifndef BSPLINETRAJ_H
#define BSPLINETRAJ_H
#include <trajectory_planner/bspline.h>
#include <trajectory_planner/compat.h>
#include <trajectory_planner/mapAdapter.h>
#include <trajectory_planner/path_search/astarOcc.h>
#include <trajectory_planner/utils.h>

#include <memory>
#include <utility>
#include <string>
#include <vector>

const int bsplineDegree = 3;
struct vigo_context;
struct vigo_params_s;

namespace trajPlanner {
struct optData {
    Eigen::MatrixXd controlPoints;
    std::vector<std::vector<Eigen::Vector3d>> guidePoints;
    std::vector<std::vector<Eigen::Vector3d>> guideDirections;
    std::vector<bool> findGuidePoint;
    std::vector<Eigen::Vector3d> dynamicObstaclesPos;
    std::vector<Eigen::Vector3d> dynamicObstaclesVel;
    std::vector<Eigen::Vector3d> dynamicObstaclesSize;
};

class polyTrajOccMap;

class bsplineTraj {
private:
    ros::NodeHandle nh_;
    double controlPointDistance_ = 0.25;  // bsplineTraj.h:46
    double controlPointsTs_ = 0.2;        // bsplineTraj.h:47
    trajPlanner::bspline bspline_;
    trajPlanner::optData optData_;
    double ts_, dthresh_, maxVel_, maxAcc_;
    double weightDistance_, weightSmoothness_, weightFeasibility_, weightDynamicObstacle_;
    double notCheckRatio_ = 0.0;
    bool planInZAxis_;
    double minHeight_, maxHeight_, uncertainAwareFactor_, predHorizon_, distThreshDynamic_, maxPathLength_;
    Eigen::Vector3d maxObstacleSize_;
    std::shared_ptr<AStar> pathSearch_;
    std::vector<std::pair<int, int>> collisionSeg_;
    std::vector<std::vector<Eigen::Vector3d>> astarPaths_;
    bool init_ = false;
    double linearFactor_ = 1.0;
    std::vector<Eigen::Vector3d> inputPathVis_;

    // device
    DeviceLink link_;                  // the map, its snapshot on the handle, the handle (mapAdapter.h)
    int lastStatus_ = 0;
    bool syncDevice();   // params + map snapshot -> handle; false when no GPU / HIP failure

    // per-planner state of the rebound loop (BT.cpp:611-685) so makePlanBatch can interleave planners
    struct Rebound {
        double w0 = 0, wo0 = 0;
        int failCount = 0;
        bool done = false, ok = false, needOptimize = true;
        // filled by the device-resident rounds (vigo_rebound_rounds) for the host's part of the loop
        int devStatus = 0;
        bool gateStatic = false, gateDynamic = false;
    };

public:
    bsplineTraj();
    bsplineTraj(const ros::NodeHandle& nh);
    ~bsplineTraj();
    bsplineTraj(const bsplineTraj&) = delete;
    bsplineTraj& operator=(const bsplineTraj&) = delete;
    void init(const ros::NodeHandle& nh);
    void initParam();
    void setMap(const std::shared_ptr<mapManager::occMap>& map);
    /* not in the reference: the box of the map the device snapshot covers (needed for a map type that offers no bulk
     * access, see mapAdapter.h; ignored by the in-tree dense map) and the request to re-snapshot a map that changed */
    void setMapRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);
    void refreshMap();
    /* ... that changed inside this metric box only: a snapshot that was current gets the box alone (mapAdapter.h) */
    void refreshMap(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);
    /* not in the reference: the HIP device ordinal this planner's back-end handle lives on (default 0); call it before
     * the first plan, or later to move the planner (the handle is re-created and the map uploaded again) */
    void setDevice(int ordinal);
    void updateMaxVel(double maxVel);
    void updateMaxAcc(double maxAcc);
    bool inputPathCheck(const nav_msgs::Path& path, nav_msgs::Path& adjustedPath, double dt, double& finalTime);
    bool fillPath(const nav_msgs::Path& path, nav_msgs::Path& adjustedPath);
    bool updatePath(const nav_msgs::Path& adjustedPath, const std::vector<Eigen::Vector3d>& startEndConditions);
    void updateDynamicObstacles(const std::vector<Eigen::Vector3d>& obstaclesPos, const std::vector<Eigen::Vector3d>& obstaclesVel,
                                const std::vector<Eigen::Vector3d>& obstaclesSize);

    bool makePlan();
    bool makePlan(nav_msgs::Path& trajectory, bool yaw = true);

    /* added (tests, cabiPlanBatch.cpp: vigo_host_plan_batch): the inputs of one re-guide step the workers' twin runs
     * (BatchOptions::reguideStepLog), so the same steps can be put to the kernels' host twin afterwards */
    struct ReguideStepRecord {
        int N;
        std::vector<double> ctrl, gpv;
        std::vector<int32_t> goff, seg;          /* seg: collisionSeg_ as (first, second) pairs */
        int failCount, gateDynamic;
        double weights[4];
    };

    /* ---- the batch calls: makePlanBatch, finishBatch, updatePathBatch, seedPathBatch ------------------------------
     * Which opt-in device stages a batch call uses is a value of the call: a BatchOptions.  The call reads it once, at
     * entry (normalized()), and hands it by value to everything it runs, the companion threads of a pipelined call
     * included; what its stages did comes back as the call's own BatchStats.  Two calls on two host threads, each with
     * its own planners, therefore neither change each other's route nor see each other's counts.  Under every option a
     * planner's result is the same bits, except where a field says otherwise (the last places of atan2). */
    struct BatchOptions {
        /* The A* searches of makePlanBatch's prologue as ONE vigo_astar_search launch per device group (plus one for the
         * merged retries of the failures) instead of host searches on the worker threads.  Same plans: a search the
         * device defers (its budgets, deviceAstarBudget), and every search of a planner whose handle has no map
         * snapshot, is run by the host A*.  The A* of a re-guide inside the rebound loop is deviceReguide's. */
        bool deviceAstar = false;
        /* max_expansions of the device searches of every stage (pops per search before the device hands the search
         * back); negative values count as 0 */
        int deviceAstarBudget = 16384;
        /* Step 3 of makePlanBatch's prologue (assignGuidePointsSemiCircle).  0: the host step as it always was.
         * 1: ONE vigo_guide_assign launch per device group; a planner the device defers (a path longer than
         * vigo_guide_capacity), or whose group has no device or snapshot, runs the same code on the worker threads —
         * csrc/vigo_guide_core.hpp with its portable atan2, the kernel's bit-exact twin — so a planner's guides do not
         * depend on which side produced them.  2: every planner runs that twin on the workers (the emulation of 1).
         * Settings 1 and 2 differ from 0 by the last places of atan2 (vigo.h: vigo_guide_assign); any other value
         * counts as 0.  The re-guide step inside the rebound loop does not consult this field: it is deviceReguide's. */
        int deviceGuides = 0;
        /* The whole prologue of makePlanBatch (steps 1-3) as ONE device chain per group of planners that share a batch
         * key: control points up, vigo_path_search (findCollisionSeg, the A* searches, pathSearch's merge rules) and
         * vigo_guide_assign on its output, one download; collisionSeg_, astarPaths_ and the guide pairs are then
         * installed where the host steps put them.  When on, deviceAstar / deviceGuides are not consulted.  A planner
         * either call defers, one whose merges leave more paths than segments (the device returns the bounded lists
         * only), and every planner of a group without device or snapshot run host steps 1-3 on the workers with the
         * guide step's bit-exact twin (as deviceGuides = 1 does for what the device defers): a plan does not depend on
         * which side ran it.  A planner whose path search FAILS on the device takes the "Fail because of A* failure"
         * path after replaying host steps 1-2 on the workers: vigo_path_search returns nothing for it, and the host
         * steps leave the scanned segments and the paths found before the failure in getCollisionSeg() /
         * getAstarPaths(), so these read the same under every setting.  Searches run under deviceAstarBudget.  The
         * re-guide step inside the rebound loop is not part of the chain: deviceReguide puts it on the device. */
        bool devicePrologue = false;
        /* The re-guide step of the device-resident rebound loop (the `if (hasCollision)` block of BT.cpp:656-679) for
         * the planners vigo_rebound_rounds hands back with a static collision and failCount < 4.  0: reboundStep on the
         * workers, as it always was.  1: ONE vigo_rebound_reguide call per device group on the group's staged batch;
         * collisionSeg_, the appended guide pairs, astarPaths_, the weights, failCount and needOptimize are installed
         * from its outputs (through the host: the batch is packed again for the next vigo_rebound_rounds call).  A
         * planner the call defers, and every planner of a group without device or snapshot, runs the same step on the
         * workers with the guide step's bit-exact twin, so a plan does not depend on which side ran the step.  2: every
         * such planner runs that twin on the workers (the emulation of 1).  Settings 1 and 2 differ from 0 by the last
         * places of atan2; any other value counts as 0.  The forced A* of failCount >= 4 (BT.cpp:640-654), a planner
         * with a dynamic collision only, and the 30 ms budget's exit stay with reboundStep on the host under every
         * setting.  Searches run under deviceAstarBudget.  Only consulted when deviceResidentRebound. */
        int deviceReguide = 0;
        /* The rebound loop of BT.cpp:611-685 runs on the device between two A* calls (vigo_rebound_rounds), or, when
         * false, round by round from the host (the round-1 path, kept for comparison: identical control points) */
        bool deviceResidentRebound = true;
        /* Planners of DIFFERENT control-point counts in one device batch of the solves and of the device-resident
         * rebound rounds: vigo_optimize_mixed / vigo_rebound_rounds_mixed.  Off: one device batch per distinct count.
         * On: planners that share everything but the count share a batch when their counts lie in one shape class of the
         * kernels — all 7 .. 32, or all 33 .. 64; counts above 64 keep a batch per count.  A group whose counts are all
         * equal calls the uniform entry, so a workload of one count runs the same kernels under either setting
         * (include/vigo.h, "mixed control-point counts").  The gates, costGrad and the host-driven loop's gates keep their
         * grouping by exact count; so do the opt-in device stages (A*, guide launch, prologue chain, re-guide) unless
         * mixedPrologue regroups them. */
        bool mixedBatches = false;
        /* The opt-in device stages around the solves — the devicePrologue chain, the deviceGuides = 1 launch, the
         * deviceAstar launches and the deviceReguide = 1 call — group their planners as the mixed solves do
         * (sameSolveGroup(other, true): everything but the count shared, the counts in one shape class, 7 .. 32 or
         * 33 .. 64) instead of by exact count.  Rows are padded to the group's largest count and the stage calls its
         * _mixed entry (vigo_path_search_mixed, vigo_guide_assign_mixed, vigo_rebound_reguide_mixed; the A* launch has no
         * count at all); a group whose counts are all equal calls the uniform entry, as mixedBatches does.  Deferred,
         * failed and no-device planners take the host routes they take when this is off, and a plan does not depend on
         * the setting: fewer device groups open (BatchStats::prologueGroups, reguideGroups). */
        bool mixedPrologue = false;
        /* Steps 5-6 of makePlan() (the spline object, linearFeasibilityReparam) and, for the calls with trajectories, the
         * samples of evalTrajToMsg.  Off: per planner on the host workers, as it always was.  On: ONE vigo_traj_finish
         * call per device group — planners that share a device target, ts_ and controlPointsTs_ (the sample step is
         * ts_), whatever their control-point counts: rows are padded to the group's largest count; linearFactor_,
         * bspline_ and the path are installed from its downloads, the yaw from the downloaded velocity with libm's atan2
         * as evalTrajToMsg takes it.  A planner without a device, one of more than VIGO_MAX_CTRL_POINTS control points,
         * a row the call reports over capacity (the facade sizes at most 2048 samples per trajectory) or with an invalid
         * count, and every planner of a group whose call failed take the host route. */
        bool deviceEpilogue = false;
        /* makePlanBatch of at least this many planners runs as two to four pipelined parts of >= half this size (all but
         * the first on companion host threads with their own handles and HIP streams); 0 = never.  Same plans. */
        size_t pipelineThreshold = 2048;
        /* seedPathBatch.  Off: the searches and updatePath's head run on the host workers.  On: ONE vigo_seed_paths
         * launch per device group and one download; a trajectory the launch defers or refuses, a poly planner flying its
         * PWL fallback or without a polynomial, and a planner without a map snapshot take the host steps.  The kernels'
         * power is the correctly rounded one; libm's is that value or its neighbour (csrc/vigo_exact_pow.hpp; the rate
         * is counted by tools/pow_rounding_rate.py): the seeds agree to that. */
        bool deviceSeed = false;
        /* The fit stage of updatePathBatch and seedPathBatch.  Off: one vigo_bspline_fit launch per point count.  On:
         * every ready planner of up to 62 points takes ONE vigo_bspline_fit_mixed call per knot span, whatever the
         * counts (planners with more points keep the per-count launches); the installed control points are the same. */
        bool mixedFit = false;
        /* tries of seedPathBatch's inputPathCheck search per planner (instead of the reference's 50 ms): dt has shrunk to
         * 2.8 % of getInitTs() by the 16th; values below 1 count as 1 */
        int seedMaxTries = 16;
        /* tests: the inputs of every re-guide step the workers' twin runs are appended to *reguideStepLog (NULL: off);
         * the vector belongs to this call alone while it runs */
        std::vector<ReguideStepRecord>* reguideStepLog = nullptr;

        /* the options as a call takes them: the out-of-range values folded as the fields say */
        BatchOptions normalized() const {
            BatchOptions o = *this;
            if (o.deviceAstarBudget < 0) o.deviceAstarBudget = 0;
            if (o.deviceGuides != 1 && o.deviceGuides != 2) o.deviceGuides = 0;
            if (o.deviceReguide != 1 && o.deviceReguide != 2) o.deviceReguide = 0;
            if (o.seedMaxTries < 1) o.seedMaxTries = 1;
            return o;
        }
    };
    /* What the stages of one call did.  Per opt-in stage: the work items the device decided / those that took the host
     * route while the stage was selected (deferred, over a capacity, no device or snapshot; for deviceGuides and
     * deviceReguide also everything under setting 2). */
    struct BatchStats {
        long long astarDecided = 0, astarHost = 0;         /* prologue searches (deviceAstar) */
        long long guidesDecided = 0, guidesHost = 0;       /* prologue trajectories (deviceGuides) */
        long long prologueDecided = 0, prologueHost = 0;   /* prologue planners (devicePrologue); a planner that failed on the device counts as decided */
        long long reguideDecided = 0, reguideHost = 0;     /* re-guide steps (deviceReguide) */
        long long epilogueDecided = 0, epilogueHost = 0;   /* planners (deviceEpilogue) */
        long long seedDecided = 0, seedHost = 0;           /* seedPathBatch's planners, under either setting of deviceSeed */
        long long epilogueGroups = 0;                      /* vigo_traj_finish calls made (one per device group) */
        long long solveBatches = 0, solvePlanners = 0;     /* device batches the solves and device rounds opened, under either setting of mixedBatches, and the planners in them */
        double prologueSeconds = 0.0;                      /* wall time of makePlanBatch's prologue, summed over the parts of a pipelined call, which run side by side */
        double chainSeconds = 0.0;                         /* ... of devicePrologue's chains (upload to installed results) */
        long long prologueGroups = 0;                      /* device groups the prologue's stages opened (devicePrologue chains, deviceGuides = 1 and deviceAstar launches), under either setting of mixedPrologue */
        long long reguideGroups = 0;                       /* ... and the deviceReguide = 1 calls */
        long long validateDecided = 0, validateHost = 0;   /* isCurrTrajValidBatch's initialised planners: answered by vigo_traj_validate / by the per-planner route */
        long long validateGroups = 0;                      /* vigo_traj_validate calls made (one per device group, whatever the counts in it) */
        BatchStats& operator+=(const BatchStats& o) {
            astarDecided += o.astarDecided; astarHost += o.astarHost;
            guidesDecided += o.guidesDecided; guidesHost += o.guidesHost;
            prologueDecided += o.prologueDecided; prologueHost += o.prologueHost;
            reguideDecided += o.reguideDecided; reguideHost += o.reguideHost;
            epilogueDecided += o.epilogueDecided; epilogueHost += o.epilogueHost;
            seedDecided += o.seedDecided; seedHost += o.seedHost;
            epilogueGroups += o.epilogueGroups;
            solveBatches += o.solveBatches; solvePlanners += o.solvePlanners;
            prologueSeconds += o.prologueSeconds; chainSeconds += o.chainSeconds;
            prologueGroups += o.prologueGroups; reguideGroups += o.reguideGroups;
            validateDecided += o.validateDecided; validateHost += o.validateHost; validateGroups += o.validateGroups;
            return *this;
        }
    };

    /* Planners are grouped by control-point count, map object and every hot-path parameter (the yaml values, maxVel):
     * each group is one batch on the device.  Returns per-planner success like makePlan().  *stats, when given, receives
     * what this call's stages did. */
    static std::vector<bool> makePlanBatch(const std::vector<bsplineTraj*>& planners, const BatchOptions& options, BatchStats* stats = nullptr);
    /* not in the reference: the batched makePlan(nav_msgs::Path&, bool) — trajectories[i] receives what planner i's
     * evalTrajToMsg(yaw) gives after the plan; a planner that fails gets an empty path */
    static std::vector<bool> makePlanBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>& trajectories, bool yaw,
                                           const BatchOptions& options, BatchStats* stats = nullptr);
    /* added (workload tools, cabi_host.cpp: vigo_host_finish_timing): the epilogue stage alone on the planners' current
     * control points, as makePlanBatch runs it for planners that all succeeded; trajectories may be NULL */
    static void finishBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>* trajectories, bool yaw, const BatchOptions& options,
                            BatchStats* stats = nullptr);
    /* updatePath() for many planners at once: the least-squares fits run as device launches (mixedFit) */
    static std::vector<bool> updatePathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<nav_msgs::Path>& paths,
                                             const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions, const BatchOptions& options,
                                             BatchStats* stats = nullptr);
    /* not in the reference: the seed-path stage of bspline_node's replan step (src/bspline_node.cpp:317-378) and
     * updatePath for many planners at once — polys[i]'s plan sampled by getTrajectory(dt) from dt = getInitTs(), the
     * inputPathCheck search (dt *= 0.8 per failed try, at most seedMaxTries tries), then
     * updatePath(seed, startEndConditions[i]).  Returns updatePath's verdicts; seeds[i], when given, receives
     * adjustedInputPolyTraj (empty when no try passed), info[i] the search's outcome.  Same results as one planner after
     * another in the reference's order: every planner's search, then every planner's updatePath.  Stages: deviceSeed,
     * mixedFit. */
    struct SeedInfo {
        bool found = false;      /* a try passed inputPathCheck */
        int tries = 0;
        double dt = 0.0, finalTime = 0.0;
        bool wrote = false;      /* (internal) the search reached adjustPathLengthDirect; prevOut: what it left there */
        double prevOut = 0.0;
    };
    static std::vector<bool> seedPathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys,
                                           const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions, const BatchOptions& options,
                                           BatchStats* stats = nullptr, std::vector<nav_msgs::Path>* seeds = nullptr, std::vector<SeedInfo>* info = nullptr);

    /* not in the reference: isCurrTrajValid(firstCollisionPos) and hasDynamicCollisionTrajectory(controlPoints) for every
     * plan a service holds, after a map change.  Element i is what planners[i]->isCurrTrajValid(pos) returns — the index
     * rule of BT.h:329 with the planner's notCheckRatio_ and the gate step res / maxVel_ / 2 — and (*firstCollisionPos)[i]
     * is written only where that call would write it (the vector is resized to the planners, entries it holds are kept);
     * (*dynamicCollision)[i] is hasDynamicCollisionTrajectory on the planner's control points, false without obstacles.
     * Planners that share a device target, maxVel_ and notCheckRatio_ share ONE vigo_traj_validate (include/vigo_validate.h)
     * whatever their control-point counts, in rows of the group's largest count.  A planner that is not initialised is
     * invalid with no device work; planners without a device, of more than VIGO_MAX_CTRL_POINTS control points or whose
     * device call fails take the per-planner route, with the same answer (BatchStats::validateDecided / validateHost /
     * validateGroups). */
    static std::vector<bool> isCurrTrajValidBatch(const std::vector<bsplineTraj*>& planners, std::vector<Eigen::Vector3d>* firstCollisionPos = nullptr,
                                                  std::vector<bool>* dynamicCollision = nullptr, BatchStats* stats = nullptr);

    /* ---- the process default ----------------------------------------------------------------------------------------
     * The overloads without options take a snapshot of ONE process-wide BatchOptions, guarded by a lock, when they are
     * called; the setters below each write one field of it (see that field) and the getters read it.  A setter changes
     * the calls that start after it, on any thread, and none that is running.  Every batch call, with or without
     * options, adds its BatchStats to one process-wide total when it returns: the *Totals functions read that, and a
     * difference taken around a call is that call's stats as long as no other thread's call returns in between. */
    static BatchOptions defaultBatchOptions();
    static BatchStats batchTotals();
    static std::vector<bool> makePlanBatch(const std::vector<bsplineTraj*>& planners);
    static std::vector<bool> makePlanBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>& trajectories, bool yaw = true);
    static void finishBatch(const std::vector<bsplineTraj*>& planners, std::vector<nav_msgs::Path>* trajectories, bool yaw = true);
    static std::vector<bool> updatePathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<nav_msgs::Path>& paths,
                                             const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions);
    static std::vector<bool> seedPathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys,
                                           const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions,
                                           std::vector<nav_msgs::Path>* seeds = nullptr, std::vector<SeedInfo>* info = nullptr);
    static void setDeviceAstar(bool on);                       /* BatchOptions::deviceAstar */
    static bool deviceAstar();
    static void setDeviceAstarBudget(int maxExpansions);       /* BatchOptions::deviceAstarBudget */
    static void setDeviceGuides(int mode);                     /* BatchOptions::deviceGuides */
    static int deviceGuides();
    static void setDevicePrologue(bool on);                    /* BatchOptions::devicePrologue */
    static bool devicePrologue();
    static void setDeviceReguide(int mode);                    /* BatchOptions::deviceReguide */
    static int deviceReguide();
    static void setReguideStepLog(std::vector<ReguideStepRecord>* log);   /* BatchOptions::reguideStepLog: every later call without options appends */
    static void setDeviceResidentRebound(bool on);             /* BatchOptions::deviceResidentRebound */
    static bool deviceResidentRebound();
    static void setMixedBatches(bool on);                      /* BatchOptions::mixedBatches */
    static bool mixedBatches();
    static void setMixedPrologue(bool on);                     /* BatchOptions::mixedPrologue */
    static bool mixedPrologue();
    static void setDeviceEpilogue(bool on);                    /* BatchOptions::deviceEpilogue */
    static bool deviceEpilogue();
    static void setBatchPipelineThreshold(size_t planners);    /* BatchOptions::pipelineThreshold */
    static void setDeviceSeed(bool on);                        /* BatchOptions::deviceSeed */
    static bool deviceSeed();
    static void setMixedFit(bool on);                          /* BatchOptions::mixedFit */
    static bool mixedFit();
    static void setSeedMaxTries(int n);                        /* BatchOptions::seedMaxTries */
    static int seedMaxTries();
    /* Process-wide running totals (BatchStats' fields of the same names; take the difference around a call) */
    static void deviceAstarTotals(long long* deviceDecided, long long* hostRun, double* prologueSeconds);
    static void deviceGuideTotals(long long* deviceDecided, long long* hostRun);
    static void devicePrologueTotals(long long* deviceDecided, long long* hostRun, double* chainSeconds);
    static void deviceReguideTotals(long long* deviceDecided, long long* hostRun);
    static void deviceEpilogueTotals(long long* deviceDecided, long long* hostRun, long long* deviceGroups);
    static void mixedBatchTotals(long long* deviceBatches, long long* planners);
    static void deviceSeedTotals(long long* deviceDecided, long long* hostRun);

    const std::vector<std::vector<Eigen::Vector3d>>& getAstarPaths() const { return astarPaths_; }   /* added (tests) */
    const std::vector<std::pair<int, int>>& getCollisionSeg() const { return collisionSeg_; }         /* added (tests) */
    /* added (tests, cabi_host.cpp: vigo_host_seed_steps): one planner's host steps of the seed stage with the previous path
     * lengths passed in and out — the search from dt0, then updatePath's head on its seed */
    struct SeedSteps {
        SeedInfo search;
        nav_msgs::Path seed;
        bool fitOk = false, fitWrote = false;
        double prevFitOut = 0.0;
        std::vector<Eigen::Vector3d> fitPoints;
    };
    void seedSteps(polyTrajOccMap& poly, double dt0, int maxTries, double prevSeedIn, double prevFitIn, SeedSteps& out);
    double getMaxPathLength() const { return maxPathLength_; }
    void clear();
    void findCollisionSeg(const Eigen::MatrixXd& controlPoints, std::vector<std::pair<int, int>>& collisionSeg);
    bool pathSearch(std::vector<std::pair<int, int>>& collisionSeg, std::vector<std::vector<Eigen::Vector3d>>& paths);
    void assignGuidePointsSemiCircle(const std::vector<std::vector<Eigen::Vector3d>>& paths,
                                     const std::vector<std::pair<int, int>>& collisionSeg);
    bool isReguideRequired(std::vector<std::pair<int, int>>& reguideCollisionSeg);
    bool optimizeTrajectory();
    int optimize();
    void adjustPathLengthDirect(const std::vector<Eigen::Vector3d>& path, std::vector<Eigen::Vector3d>& adjustedPath);

    /* the lbfgs_evaluate_t seam (BT.h:118-119) on the device: cost and gradient of x */
    double costFunction(const double* x, double* grad, const int n);
    static double solverCostFunction(void* func_data, const double* x, double* grad, const int n);   // BT.h:118
    /* the four terms on their own (BT.h:120-123); gradient is 3 x N with the fixed end columns left zero */
    void getDistanceCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient);
    void getSmoothnessCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient);
    void getFeasibilityCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient);
    void getDynamicObstacleCost(const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient);
    void writeCurrentTrajInfo(const std::string& filePath, double dt);                               // BT.cpp:1464-1496

    void linearFeasibilityReparam();
    double getLinearReparamTime(double t);
    double getLinearFactor();

    double getInitTs();
    double getControlPointTs();
    double getControlPointDist();
    trajPlanner::bspline getTrajectory();
    geometry_msgs::PoseStamped getPose(double t, bool yaw = true);
    double getDuration();
    double getTimestep();
    Eigen::MatrixXd getControlPoints();
    const optData& getOptData() const { return optData_; }   /* added (tests): guide points / directions as the optimizer gets them */
    /* added (workload tools, cabi_host.cpp): take these control points as the planner's current ones with empty guide
     * lists — the state updatePath() leaves (BT.cpp:315-322) — so the host steps of the rebound loop can be replayed on them */
    void setControlPoints(const Eigen::MatrixXd& controlPoints) { installControlPoints(controlPoints, {}); }
    /* added (tests, cabi_host.cpp: vigo_host_reguide_facade): the state the rebound loop carries between two rounds —
     * collisionSeg_, the guide pairs per control point (after setControlPoints), the two weights the loop doubles — and
     * ONE pass of the loop body (reboundStep) on it with the given gate results; failCount in/out */
    void setLoopState(const std::vector<std::pair<int, int>>& collisionSeg, const std::vector<std::vector<Eigen::Vector3d>>& guidePoints,
                      const std::vector<std::vector<Eigen::Vector3d>>& guideDirections, double weightDistance, double weightDynamicObstacle);
    void runLoopBody(bool hasCollision, bool hasDynamicCollision, int& failCount, bool& needOptimize, bool& done);
    void getLoopWeights(double& weightDistance, double& weightDynamicObstacle) const { weightDistance = weightDistance_; weightDynamicObstacle = weightDynamicObstacle_; }
    bool isCurrTrajValid();
    bool isCurrTrajValid(Eigen::Vector3d& firstCollisionPos);
    int getLastSolverStatus() const { return lastStatus_; }
    bool hasDynamicObstacles() const { return !optData_.dynamicObstaclesPos.empty(); }

    std::vector<Eigen::Vector3d> evalTraj();
    std::vector<Eigen::Vector3d> evalTraj(double dt);
    nav_msgs::Path evalTrajToMsg(bool yaw = true);
    nav_msgs::Path evalTrajToMsg(double dt, bool yaw = true);
    void pathMsgToEigenPoints(const nav_msgs::Path& path, std::vector<Eigen::Vector3d>& points);
    void eigenPointsToPathMsg(const std::vector<Eigen::Vector3d>& points, nav_msgs::Path& path);

    bool checkCollisionLine(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2);
    void shortcutPath(const std::vector<Eigen::Vector3d>& path, std::vector<Eigen::Vector3d>& pathSC);
    bool findGuidePointSemiCircle(int controlPointIdx, const std::pair<int, int>& seg, const std::vector<Eigen::Vector3d>& path,
                                  Eigen::Vector3d& guidePoint);
    bool hasCollisionTrajectory(const Eigen::MatrixXd& controlPoints);
    bool hasDynamicCollisionTrajectory(const Eigen::MatrixXd& controlPoints);
    /* public helpers of the reference's class, BT.h:165-172 (its triangle / distance-field / polygon helpers, :173-177,
       are only called from commented-out code and are not carried) */
    void shortcutPaths(const std::vector<std::vector<Eigen::Vector3d>>& paths, std::vector<std::vector<Eigen::Vector3d>>& pathsSC);
    bool indexInCollisionSeg(const std::vector<std::pair<int, int>>& collisionSeg, int idx);
    void compareCollisionSeg(const std::vector<std::pair<int, int>>& prevCollisionSeg, const std::vector<std::pair<int, int>>& newCollisionSeg,
                             std::vector<int>& newCollisionPoints, std::vector<int>& overlappedCollisionPoints);
    int findCollisionSegIndex(const std::vector<std::pair<int, int>>& collisionSeg, int idx);
    bool isControlPointRequireNewGuide(int controlPointIdx);

private:
    void reboundBegin(Rebound& r);
    /* one pass of the loop body of BT.cpp:619-681 given the gate results; sets r.done/ok/needOptimize */
    void reboundStep(Rebound& r, bool hasCollision, bool hasDynamicCollision, bool timedOut);
    bool prepareFitPoints(const nav_msgs::Path& adjustedPath, std::vector<Eigen::Vector3d>& adjustedCurveFitPoints);
    /* the same with the previous path length (adjustPathLengthDirect's function-static, BT.cpp:755) passed in and out:
       *wrote says whether the call reached that function at all */
    bool prepareFitPointsWith(const nav_msgs::Path& adjustedPath, std::vector<Eigen::Vector3d>& adjustedCurveFitPoints, double prevIn,
                              double& prevOut, bool& wrote);
    void adjustPathLengthWith(const std::vector<Eigen::Vector3d>& path, std::vector<Eigen::Vector3d>& adjustedPath, double prevIn, double& prevOut);
    bool inputPathCheckWith(const nav_msgs::Path& path, nav_msgs::Path& adjustedPath, double dt, double& finalTime, double prevIn,
                            double& prevOut, bool& wrote);
    /* the inputPathCheck search of one planner: getTrajectory(dt) from dt0, dt *= 0.8 per failed try */
    void seedSearchWith(polyTrajOccMap& poly, double dt0, int maxTries, double prevIn, SeedInfo& s, nav_msgs::Path& seed);
    /* the launch of seedPathBatch under deviceSeed: fills the entries of the planners it decided (onDevice) */
    struct SeedBatch;
    static void seedOnDevice(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys, SeedBatch& sb);
    /* the fit stage of updatePathBatch / seedPathBatch: one vigo_bspline_fit launch per group of equal point count and
     * device target among the ready planners (mixedFit: see there), control points installed; ok[i] set for the fitted ones */
    static void fitGroups(const std::vector<bsplineTraj*>& planners, const std::vector<std::vector<Eigen::Vector3d>>& fitPts,
                          const std::vector<bool>& ready, const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions,
                          std::vector<bool>& ok, bool mixedFit);
    void installControlPoints(const Eigen::MatrixXd& controlPoints, const std::vector<Eigen::Vector3d>& adjustedCurveFitPoints);
    bool termCost(int term, const Eigen::MatrixXd& controlPoints, double& cost, Eigen::MatrixXd& gradient);
    void reboundFinish(Rebound& r, bool ok);
    bool sameBatchKey(const bsplineTraj& o) const;                  // may share a device batch with o
    bool sameBatchKeyAnyCount(const bsplineTraj& o) const;          // ... but for the control-point count
    bool sameSolveGroup(const bsplineTraj& o, bool mixed) const;    // ... a batch of solveBatch / deviceRounds (mixedBatches)
    struct SearchGroup;                                             // ... and what its device A* searches share on top
    void fillParams(vigo_params_s* P) const;
    static void solveBatch(const std::vector<bsplineTraj*>& ps, const BatchOptions& o, BatchStats& stats);   // one vigo_optimize for all
    /* up to maxRounds rounds of the loop on the device for one group; fills rb[i]->devStatus / gate flags and the
     * planners' control points, weights, failCount, collisionSeg_.  false: device failure (nothing usable) */
    static bool deviceRounds(const std::vector<bsplineTraj*>& grp, const std::vector<Rebound*>& rb, int maxRounds, const BatchOptions& o,
                             BatchStats& stats);
    static void gateBatch(const std::vector<bsplineTraj*>& ps, std::vector<uint8_t>& col, std::vector<uint8_t>& dyn);
    /* the steps of makePlanBatch: the split into pipelined parts; for one part the prologue (steps 1-3), the rebound loop
     * on the device or driven from the host, the move of finished planners out of the loop, the epilogue (steps 5-6) */
    struct PlanBatch;
    /* paths: NULL, or one per planner (the calls with trajectories); o: normalized; stats: the call's, added to */
    static std::vector<bool> planBatch(const std::vector<bsplineTraj*>& planners, nav_msgs::Path* paths, bool yaw, const BatchOptions& o, BatchStats& stats);
    static std::vector<bool> makePlanPipelined(const std::vector<bsplineTraj*>& planners, nav_msgs::Path* paths, bool yaw, const BatchOptions& o,
                                               BatchStats& stats);
    static std::vector<bool> planPart(const std::vector<bsplineTraj*>& planners, nav_msgs::Path* paths, bool yaw, const BatchOptions& o, BatchStats& stats);
    static void planPrologue(const std::vector<bsplineTraj*>& planners, PlanBatch& pb);
    /* step 2 of the prologue for all planners with device searches; found[i]: planner i's pathSearch outcome */
    struct AstarJob;
    static void pathSearchBatch(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, const std::vector<uint8_t>& ready, std::vector<uint8_t>& found);
    static void runAstarJobs(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, std::vector<AstarJob>& jobs);
    /* step 3 of the prologue under deviceGuides = 1 | 2 for the planners with found[i] */
    static void assignGuidesBatch(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, const std::vector<uint8_t>& found);
    void assignGuidesCore();
    void assignGuidesCoreOn(const std::vector<std::pair<int, int>>& collisionSeg, const std::vector<std::vector<Eigen::Vector3d>>& paths);
    /* deviceReguide = 1: the eligible planners of `active` through vigo_rebound_reguide; the ones it decided get
     * devStatus VIGO_RB_ACTIVE.  (2, and what 1 left: reguideStepCore on the workers, which logs to pb's reguideStepLog) */
    static void reguideOnDevice(PlanBatch& pb, const std::vector<uint8_t>& devOk);
    static bool reguideEligible(const Rebound& r);
    void reguideStepCore(Rebound& r, PlanBatch& pb);
    /* steps 1-3 under devicePrologue; outcome[i]: 1 prepared, 2 failed (A*), 0 not a planner of the batch */
    static void prologueOnDevice(const std::vector<bsplineTraj*>& planners, PlanBatch& pb, std::vector<uint8_t>& outcome);
    void packGuideInput(std::vector<int32_t>& seg, std::vector<int32_t>& pathOff, std::vector<double>& path) const;
    static void reboundOnDevice(PlanBatch& pb, bool timing);
    static void reboundFromHost(PlanBatch& pb, bool timing);
    static void retireFinished(PlanBatch& pb);
    static void planEpilogue(const std::vector<bsplineTraj*>& planners, const std::vector<bool>& result, nav_msgs::Path* paths, bool yaw,
                             const BatchOptions& o, BatchStats& stats);
    /* deviceEpilogue: the planners with todo[i] through vigo_traj_finish; todo[i] is cleared for those it finished */
    static void finishOnDevice(const std::vector<bsplineTraj*>& planners, std::vector<uint8_t>& todo, nav_msgs::Path* paths, bool yaw, BatchStats& stats);
    static void validateOnDevice(const std::vector<bsplineTraj*>& planners, std::vector<uint8_t>& todo, std::vector<bool>& valid,
                                 std::vector<Eigen::Vector3d>* firstCollisionPos, std::vector<bool>* dynamicCollision, BatchStats& stats);
};
}  // namespace trajPlanner
#endif
