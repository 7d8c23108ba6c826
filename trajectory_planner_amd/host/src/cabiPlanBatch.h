// cabiPlanBatch.h — the tests' and tools' one driver of bsplineTraj::makePlanBatch (vigo_host_plan_batch) and the pieces
// the other entry points of cabi_host.cpp share with it: what a batch plans on, fresh planners per run, one timed call,
// the planners' results as one slot of the outputs.  tests/plan_batch.py mirrors the job struct.
#pragma once
#ifdef __cplusplus
#include <trajectory_planner/bsplineTraj.h>

#include <memory>
#include <vector>

extern "C" {
#endif

// One job of vigo_host_plan_batch: n planners on n_maps dense maps plan under the options of a SLOT, one
// updatePathBatch + makePlanBatch on fresh planners per RUN, in the order of run_slot.
typedef struct vigo_host_plan_batch_job {
    int size;                          // sizeof(vigo_host_plan_batch_job_t): anything else is refused
    // the world: n_maps map objects (separate device groups) of dims voxel bytes, planner t on map t % n_maps; copies
    // of vox, the odd ones of vox2 when that is given (same extents, other contents)
    int n_maps;
    const unsigned char* vox;
    const unsigned char* vox2;
    const int* dims;                   // [3]
    const double* origin;              // [3]
    double res;
    const double* cfg;                 // [6] as in vigo_host_bspline_prologue
    // the planners: path t = poses path_off[t] .. path_off[t + 1] - 1 of path_xyz, at least 2
    int n;
    int with_paths, yaw;               // with_paths != 0: the overload makePlanBatch(planners, trajectories, yaw != 0)
    const int* path_off;               // [n + 1]
    const double* path_xyz;
    const int* planner_device;         // [n] or NULL; >= 0: setDevice(it) before setMap, < 0: as cfg
    const double* planner_timestep;    // [n] or NULL; bspline_traj/timestep of planner t, NaN: as cfg
    // the slots: mask in vigo_host_switches' bit layout, budget = deviceAstarBudget, route
    //   0  the options are passed to the call; the process default is not touched
    //   1  the options are set as the process default through the setters, the overload without options is called, and
    //      the setters put the default back
    //   2  (mask must be 0) the overload without options and no setter called: the untouched default
    // routes 1 and 2 have no BatchStats of the call: there, what bsplineTraj::batchTotals() moved by around the run
    int n_slots;
    const int* slot_mask;
    const int* slot_budget;
    const int* slot_route;
    // the schedule: the slot of each run, in order
    int n_runs;
    const int* run_slot;
    // != 0: exactly two runs, of two different slots on route 0, at the same time on two threads, each with map objects,
    // planners and handles of its own; each thread makes its planners, waits for the other to have done so, and plans
    int concurrent;
    // >= 0: the last run of this slot (route 0) logs its re-guide steps; twin[2] receives their number and how many of
    // them the kernels' host twin (vigo_host_rebound_reguide_core, mode 1) under the capacities caps = (cap_log2,
    // max_nodes, heap_cap, guide_path_cap) does not answer with VIGO_REGUIDE_DEFERRED: the share the device can decide
    int replay_slot;
    int caps[4];
    int ncp_cap, pose_cap;
    long long cap;
    // outputs per slot [n_slots] x ..., of the slot's LAST run, each skipped when NULL: ok[n] makePlanBatch's flags,
    // solver[n] the last L-BFGS status, ncp[n], ctrl[n][ncp_cap][3], factor[n] (linearFactor_); concatenated in planner
    // order n_seg[n] + segs[cap][2] (collisionSeg_), n_path_pts[n] + paths[cap][3] (astarPaths_' points), n_guides[n] +
    // guides[cap][6] (point, direction); n_poses[n] + pos[n][pose_cap][3] + quat[n][pose_cap][4] (x, y, z, w).  Padding
    // is the caller's.  stats[n_slots][K]: every count field of BatchStats in the order of its declaration
    int *ok, *solver, *ncp;
    double *ctrl, *factor;
    int *n_seg, *segs, *n_path_pts;
    double* paths;
    int* n_guides;
    double* guides;
    int* n_poses;
    double *pos, *quat;
    long long* stats;
    long long* totals;                 // [K]: what the process totals' counts moved by across the whole call
    long long* twin;                   // [2]
    double* seconds;                   // [n_runs][3]: prologueSeconds, chainSeconds, the call's wall time
} vigo_host_plan_batch_job_t;

// Returns 0, -1 on a bad argument (checked before a map or a planner is made), -2 when a buffer is too small, -3 when a
// call threw.  Needs a GPU.
int vigo_host_plan_batch(const vigo_host_plan_batch_job_t* job);
int vigo_host_plan_batch_job_size(void);
// the facade's opt-in switches of the process default (bsplineTraj::defaultBatchOptions) as they stand: bit 0
// deviceAstar, bits 1-2 deviceGuides, bit 3 devicePrologue, bits 4-5 deviceReguide, bit 6 mixedBatches, bit 7
// deviceEpilogue, bit 8 mixedPrologue (0: everything off, the default)
int vigo_host_switches(void);

#ifdef __cplusplus
}  // extern "C"

namespace cabi {
using trajPlanner::bsplineTraj;

// a dense map of nx * ny * nz voxel bytes (vigo.h voxel contract)
std::shared_ptr<mapManager::occMap> denseMap(int nx, int ny, int nz, const double* origin, double res, const unsigned char* voxels);
// cfg[6] of the entry points: distance_threshold, min_height, max_height, max_obstacle_size[3]
void setBsplineParams(ros::NodeHandle& nh, const double* cfg);
// the A* node pool of a planner with these parameters on a map of resolution res (bsplineTraj::setMap, BT.cpp:187-195)
void nodePool(const double* cfg, double res, int pool[3]);
// n_pts poses at the xyz triples q
nav_msgs::Path pathFromXyz(const double* q, int n_pts);

// built once per call: n_maps dense maps; the planners' parameters; the n input paths (path t = poses path_off[t] ..
// path_off[t + 1] - 1 of path_xyz); zero start / end conditions; device[t] / stepNh[t] where the job overrides them
struct BatchFixture {
    std::vector<std::shared_ptr<mapManager::occMap>> maps;
    ros::NodeHandle nh;
    std::vector<nav_msgs::Path> in;
    std::vector<std::vector<Eigen::Vector3d>> cond;
    std::vector<int> device;               // empty: none
    std::vector<ros::NodeHandle> stepNh;   // empty: nh for everyone
    BatchFixture(const unsigned char* vox, const int* dims, const double* origin, double res, const double* cfg, int n, const int* path_off,
                 const double* path_xyz, const unsigned char* vox2 = nullptr, int n_maps = 1, const int* planner_device = nullptr,
                 const double* planner_timestep = nullptr);
};

// new planners for one run, planner t on map t % n_maps, through updatePathBatch
struct FreshPlanners {
    std::vector<std::unique_ptr<bsplineTraj>> owners;
    std::vector<bsplineTraj*> ps;
};
FreshPlanners freshPlanners(const BatchFixture& fx);

// makePlanBatch's flags, its wall time in ms: the overload without options (the process default) ...
std::vector<bool> timedPlan(const std::vector<bsplineTraj*>& ps, double& ms, std::vector<nav_msgs::Path>* traj = nullptr, bool yaw = true);
// ... and a call under its own options, what its stages did in st; traj: the overload with trajectories
std::vector<bool> timedPlan(const std::vector<bsplineTraj*>& ps, const bsplineTraj::BatchOptions& o, double& ms, bsplineTraj::BatchStats& st,
                            std::vector<nav_msgs::Path>* traj = nullptr, bool yaw = true);

// The n planners' results as slot `slot` of out's per-slot outputs up to guides (out.ncp_cap, out.cap their room).
// Returns 0, -2 when ncp_cap or cap is too small.
int dumpSlot(const std::vector<bsplineTraj*>& ps, const std::vector<bool>& planned, int slot, const vigo_host_plan_batch_job_t& out);
// ... and the n trajectories of the overload with trajectories (an empty traj: no poses).  Returns 0, -2 when pose_cap
// is too small.
int dumpPoses(const std::vector<nav_msgs::Path>& traj, size_t n, int slot, int pose_cap, int* n_poses, double* pos, double* quat);

constexpr int kStatCounts = 20;
void statCounts(const bsplineTraj::BatchStats& s, long long* out);
bsplineTraj::BatchOptions optionsOfMask(int mask, int budget);
// the fields optionsOfMask writes, as the process default, through their setters
void setDefaults(const bsplineTraj::BatchOptions& o);
}  // namespace cabi
#endif
