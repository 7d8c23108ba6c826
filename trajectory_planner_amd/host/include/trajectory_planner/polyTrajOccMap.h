/*
 * polyTrajOccMap.h — trajPlanner::polyTrajOccMap with the reference's public interface
 * (include/trajectory_planner/polyTrajOccMap.h:49-98, PM below), the min-snap seed planner of bspline_node.
 *
 * makePlan(): waypoint path -> min-snap QP (polyTrajSolver, host) -> trajectory sampled at sample_delta_time -> every
 * sample looked up in the map (isInflatedOccupied AND isUnknown, PM.cpp:524-546) -> shrink the colliding segments'
 * corridors -> repeat (PM.cpp:326-399); piecewise-linear fallback with use_pwl_failsafe.  The solo makePlan runs
 * entirely on the host (no GPU, no map snapshot) and is the twin makePlanBatch is pinned against: there the QPs go to
 * vigo_minsnap and the checks to ONE vigo_traj_point_check launch per round.
 * Differences to the reference: no ROS publisher or timer (registerPub / registerCallback / visCB / publishTrajVis do
 * nothing); calls that would dereference a solver that does not exist yet (getDuration, getPos before any makePlan)
 * answer zero or empty instead of crashing.
 */
#ifndef POLYTRAJOCCMAP_H
#define POLYTRAJOCCMAP_H
#include <trajectory_planner/compat.h>
#include <trajectory_planner/mapAdapter.h>
#include <trajectory_planner/piecewiseLinearTraj.h>
#include <trajectory_planner/polyTrajSolver.h>
#include <trajectory_planner/utils.h>

#include <memory>
#include <set>
#include <vector>

namespace vigo_host {
template <class Planner> struct LockStepBatch;   // the lock-step loop of makePlanBatch (src/polyBatchLoop.h)
struct QpMember;
struct TrajCheck;
}  // namespace vigo_host

namespace trajPlanner {
class polyTrajOccMap {
private:
    ros::NodeHandle nh_;
    std::shared_ptr<trajPlanner::polyTrajSolver> trajSolver_;
    std::shared_ptr<trajPlanner::pwlTraj> pwlTrajSolver_;
    std::vector<pose> path_;
    nav_msgs::Path trajVisMsg_;
    geometry_msgs::Twist initVel_, endVel_, initAcc_, endAcc_;

    // parameters (PM.cpp:20-138)
    int polyDegree_;
    int diffDegree_;
    int continuityDegree_;
    double desiredVel_;
    double desiredAcc_;
    double initR_;
    double timeout_;
    double corridorRes_;
    double fs_;
    bool softConstraint_;
    double softConstraintRadius_ = 0.5;
    double delT_;
    int maxIter_;
    bool usePWL_;

    // status
    bool findValidTraj_ = false;
    int lastIterations_ = 0;

    // the device back-end of makePlanBatch: the map, its snapshot on the handle, the handle (mapAdapter.h)
    DeviceLink link_;
    bool syncDevice();
    /* the planning loop of PM.cpp:326-399 in steps, driven by makePlan and makePlanBatch (polyTrajOccMap.cpp) */
    struct PlanState {
        bool corridors = true;          // makePlan's corridorConstraint
        std::vector<double> corridor;   // corridorSizeVec
        int iters = 0;                  // countIter
        double t0 = 0;
    };
    PlanState begin(bool corridorConstraint);
    void solveOnHost(PlanState& s);
    bool advance(PlanState& s, bool collides, const std::set<int>& collisionSeg);
    void finish(std::vector<pose>& trajectory, bool valid);
    /* this planner's rules in the lock-step loop of makePlanBatch (src/polyBatchLoop.h; each is stated at its definition) */
    friend struct vigo_host::LockStepBatch<polyTrajOccMap>;
    struct DeviceSteps;
    static const polyTrajOccMap* batchReference(const std::vector<polyTrajOccMap*>& ps);
    bool batchable(const polyTrajOccMap* ref) const;
    bool planAlone(std::vector<pose>& trajectory, bool corridorConstraint, bool& told);
    static void planWithoutDevice(const std::vector<polyTrajOccMap*>& ps, const std::vector<size_t>& grp, bool corridorConstraint,
                                  std::vector<std::vector<pose>>& out, std::vector<bool>& result);
    PlanState beginBatch(bool corridorConstraint) { return begin(corridorConstraint); }
    bool timedOutBeforeRound(const PlanState& s, size_t G) const;
    bool timedOutAfterRound(const PlanState&, size_t) const { return false; }
    bool hostQpOnly() const { return softConstraint_; }
    bool sameQpGroup(const PlanState& mine, const polyTrajOccMap& o, const PlanState& theirs) const;
    vigo_host::QpMember qpMember(size_t who, const PlanState& s) const;
    void takeQpResult(PlanState& s, const vigo_host::QpMember& m);
    bool validWithoutCheck(PlanState& s);
    void checkOnHost(polyTrajOccMap& lead, vigo_host::TrajCheck& c);
    bool finishBatch(std::vector<pose>& trajectory, bool valid);
    static const char* batchTag() { return "[minSnapTraj]: "; }

public:
    polyTrajOccMap(const ros::NodeHandle& nh);
    ~polyTrajOccMap();
    polyTrajOccMap(const polyTrajOccMap&) = delete;
    polyTrajOccMap& operator=(const polyTrajOccMap&) = delete;
    void initParam();
    void registerPub() {}
    void registerCallback() {}
    void setMap(const std::shared_ptr<mapManager::occMap>& map);
    void initSolver();
    void initPWLSolver();

    // update desired vel
    void updateDesiredVel(double desiredVel);
    void updateDesiredAcc(double desiredAcc);

    // update waypoint path
    void updatePath(const nav_msgs::Path& path);
    void updatePath(const nav_msgs::Path& path, const std::vector<Eigen::Vector3d>& startEndCondition);
    void updatePath(const std::vector<pose>& path);

    // initial condition
    void updateInitVel(double vx, double vy, double vz);
    void updateInitVel(const geometry_msgs::Twist& v);
    void updateEndVel(double vx, double vy, double vz);
    void updateEndVel(const geometry_msgs::Twist& v);
    void updateInitAcc(double ax, double ay, double az);
    void updateInitAcc(const geometry_msgs::Twist& a);
    void updateEndAcc(double ax, double ay, double az);
    void updateEndAcc(const geometry_msgs::Twist& a);
    void setDefaultInit();

    bool makePlan(bool corridorConstraint);
    bool makePlan(std::vector<pose>& trajectory);
    bool makePlan(std::vector<pose>& trajectory, bool corridorConstraint);
    bool makePlan(nav_msgs::Path& trajectory);
    bool makePlan(nav_msgs::Path& trajectory, bool corridorConstraint);

    /* not in the reference: makePlan(trajectory, corridorConstraint) of many planners in lock-step.  Per round ONE
     * vigo_minsnap launch per (waypoint count, degrees) group solves the active planners' QPs and ONE
     * vigo_traj_point_check launch checks every candidate whole; soft constraints, shapes vigo_minsnap_supported refuses
     * and device results other than "solved" take the host QP.  The bookkeeping (corridors, iteration limit, time limit,
     * PWL fallback) stays per planner, and each planner is left as its own makePlan leaves it.  trajectories[i], when
     * given, receives planner i's samples.  Returns the verdicts. */
    static std::vector<bool> makePlanBatch(const std::vector<polyTrajOccMap*>& planners, bool corridorConstraint,
                                           std::vector<std::vector<pose>>* trajectories = nullptr);

    /* not in the reference: the box of the map the device snapshot covers (mapAdapter.h), the request to re-snapshot a
     * map that changed, the HIP device of the back-end handle (default 0) — makePlanBatch only */
    void setMapRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);
    void refreshMap();
    void refreshMap(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);   // ... inside this metric box only
    void setDevice(int ordinal);

    // visualization (no ROS here: nothing is published)
    template <class Event>
    void visCB(const Event&) {}
    void publishTrajVis() {}

    nav_msgs::Path getTrajectory(double dt);
    geometry_msgs::PoseStamped getPose(double t);
    Eigen::Vector3d getPos(double t);
    Eigen::Vector3d getVel(double t);
    Eigen::Vector3d getAcc(double t);
    double getDuration();
    bool checkCollisionTraj(const std::vector<pose>& trajectory, double delT, std::set<int>& collisionSeg);
    void adjustCorridorSize(const std::set<int>& collisionSeg, std::vector<double>& corridorSizeVec);
    void trajMsgConverter(const std::vector<pose>& trajectoryTemp, nav_msgs::Path& trajectory);

    /* not in the reference (bsplineTraj::seedPathBatch): the polynomial getTrajectory / getPos sample — NULL before the
     * first plan — and whether they fly the PWL fallback's duration instead of its own (use_pwl_failsafe and no valid plan) */
    const polyTrajSolver* getSolver() const { return trajSolver_.get(); }
    bool usesPwlFallback() const { return usePWL_ && !findValidTraj_; }
    /* not in the reference: the verdict and the QP solves of the last makePlan */
    bool isValid() const { return findValidTraj_; }
    int getIterations() const { return lastIterations_; }
};
}  // namespace trajPlanner
#endif
