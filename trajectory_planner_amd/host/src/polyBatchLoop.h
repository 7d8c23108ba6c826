// polyBatchLoop.h — internal to the host facades: makePlanBatch of both min-snap planners (polyTrajOctomap, polyTrajOccMap)
// as ONE lock-step loop over the planner class, LockStepBatch<Planner>::run.  The loop text — who plans alone, the active
// set, the QP groups and their member lists, install or host fallback, the candidate list, the exit on a failed device
// step — exists here once; each class supplies, as private members of the same names, the rules in which the two planners
// differ (listed at run()).  The two device steps of a round are the `steps` argument: in the library each class passes
// its DeviceSteps, whose members call minsnapGroupOnDevice / checkTrajectoriesOnDevice (polyBatch.h) with the class's
// entry point; tests/poly_batch_check.cpp passes scripted ones.  Nothing of HIP is included here.
#ifndef VIGO_HOST_POLY_BATCH_LOOP_H
#define VIGO_HOST_POLY_BATCH_LOOP_H
#include <trajectory_planner/polyTrajSolver.h>

#include <chrono>
#include <cstdint>
#include <iostream>
#include <set>
#include <vector>

#include "../../../include/vigo.h"

namespace vigo_host {

inline double nowSec() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

inline void appendXyz(const std::vector<trajPlanner::pose>& pts, std::vector<double>& xyz) {
    for (const trajPlanner::pose& q : pts) { xyz.push_back(q.x); xyz.push_back(q.y); xyz.push_back(q.z); }
}

// both planners' trajMsgConverter (PO.cpp:597-617, PM.cpp:554-571)
inline void posesToPathMsg(const std::vector<trajPlanner::pose>& poses, nav_msgs::Path& msg) {
    msg.poses.clear();
    for (const trajPlanner::pose& p : poses) {
        geometry_msgs::PoseStamped ps;
        ps.header.frame_id = "map";
        ps.pose.position.x = p.x; ps.pose.position.y = p.y; ps.pose.position.z = p.z;
        ps.pose.orientation = trajPlanner::quaternion_from_rpy(0, 0, p.yaw);
        msg.poses.push_back(ps);
    }
    msg.header.frame_id = "map";
}

// checkCollisionTraj(trajectory, delT, collisionSeg) of both planners (PO.cpp:634-656, PM.cpp:524-546) on per-sample flags:
// t accumulates delT per sample; a colliding sample blames the first time-knot interval containing t (inclusive)
inline bool collisionSegments(const uint8_t* flags, size_t n, const std::vector<double>& knots, double delT, std::set<int>& collisionSeg) {
    double t = 0;
    bool has = false;
    for (size_t k = 0; k < n; ++k) {
        if (flags[k]) {
            has = true;
            for (size_t i = 0; i + 1 < knots.size(); ++i)
                if (t >= knots[i] && t <= knots[i + 1]) { collisionSeg.insert((int)i); break; }
        }
        t += delT;
    }
    return has;
}

// ---- one member of a QP group (T paths of the same waypoint count W, degree 7, solved in one call of the QP step) ----
struct QpMember {
    size_t who;                             // the caller's own index of this member (not read by the step)
    const std::vector<trajPlanner::pose>* path;
    const std::vector<double>* corridor;    // in: radius per segment; nullptr (for the whole group): no corridor boxes
    const geometry_msgs::Twist* conds[4];   // in: start / end vel, start / end acc; nullptr (whole group): none passed, not zeros
    int32_t status;                         // out: 0 solved, -1 numerical failure, -2 infeasible corridor
    std::vector<double> sol[3];             // out: the solution per axis, as polyTrajSolver::installSolution takes it
};

// ---- one candidate of a round's whole-trajectory check (every candidate in one call of the check step) ----
struct TrajCheck {
    size_t who;                            // the caller's own index of this candidate (not read here)
    trajPlanner::polyTrajSolver* solver;   // in: the installed polynomial (device QP, host QP or a kept one) and its own knots
    double delT;
    trajPlanner::pose end;                 // in: the appended last waypoint
    int32_t status;                        // out: VIGO_TRAJ_OK, or the entry rejects it: the caller checks it on the host
    bool collides;
    std::set<int> segments;                // out: collisionSeg
};

// Steps: bool ready(Planner* lead)            the device of the batch can be reached (the lead's syncDevice)
//        bool supported(W, diff, cont)         the device QP takes this shape (vigo_minsnap_supported at degree 7)
//        bool solve(diff, cont, vel, corridorRes, std::vector<QpMember>&)   one group's QPs; false: the call failed
//        bool check(std::vector<TrajCheck>&)   every candidate of the round; false: the call failed
//        const char* lastError()
// Planner (private members; the rule each one is, per class, stands at its definition):
//        batchReference, batchable, planAlone, planWithoutDevice      who the batch takes, who leads, no device
//        beginBatch, timedOutBeforeRound, timedOutAfterRound          the start of a plan, where the time limit is tested
//        hostQpOnly, sameQpGroup, qpMember, takeQpResult, solveOnHost the QP: straight to the host, group key, conditions, status
//        validWithoutCheck, checkOnHost, advance                      a round without check, a rejected candidate, the verdict
//        finishBatch, batchTag                                        the ending, the prefix of the console line
template <class Planner>
struct LockStepBatch {
    typedef trajPlanner::pose pose;

    template <class Steps>
    static std::vector<bool> run(const std::vector<Planner*>& ps, bool corridorConstraint, std::vector<std::vector<pose>>& out, Steps& steps) {
        const size_t P = ps.size();
        std::vector<bool> result(P, false);
        out.assign(P, {});
        // ---- planners the batch cannot take plan on their own, in their turn ----
        const Planner* ref = Planner::batchReference(ps);
        std::vector<size_t> grp;
        bool told = false;
        for (size_t i = 0; i < P; ++i) {
            if (ps[i]->batchable(ref)) grp.push_back(i);
            else result[i] = ps[i]->planAlone(out[i], corridorConstraint, told);
        }
        if (grp.empty()) return result;
        Planner* lead = ps[grp[0]];
        if (!steps.ready(lead)) {
            Planner::planWithoutDevice(ps, grp, corridorConstraint, out, result);
            return result;
        }
        const size_t G = grp.size();
        std::vector<typename Planner::PlanState> st;
        std::vector<bool> active(G, true), valid(G, false);
        for (size_t g = 0; g < G; ++g) st.push_back(ps[grp[g]]->beginBatch(corridorConstraint));
        bool ok = true;
        while (ok) {
            std::vector<size_t> act;
            for (size_t g = 0; g < G; ++g) {
                if (!active[g]) continue;
                if (ps[grp[g]]->timedOutBeforeRound(st[g], G)) active[g] = false;
                else act.push_back(g);
            }
            if (act.empty()) break;
            // ---- the QPs: one device call per group of active planners with the same waypoint count and group key; the
            // groups are re-formed every round (paths grow when waypoints are inserted) ----
            std::vector<bool> solved(G, false);
            for (size_t a0 = 0; a0 < act.size() && ok; ++a0) {
                const size_t g0 = act[a0];
                if (solved[g0]) continue;
                solved[g0] = true;
                Planner* p0 = ps[grp[g0]];
                const int W = (int)p0->path_.size();
                if (p0->hostQpOnly() || !steps.supported(W, p0->diffDegree_, p0->continuityDegree_)) {
                    p0->solveOnHost(st[g0]);   // the host QP, same algorithm
                    continue;
                }
                std::vector<size_t> members{g0};
                for (size_t a = a0 + 1; a < act.size(); ++a) {
                    const size_t g = act[a];
                    if (!solved[g] && (int)ps[grp[g]]->path_.size() == W && p0->sameQpGroup(st[g0], *ps[grp[g]], st[g])) {
                        members.push_back(g);
                        solved[g] = true;
                    }
                }
                std::vector<QpMember> qp;
                for (size_t g : members) qp.push_back(ps[grp[g]]->qpMember(g, st[g]));
                ok = steps.solve(p0->diffDegree_, p0->continuityDegree_, p0->desiredVel_, p0->corridorRes_, qp);
                for (size_t a = 0; ok && a < members.size(); ++a) ps[grp[members[a]]]->takeQpResult(st[members[a]], qp[a]);
            }
            if (!ok) break;
            // ---- the candidates: every active planner with a polynomial, unless its round needs no check ----
            std::vector<TrajCheck> cand;
            for (size_t g : act) {
                Planner* p = ps[grp[g]];
                if (!p->trajSolver_->hasSolution()) {   // nothing to sample (see the solo loop): not found
                    out[grp[g]].clear();
                    active[g] = false;
                    continue;
                }
                if (p->validWithoutCheck(st[g])) {
                    valid[g] = true;
                    active[g] = false;
                    continue;
                }
                cand.push_back({g, p->trajSolver_.get(), p->delT_, p->path_.back(), 0, false, {}});
            }
            // ---- every candidate checked whole by ONE device call; verdicts and colliding segments come back ----
            ok = steps.check(cand);
            if (!ok) std::cout << Planner::batchTag() << "device trajectory check failed: " << steps.lastError() << std::endl;
            for (size_t a = 0; ok && a < cand.size(); ++a) {
                const size_t g = cand[a].who;
                Planner* p = ps[grp[g]];
                if (cand[a].status != VIGO_TRAJ_OK) p->checkOnHost(*lead, cand[a]);   // a trajectory the device entry rejects
                valid[g] = !cand[a].collides;
                if (!p->advance(st[g], cand[a].collides, cand[a].segments) || p->timedOutAfterRound(st[g], G)) active[g] = false;
            }
        }
        // ---- the returned trajectories: sampled on the host once, after the loop.  A failed device step ends the batch
        // here too: every planner not yet valid gets its class's ending for "not found" ----
        for (size_t g = 0; g < G; ++g) result[grp[g]] = ps[grp[g]]->finishBatch(out[grp[g]], valid[g]);
        return result;
    }
};

}  // namespace vigo_host
#endif  /* VIGO_HOST_POLY_BATCH_LOOP_H */
