// polyBatch.h — internal to the host facades: what both min-snap planners (polyTrajOctomap, polyTrajOccMap) share.  The two
// device steps of a makePlanBatch round (the QP of one group, the whole-trajectory check of every candidate) live here with
// their staging buffers: the layout of those C ABI entries is known in ONE place; the lock-step loops stay in each class.
#ifndef VIGO_HOST_POLY_BATCH_H
#define VIGO_HOST_POLY_BATCH_H
#include <trajectory_planner/polyTrajSolver.h>

#include <chrono>
#include <cstdint>
#include <set>
#include <vector>

#include "../../../include/vigo.h"
#include "devbuf.h"

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

// ---- the device QP of one group: T paths of the same waypoint count W, degree 7, in ONE vigo_minsnap launch ----
struct QpMember {
    const std::vector<trajPlanner::pose>* path;
    const std::vector<double>* corridor;    // in: radius per segment; nullptr (for the whole group): no corridor boxes
    const geometry_msgs::Twist* conds[4];   // in: start / end vel, start / end acc; nullptr (whole group): none passed, not zeros
    int32_t status;                         // out: 0 solved, -1 numerical failure, -2 infeasible corridor
    std::vector<double> sol[3];             // out: the solution per axis, as polyTrajSolver::installSolution takes it
};

// false on a failed copy or launch (the members' outputs are then not written).  The mode (corridors, conditions) is the
// whole group's: member 0 decides it.
inline bool minsnapGroupOnDevice(vigo_context* dev, int diffDegree, int continuityDegree, double desiredVel, double corridorRes,
                                 std::vector<QpMember>& members) {
    // reused by every batch of this thread, whichever planner class it serves: every call uploads before it launches
    static thread_local StagingBuf bWp, bCor, bCnd, bCo, bKn, bSt;
    if (members.empty()) return true;
    const int D = 8, T = (int)members.size(), W = (int)members[0].path->size(), K = W - 1;
    const bool corridors = members[0].corridor != nullptr, conds = members[0].conds[0] != nullptr;
    std::vector<double> hWp, hCor, hCnd, hCo((size_t)T * K * 3 * D);
    std::vector<int32_t> hSt(T);
    for (const QpMember& m : members) {
        appendXyz(*m.path, hWp);
        if (corridors) hCor.insert(hCor.end(), m.corridor->begin(), m.corridor->end());
        for (int c = 0; conds && c < 4; ++c) {
            hCnd.push_back(m.conds[c]->linear.x); hCnd.push_back(m.conds[c]->linear.y); hCnd.push_back(m.conds[c]->linear.z);
        }
    }
    const bool ok = bWp.upload(hWp.data(), hWp.size() * 8) && (!corridors || bCor.upload(hCor.data(), hCor.size() * 8)) &&
        (!conds || bCnd.upload(hCnd.data(), hCnd.size() * 8)) && bCo.alloc(hCo.size() * 8) && bKn.alloc((size_t)T * W * 8) &&
        bSt.alloc((size_t)T * 4) &&
        vigo_minsnap(dev, T, W, 7, diffDegree, continuityDegree, desiredVel, corridorRes, (const double*)bWp.p,
                     corridors ? (const double*)bCor.p : nullptr, conds ? (const double*)bCnd.p : nullptr, (double*)bCo.p, (double*)bKn.p,
                     (int32_t*)bSt.p) == VIGO_OK &&
        bCo.download(hCo.data(), hCo.size() * 8) && bSt.download(hSt.data(), (size_t)T * 4);
    for (int a = 0; ok && a < T; ++a) {   // a member's block [K][3][8] of the coefficients -> its per-axis solutions
        members[a].status = hSt[a];
        for (int c = 0; c < 3; ++c) {
            members[a].sol[c].resize((size_t)K * D);
            for (int sgm = 0; sgm < K; ++sgm)
                for (int d = 0; d < D; ++d) members[a].sol[c][sgm * D + d] = hCo[(((size_t)a * K + sgm) * 3 + c) * D + d];
        }
    }
    return ok;
}

// ---- the whole-trajectory check of one round: every candidate in ONE launch of a vigo_traj_*_check entry ----
struct TrajCheck {
    size_t who;                            // the caller's own index of this candidate (not read here)
    trajPlanner::polyTrajSolver* solver;   // in: the installed polynomial (device QP, host QP or a kept one) and its own knots
    double delT;
    trajPlanner::pose end;                 // in: the appended last waypoint
    int32_t status;                        // out: VIGO_TRAJ_OK, or the entry rejects it: the caller checks it on the host
    bool collides;
    std::set<int> segments;                // out: collisionSeg
};

// launch(T, S, seg_off, coeffs, knots, delT, endpoint, out_status, out_n, out_flag, out_first, out_seg) makes the one call
// with the device arrays both entries take, in their order in include/vigo.h (the entry and its own extra arguments stay
// with the caller), and says whether it succeeded; only the verdicts come back.  False on a failed copy or launch.
template <class Launch>
inline bool checkTrajectoriesOnDevice(std::vector<TrajCheck>& cands, Launch launch) {
    // a set of its own: the QP step's coefficients buffer keeps the last group's, this one holds the whole round's
    static thread_local StagingBuf cOff, cCo, cKn, cDt, cEp, cSt, cN, cFl, cFi, cSeg;
    const int D = 8, T = (int)cands.size();
    if (T == 0) return true;
    std::vector<int32_t> segOff(1, 0);
    std::vector<double> hCo, hKn, hDt, hEp;
    for (const TrajCheck& c : cands) {
        const std::vector<double>& kn = c.solver->getTimeKnot();
        const int K = (int)kn.size() - 1;
        for (int sgm = 0; sgm < K; ++sgm)          // the solver's per-axis solutions laid out as [K][3][8]
            for (int ax = 0; ax < 3; ++ax) {
                const std::vector<double>& sol = c.solver->getSolution(ax);
                hCo.insert(hCo.end(), sol.begin() + (size_t)sgm * D, sol.begin() + (size_t)(sgm + 1) * D);
            }
        hKn.insert(hKn.end(), kn.begin(), kn.end());
        hDt.push_back(c.delT);
        hEp.push_back(c.end.x); hEp.push_back(c.end.y); hEp.push_back(c.end.z);
        segOff.push_back(segOff.back() + K);
    }
    const int S = segOff.back();
    std::vector<int32_t> hStat(T);
    std::vector<uint8_t> hFlag(T), hSeg(S);
    const bool ok = cOff.upload(segOff.data(), segOff.size() * 4) && cCo.upload(hCo.data(), hCo.size() * 8) &&
        cKn.upload(hKn.data(), hKn.size() * 8) && cDt.upload(hDt.data(), hDt.size() * 8) && cEp.upload(hEp.data(), hEp.size() * 8) &&
        cSt.alloc((size_t)T * 4) && cN.alloc((size_t)T * 4) && cFl.alloc((size_t)T) && cFi.alloc((size_t)T * 4) && cSeg.alloc((size_t)S) &&
        launch(T, S, (const int32_t*)cOff.p, (const double*)cCo.p, (const double*)cKn.p, (const double*)cDt.p, (const double*)cEp.p,
               (int32_t*)cSt.p, (int32_t*)cN.p, (uint8_t*)cFl.p, (int32_t*)cFi.p, (uint8_t*)cSeg.p) &&
        cSt.download(hStat.data(), (size_t)T * 4) && cFl.download(hFlag.data(), (size_t)T) && cSeg.download(hSeg.data(), (size_t)S);
    for (int a = 0; ok && a < T; ++a) {
        cands[a].status = hStat[a];
        cands[a].collides = hFlag[a] != 0;
        for (int sgm = 0; sgm < segOff[a + 1] - segOff[a]; ++sgm)
            if (hSeg[segOff[a] + sgm]) cands[a].segments.insert(sgm);
    }
    return ok;
}

}  // namespace vigo_host
#endif  /* VIGO_HOST_POLY_BATCH_H */
