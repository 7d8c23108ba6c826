// polyBatch.h — internal to the host facades: the two device steps of a makePlanBatch round of both min-snap planners
// (polyTrajOctomap, polyTrajOccMap) — the QP of one group, the whole-trajectory check of every candidate — with their
// staging buffers: the layout of those C ABI entries is known in ONE place.  The lock-step loop that drives them, and the
// structs they fill, are polyBatchLoop.h's; each class's DeviceSteps binds its own entry point to them.
#ifndef VIGO_HOST_POLY_BATCH_H
#define VIGO_HOST_POLY_BATCH_H
#include "devbuf.h"
#include "polyBatchLoop.h"

namespace vigo_host {

// ---- the device QP of one group: T paths of the same waypoint count W, degree 7, in ONE vigo_minsnap launch ----
// false on a failed copy or launch (the members' outputs are then not written).  The mode (corridors, conditions) is the
// whole group's: member 0 decides it.
inline bool minsnapGroupOnDevice(vigo_context* dev, int diffDegree, int continuityDegree, double desiredVel, double corridorRes,
                                 std::vector<QpMember>& members) {
    // reused by every batch of this thread, whichever planner class it serves: every call uploads before it launches
    struct Stage {
        Staged<double> wp, corridor, conds, coeffs, knots;
        Staged<int32_t> status;
    };
    static thread_local Stage st;
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
    const bool ok = st.wp.upload(hWp) && (!corridors || st.corridor.upload(hCor)) && (!conds || st.conds.upload(hCnd)) &&
        st.coeffs.alloc(hCo.size()) && st.knots.alloc((size_t)T * W) && st.status.alloc(hSt.size()) &&
        vigo_minsnap(dev, T, W, 7, diffDegree, continuityDegree, desiredVel, corridorRes, st.wp.get(), corridors ? st.corridor.get() : nullptr,
                     conds ? st.conds.get() : nullptr, st.coeffs.get(), st.knots.get(), st.status.get()) == VIGO_OK &&
        st.coeffs.download(hCo) && st.status.download(hSt);
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
// launch(T, S, seg_off, coeffs, knots, delT, endpoint, out_status, out_n, out_flag, out_first, out_seg) makes the one call
// with the device arrays both entries take, in their order in include/vigo.h (the entry and its own extra arguments stay
// with the caller), and says whether it succeeded; only the verdicts come back.  False on a failed copy or launch.
template <class Launch>
inline bool checkTrajectoriesOnDevice(std::vector<TrajCheck>& cands, Launch launch) {
    // a set of its own: the QP step's coefficients buffer keeps the last group's, this one holds the whole round's
    struct Stage {
        Staged<int32_t> segOff, status, n, first;
        Staged<double> coeffs, knots, delT, endpoint;
        Staged<uint8_t> flag, seg;
    };
    static thread_local Stage st;
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
    const bool ok = st.segOff.upload(segOff) && st.coeffs.upload(hCo) && st.knots.upload(hKn) && st.delT.upload(hDt) && st.endpoint.upload(hEp) &&
        st.status.alloc(hStat.size()) && st.n.alloc((size_t)T) && st.flag.alloc(hFlag.size()) && st.first.alloc((size_t)T) && st.seg.alloc(hSeg.size()) &&
        launch(T, S, st.segOff.get(), st.coeffs.get(), st.knots.get(), st.delT.get(), st.endpoint.get(), st.status.get(), st.n.get(), st.flag.get(),
               st.first.get(), st.seg.get()) &&
        st.status.download(hStat) && st.flag.download(hFlag) && st.seg.download(hSeg);
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
