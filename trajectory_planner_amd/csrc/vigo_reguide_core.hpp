// vigo_reguide_core.hpp — the rules of the re-guide step of the rebound loop (the `if (hasCollision)` block of
// BT.cpp:656-675) around the searches and the guide step, as the kernels of vigo_reguide.hip run them and the host
// compiles too (host/src/cabi_host.cpp: vigo_host_rebound_reguide_core; tests/test_reguide_core.py pins it against the
// facade's own reboundStep and a Python restatement of isReguideRequired).
//
//   reguide_guide_far   isControlPointRequireNewGuide's test of ONE guide pair (BT.h:417-429): dthresh - dist > 0 keeps
//                       the control point's guides.  The dot product ((c - p) . d summed x, y, then z), compiled
//                       without contraction.
//   reguide_rules       isReguideRequired (BT.cpp:573-608; host/src/bsplineTraj.cpp:646-659): findCollisionSeg on the
//                       current control points (collision_segs of vigo_pathsearch_core.hpp), compareCollisionSeg against
//                       the previous segments (BT.h:379-403: the interior control points of every new segment, and BOTH
//                       ends of a segment without interior points; a point a previous segment holds, ends included, is
//                       "overlapped", the others "fresh"), then the std::set<int> of new-segment indices: the
//                       findCollisionSegIndex (the FIRST new segment that holds the point, ends included) of every
//                       fresh point and of every overlapped point whose guides all fail the test above (a point without
//                       guides fails it).  -1 is erased (it cannot arise: a compared point lies inside its own segment).
//                       The re-guide list is the new segments whose index is in the set, in ascending index.
//   reguide_outcome     what the step does with a trajectory, from the list, the search and the guide step.
//   reguide_commit      the state transition of BT.cpp:656-679 for the outcomes that are not deferred.
//
// k_rebound_decide (vigo_reguide.hip) asks reguide_rules the yes/no: a list that is not empty, or more new segments than
// the state holds, hands the trajectory to the host.  The forced A* of failCount >= 4 (BT.cpp:640-654) is NOT here: it
// precedes isReguideRequired and changes the guides that step reads, and stays with the host.
//
// Integer logic and one fp64 dot product.
#pragma once

#include "vigo_pathsearch_core.hpp"

namespace vigo {

// per-trajectory status of vigo_rebound_reguide (include/vigo.h VIGO_REGUIDE_*)
enum {
    kReguideDone = 0,            // re-guided: new segments, appended guides, paths
    kReguideSearchFailed = 1,    // the list's path search failed: new segments, weights[0] *= 2, ++fail_count
    kReguideNotRequired = 2,     // an empty list: the same transition
    kReguideDeferred = 3,        // the state is untouched: the host steps decide
    kReguideSkipped = 4,         // not eligible: nothing of the trajectory is touched
};

// pv: (point, direction) of one guide pair; c: the control point
VIGO_HD bool reguide_guide_far(double dthresh, const double* c, const double* pv) {
    const double dist = ((c[0] - pv[0]) * pv[3] + (c[1] - pv[1]) * pv[4]) + (c[2] - pv[2]) * pv[5];
    return !(dthresh - dist > 0);
}

// occ(i), line(i): the flags of findCollisionSeg (collision_segs); prev[n_prev][2]: collisionSeg_ before the step;
// need_guide(i): isControlPointRequireNewGuide(i).  Returns the number of new segments n; when n <= cap the segments are
// in seg[n][2], listed[k] != 0 marks the ones of the re-guide list and *n_list counts them.  (n > cap: seg holds the
// first cap, listed and *n_list are not written.)
template <class Occ, class Line, class NeedGuide>
VIGO_HD int reguide_rules(int N, double not_check_ratio, const Occ& occ, const Line& line, int n_prev, const int32_t* prev,
                          const NeedGuide& need_guide, int cap, int32_t* seg, uint8_t* listed, int* n_list) {
    const int n = collision_segs(N, not_check_ratio, occ, line, cap, seg);
    if (n > cap) return n;
    for (int k = 0; k < n; ++k) listed[k] = 0;
    auto in_prev = [&](int i) {
        for (int k = 0; k < n_prev; ++k)
            if (i >= prev[2 * k] && i <= prev[2 * k + 1]) return true;
        return false;
    };
    auto index_of = [&](int i) {                               // findCollisionSegIndex on the new segments
        for (int k = 0; k < n; ++k)
            if (i >= seg[2 * k] && i <= seg[2 * k + 1]) return k;
        return -1;
    };
    auto visit = [&](int i) {
        if (!in_prev(i) || need_guide(i)) {
            const int k = index_of(i);
            if (k >= 0) listed[k] = 1;
        }
    };
    for (int k = 0; k < n; ++k) {
        const int a = seg[2 * k], e = seg[2 * k + 1];
        for (int i = a + 1; i <= e - 1; ++i) visit(i);
        if (e - a - 1 == 0)
            for (int i = a; i <= e; ++i) visit(i);
    }
    int m = 0;
    for (int k = 0; k < n; ++k) m += listed[k] ? 1 : 0;
    *n_list = m;
    return n;
}

// eligible: status == NEEDS_HOST, gate_static != 0, fail_count < 4.  too_many: more new segments than the state holds.
// paths_status: kPaths* of the list's path search; paths_cut: its merges left more paths than segments
// (paths_cut_by_bound: the search returns the bounded list, astarPaths_ is the whole one); guide_deferred: the guide
// step on its output deferred the trajectory.
VIGO_HD int reguide_outcome(bool eligible, bool too_many, int n_list, int paths_status, bool paths_cut, bool guide_deferred) {
    if (!eligible) return kReguideSkipped;
    if (too_many) return kReguideDeferred;
    if (n_list == 0) return kReguideNotRequired;
    if (paths_status == kPathsFailed) return kReguideSearchFailed;
    if (paths_status != kPathsOk || paths_cut || guide_deferred) return kReguideDeferred;
    return kReguideDone;
}

// BT.cpp:656-679 for Done / SearchFailed / NotRequired.  The caller stores the new segments; w: the trajectory's
// weights[4]; *status and *solve_first become "active" (0) and 1: the optimize() of BT.cpp:680 is the next call's.
VIGO_HD void reguide_commit(int outcome, bool gate_dynamic, double* w, int32_t* fail_count, int32_t* status, int32_t* solve_first) {
    if (outcome != kReguideDone) {
        w[0] *= 2.0;                                           // BT.cpp:664 / :672
        *fail_count += 1;
    }
    if (gate_dynamic) w[3] *= 2.0;                             // BT.cpp:677-679
    *status = 0;
    *solve_first = 1;
}

}  // namespace vigo
