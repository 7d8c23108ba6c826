// bsplineTrajSeed.cpp — trajPlanner::bsplineTraj, the stages before makePlanBatch for many planners at once:
// updatePathBatch (the host prologues, then the fits as device launches) and seedPathBatch (bspline_node's seed-path
// stage, on the host workers or as ONE vigo_seed_paths launch per group).
#include <trajectory_planner/bsplineTraj.h>
#include <trajectory_planner/polyTrajOccMap.h>

#include <algorithm>
#include <cstring>

#include "bsplineTrajBatch.h"
#include "seedBlock.h"

using std::cout;
using std::endl;

namespace trajPlanner {

// updatePath() for many planners: the host prologue per planner, then ONE vigo_bspline_fit launch
// per group of equal waypoint count (bspline::parameterizeToBspline, bspline.cpp:74-138, batched).
std::vector<bool> bsplineTraj::updatePathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<nav_msgs::Path>& paths,
                                               const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions) {
    return updatePathBatch(planners, paths, startEndConditions, defaultBatchOptions());
}

std::vector<bool> bsplineTraj::updatePathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<nav_msgs::Path>& paths,
                                               const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions, const BatchOptions& options,
                                               BatchStats* stats) {
    std::vector<bool> ok(planners.size(), false);
    if (stats) *stats = BatchStats();           // (none of this call's stages counts anything)
    if (paths.size() != planners.size() || startEndConditions.size() != planners.size()) return ok;
    std::vector<std::vector<Eigen::Vector3d>> fitPts(planners.size());
    std::vector<bool> ready(planners.size(), false);
    // The prologues (goal check, path-length adjustment with its line checks against the map, filling) run on the host
    // workers, each as if its predecessor had left a previous path length not above its own max_path_length — then the
    // value does not enter (BT.cpp:762: max(prevPathLength, maxPathLength_)); a serial pass hands the real value down the
    // line and repeats, in order, the rare planner for which it does enter.  Same results as one planner after another.
    std::vector<uint8_t> okv(planners.size(), 0), wrote(planners.size(), 0);
    std::vector<double> prevOut(planners.size(), 0.0);
    parallelFor(planners.size(), [&](size_t i) {
        if (startEndConditions[i].size() != 4) return;
        bool w = false;
        okv[i] = planners[i]->prepareFitPointsWith(paths[i], fitPts[i], 0.0, prevOut[i], w) ? 1 : 0;
        wrote[i] = w ? 1 : 0;
    });
    double prev = g_prevPathLength.load();
    for (size_t i = 0; i < planners.size(); ++i) {
        if (startEndConditions[i].size() == 4 && wrote[i] && prev > planners[i]->maxPathLength_) {
            bool w = false;
            okv[i] = planners[i]->prepareFitPointsWith(paths[i], fitPts[i], prev, prevOut[i], w) ? 1 : 0;
        }
        if (wrote[i]) prev = prevOut[i];
        ready[i] = okv[i] && fitPts[i].size() > 3;
    }
    g_prevPathLength.store(prev);
    fitGroups(planners, fitPts, ready, startEndConditions, ok, options.mixedFit);
    return ok;
}

namespace {
struct FitStage {
    Staged<double> pts, cond, ctrl;   // [B][K][3], [B][4][3] up; [B][K + 2][3] back
};
// the mixed fit's padded block: [B][stride][3], [B][4][3], n_fit [B] up; [B][Ns][3], n_pts [B] back
struct MixedFitStage {
    Staged<double> pts, cond, ctrl;
    Staged<int32_t> nfit, npts;
};
constexpr int kMixedFitMaxStride = 64;   // vigo_bspline_fit_mixed's largest Ns: K + 2 control points beyond it keep the per-count route
}  // namespace

// The fit stage of updatePathBatch and seedPathBatch, the control points installed (BT.cpp:315-322).  Per count: ONE
// vigo_bspline_fit launch per group of ready planners with equal point count and knot span.  With `mixed` (mixedFit) the
// ready planners of up to 62 points group by knot span alone and take ONE vigo_bspline_fit_mixed call on a padded block:
// the same control points, bit for bit (include/vigo.h); planners with more points keep the per-count route.
void bsplineTraj::fitGroups(const std::vector<bsplineTraj*>& planners, const std::vector<std::vector<Eigen::Vector3d>>& fitPts,
                            const std::vector<bool>& ready, const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions,
                            std::vector<bool>& ok, bool mixed) {
    auto viaMixed = [&](size_t a) { return mixed && ready[a] && fitPts[a].size() + 2 <= (size_t)kMixedFitMaxStride; };
    auto sameSpan = [&](size_t a, size_t b) {
        return planners[a]->controlPointsTs_ == planners[b]->controlPointsTs_ &&
               planners[a]->link_.sameTarget(planners[b]->link_);   // the fit runs on the lead's handle: a lead without a device fails its own group only
    };
    auto install = [&](const std::vector<size_t>& grp, const std::vector<double>& ctrl, size_t rowStride) {
        parallelFor(grp.size(), [&](size_t b) {
            const int N = (int)fitPts[grp[b]].size() + 2;
            Eigen::MatrixXd controlPoints;
            controlPoints.resize(3, N);
            std::memcpy(controlPoints.data(), ctrl.data() + b * rowStride * 3, sizeof(double) * 3 * N);
            planners[grp[b]]->installControlPoints(controlPoints, fitPts[grp[b]]);
        });
        for (size_t b = 0; b < grp.size(); ++b) ok[grp[b]] = true;
    };
    // the groups are formed among the candidates only: forEachGroup compares every ungrouped element with all that follow
    std::vector<size_t> mixedIdx, countIdx;
    for (size_t i = 0; i < planners.size(); ++i)
        if (ready[i]) (viaMixed(i) ? mixedIdx : countIdx).push_back(i);
    auto sameMixed = [&](size_t a, size_t b) { return sameSpan(mixedIdx[a], mixedIdx[b]); };
    vigo_host::forEachGroup(mixedIdx.size(), sameMixed, [&](const std::vector<size_t>& members) {
        std::vector<size_t> grp;
        for (size_t m : members) grp.push_back(mixedIdx[m]);
        bsplineTraj* lead = planners[grp[0]];
        if (!lead->syncDevice()) return;
        const int B = (int)grp.size();
        size_t stride = 0;
        for (size_t i : grp) stride = std::max(stride, fitPts[i].size());
        const int Ns = std::max(7, (int)stride + 2);
        std::vector<double> pts((size_t)B * stride * 3, 0.0), cond((size_t)B * 12), ctrl((size_t)B * Ns * 3);
        std::vector<int32_t> nfit((size_t)B), npts((size_t)B);
        for (int b = 0; b < B; ++b) {
            const std::vector<Eigen::Vector3d>& f = fitPts[grp[b]];
            nfit[b] = (int32_t)f.size();
            for (size_t i = 0; i < f.size(); ++i)
                for (int q = 0; q < 3; ++q) pts[((size_t)b * stride + i) * 3 + q] = f[i](q);
            for (int i = 0; i < 4; ++i)
                for (int q = 0; q < 3; ++q) cond[((size_t)b * 4 + i) * 3 + q] = startEndConditions[grp[b]][i](q);
        }
        static thread_local MixedFitStage st;
        vigo_handle_t h = lead->link_.handle();
        if (!st.pts.upload(pts) || !st.cond.upload(cond) || !st.nfit.upload(nfit) || !st.ctrl.alloc(ctrl.size()) || !st.npts.alloc(npts.size())) return;
        if (!deviceCallOk(vigo_bspline_fit_mixed(h, B, Ns, lead->controlPointsTs_, st.nfit.get(), nullptr, st.pts.get(), (int)stride, st.cond.get(),
                                                 st.ctrl.get(), st.npts.get()),
                          "vigo_bspline_fit_mixed", h))
            return;
        if (!st.ctrl.download(ctrl) || !st.npts.download(npts)) return;   // (each waits for the stream: the call is done)
        for (int b = 0; b < B; ++b)
            if (npts[b] != nfit[b] + 2) return;                  // (every count was in range: cannot happen)
        install(grp, ctrl, (size_t)Ns);
    });
    auto sameFit = [&](size_t a, size_t b) {
        return fitPts[countIdx[a]].size() == fitPts[countIdx[b]].size() && sameSpan(countIdx[a], countIdx[b]);
    };
    vigo_host::forEachGroup(countIdx.size(), sameFit, [&](const std::vector<size_t>& members) {
        std::vector<size_t> grp;
        for (size_t m : members) grp.push_back(countIdx[m]);
        bsplineTraj* lead = planners[grp[0]];
        const int K = (int)fitPts[grp[0]].size();
        const double ts = lead->controlPointsTs_;
        if (K + 2 > VIGO_MAX_CTRL_POINTS || !lead->syncDevice()) return;
        const int B = (int)grp.size();
        std::vector<double> pts((size_t)B * K * 3), cond((size_t)B * 12), ctrl((size_t)B * (K + 2) * 3);
        for (int b = 0; b < B; ++b) {
            for (int i = 0; i < K; ++i)
                for (int q = 0; q < 3; ++q) pts[((size_t)b * K + i) * 3 + q] = fitPts[grp[b]][i](q);
            for (int i = 0; i < 4; ++i)
                for (int q = 0; q < 3; ++q) cond[((size_t)b * 4 + i) * 3 + q] = startEndConditions[grp[b]][i](q);
        }
        static thread_local FitStage st;
        vigo_handle_t h = lead->link_.handle();
        if (!st.pts.upload(pts) || !st.cond.upload(cond) || !st.ctrl.alloc(ctrl.size())) return;
        if (!deviceCallOk(vigo_bspline_fit(h, B, K, ts, st.pts.get(), st.cond.get(), st.ctrl.get()), "vigo_bspline_fit", h)) return;
        if (!vigo_host::threadSync() || !st.ctrl.download(ctrl)) return;
        install(grp, ctrl, (size_t)K + 2);
    });
}

// ---- the seed-path stage for many planners (bspline_node.cpp:317-378): seedPathBatch -------------------------------
namespace {
constexpr int kSeedPointCap = 128;   // rows of the launch's seed / fit outputs per planner; a longer list is the host's
}  // namespace

// bspline_node.cpp:338-352 for one planner, the loop ending on the try count
void bsplineTraj::seedSearchWith(polyTrajOccMap& poly, double dt0, int maxTries, double prevIn, SeedInfo& s, nav_msgs::Path& seed) {
    s = SeedInfo();
    s.dt = dt0;
    seed.poses.clear();
    double prev = prevIn;
    for (int k = 0; k < maxTries; ++k) {
        ++s.tries;
        const nav_msgs::Path input = poly.getTrajectory(s.dt);
        bool wrote = false;
        double prevOut = prev;
        const bool ok = this->inputPathCheckWith(input, seed, s.dt, s.finalTime, prev, prevOut, wrote);
        if (wrote) {
            prev = prevOut;
            s.wrote = true;
        }
        if (ok) {
            s.found = true;
            break;
        }
        s.dt *= 0.8;
    }
    s.prevOut = prev;
}

void bsplineTraj::seedSteps(polyTrajOccMap& poly, double dt0, int maxTries, double prevSeedIn, double prevFitIn, SeedSteps& out) {
    out = SeedSteps();
    this->seedSearchWith(poly, dt0, maxTries, prevSeedIn, out.search, out.seed);
    out.fitOk = this->prepareFitPointsWith(out.seed, out.fitPoints, prevFitIn, out.prevFitOut, out.fitWrote);
}

// one seedPathBatch call: its options, and what it keeps per planner between its passes
struct bsplineTraj::SeedBatch {
    const BatchOptions o;
    std::vector<nav_msgs::Path> seed;
    std::vector<SeedInfo> info;
    std::vector<std::vector<Eigen::Vector3d>> fitPts;
    std::vector<uint8_t> eligible, onDevice, okv, wroteFit;
    std::vector<double> prevFitOut;
    // mixedFit: the control points vigo_bspline_fit_mixed made of the launch's own fit points ([K + 2][3]; empty: none)
    const std::vector<std::vector<Eigen::Vector3d>>* conds = nullptr;
    std::vector<std::vector<double>> devCtrl;
    SeedBatch(size_t n, const BatchOptions& options)
        : o(options), seed(n), info(n), fitPts(n), eligible(n, 0), onDevice(n, 0), okv(n, 0), wroteFit(n, 0), prevFitOut(n, 0.0), devCtrl(n) {}
};

namespace {
struct SeedStage {
    Staged<double> in, out;   // the two blocks of seedBlock.h, as whole doubles
    Staged<double> ctrl;      // mixedFit: [T][kMixedFitMaxStride][3] of vigo_bspline_fit_mixed ...
    Staged<int32_t> npts;     // ... and its counts
    Staged<double> cut;       // ... the seed, fit and control-point rows cut to the group's largest counts, packed for ONE download
};
// rows [0, rows) of each of the T blocks of srcRows rows of xyz, packed, device to device (a strided copy into the block
// that goes down whole: a strided copy into pageable host memory is staged row by row); on the thread's stream
bool cutRows(double* dst, const double* src, size_t T, size_t srcRows, size_t rows) {
    if (T == 0 || rows == 0) return true;
    return hipMemcpy2DAsync(dst, rows * 24, src, srcRows * 24, rows * 24, T, hipMemcpyDeviceToDevice, vigo_host::threadStream()) == hipSuccess;
}
}  // namespace

// ONE vigo_seed_paths launch per group of eligible planners that share a device batch and a polynomial degree, as if
// every predecessor had left a previous path length of 0; one upload, one download.  A trajectory the launch defers or
// refuses stays with the host steps.
// With mixedFit the conditions travel up with the inputs and vigo_bspline_fit_mixed runs on the launch's own
// out_fit / out_fit_n / out_status, nothing downloaded in between; what comes down is the per-planner scalars, then the
// control points and the seed / fit rows cut to the group's largest counts instead of point_cap rows each.
void bsplineTraj::seedOnDevice(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys, SeedBatch& sb) {
    auto same = [&](size_t a, size_t b) {
        // (whatever control points the planners hold from before: the launch reads none of them)
        return sb.eligible[a] && sb.eligible[b] && planners[a]->sameBatchKeyAnyCount(*planners[b]) &&
               polys[a]->getSolver()->getPolyDegree() == polys[b]->getSolver()->getPolyDegree();
    };
    vigo_host::forEachGroup(planners.size(), same, [&](const std::vector<size_t>& grp) {
        bsplineTraj* lead = planners[grp[0]];
        const int deg = polys[grp[0]]->getSolver()->getPolyDegree();
        if (deg < 0 || deg > 15 || !lead->syncDevice()) return;
        const int T = (int)grp.size(), cap = kSeedPointCap;
        std::vector<int32_t> segOff(1, 0);
        for (size_t i : grp) segOff.push_back(segOff.back() + (int32_t)polys[i]->getSolver()->timeKnots().size() - 1);
        const int S = segOff.back();
        // the inputs as one block, the outputs as another (seedBlock.h): `in` is the host's view, filled here
        vigo_host::SeedIn in, dIn;
        vigo_host::SeedOut out, dOut;
        const bool chain = sb.o.mixedFit && sb.conds;
        double *conds = nullptr, *dConds = nullptr;
        std::vector<double> inBlock((chain ? vigo_host::seedInBlockWithConds(nullptr, T, S, deg, in, conds) : vigo_host::seedInBlock(nullptr, T, S, deg, in)) /
                                    sizeof(double));
        std::vector<double> outBlock(vigo_host::seedOutBlock(nullptr, T, cap, out) / sizeof(double));
        if (chain) {
            vigo_host::seedInBlockWithConds(inBlock.data(), T, S, deg, in, conds);
            for (int b = 0; b < T; ++b)
                for (int i = 0; i < 4; ++i)
                    for (int q = 0; q < 3; ++q) conds[((size_t)b * 4 + i) * 3 + q] = (*sb.conds)[grp[b]][i](q);
        } else {
            vigo_host::seedInBlock(inBlock.data(), T, S, deg, in);
        }
        std::copy(segOff.begin(), segOff.end(), in.segOff);
        for (int b = 0; b < T; ++b) {
            bsplineTraj* p = planners[grp[b]];
            const polyTrajSolver* sol = polys[grp[b]]->getSolver();
            in.duration[b] = polys[grp[b]]->getDuration();
            in.dt0[b] = p->getInitTs();
            in.controlPointDistance[b] = p->controlPointDistance_;
            in.maxPathLength[b] = p->maxPathLength_;
            in.prevSeed[b] = 0.0;
            in.prevFit[b] = 0.0;
            const std::vector<double>& k = sol->timeKnots();
            std::copy(k.begin(), k.end(), in.knots + segOff[b] + b);
            for (int sgm = 0; sgm < segOff[b + 1] - segOff[b]; ++sgm)
                for (int ax = 0; ax < 3; ++ax)
                    std::copy(sol->getSolution(ax).begin() + (size_t)sgm * (deg + 1), sol->getSolution(ax).begin() + (size_t)(sgm + 1) * (deg + 1),
                              in.coeffs + ((size_t)(segOff[b] + sgm) * 3 + ax) * (deg + 1));
        }
        static thread_local SeedStage st;
        vigo_handle_t h = lead->link_.handle();
        if (!st.in.upload(inBlock) || !st.out.alloc(outBlock.size())) return;
        if (chain) vigo_host::seedInBlockWithConds(st.in.get(), T, S, deg, dIn, dConds);
        else vigo_host::seedInBlock(st.in.get(), T, S, deg, dIn);
        vigo_host::seedOutBlock(st.out.get(), T, cap, dOut);
        if (!deviceCallOk(vigo_seed_paths(h, T, S, deg, dIn.segOff, dIn.coeffs, dIn.knots, dIn.duration, dIn.dt0, dIn.controlPointDistance,
                                          dIn.maxPathLength, dIn.prevSeed, dIn.prevFit, sb.o.seedMaxTries, cap, dOut.status, dOut.tries, dOut.dt,
                                          dOut.finalTime, dOut.seedN, dOut.seed, dOut.fitN, dOut.fit, dOut.prevSeed, dOut.prevFit),
                          "vigo_seed_paths", h))
            return;
        vigo_host::seedOutBlock(outBlock.data(), T, cap, out);
        const int32_t *status = out.status, *tries = out.tries, *seedN = out.seedN, *fitN = out.fitN;
        const double *dt = out.dt, *finalTime = out.finalTime, *prevSeedOut = out.prevSeed, *prevFitOut = out.prevFit;
        const double *seedPts = out.seed, *fitPts = out.fit;
        size_t seedRows = cap, fitRows = cap, ctrlRows = 0;      // rows per planner of the host copies below
        std::vector<int32_t> npts;
        std::vector<double> cut;
        const double* ctrlCut = nullptr;
        if (chain) {
            const int Ns = kMixedFitMaxStride;
            if (!st.ctrl.alloc((size_t)T * Ns * 3) || !st.npts.alloc((size_t)T)) return;
            if (!deviceCallOk(vigo_bspline_fit_mixed(h, T, Ns, lead->controlPointsTs_, dOut.fitN, dOut.status, dOut.fit, cap, dConds, st.ctrl.get(),
                                                     st.npts.get()),
                              "vigo_bspline_fit_mixed", h))
                return;
            // the scalars are the head of the out block: they say how many rows of each list are worth the copy
            npts.resize((size_t)T);
            const size_t scalars = (size_t)(reinterpret_cast<const char*>(out.seed) - reinterpret_cast<const char*>(outBlock.data()));
            if (!st.npts.download(npts) || !vigo_host::download(outBlock.data(), st.out.get(), scalars)) return;
            seedRows = fitRows = 0;
            for (int b = 0; b < T; ++b) {
                if (status[b] == VIGO_SEED_DEFERRED || status[b] == VIGO_SEED_BAD_INPUT) continue;
                if (seedN[b] < 0 || seedN[b] > cap || fitN[b] < 0 || fitN[b] > cap || npts[b] < 0 || npts[b] > Ns) return;
                seedRows = std::max(seedRows, (size_t)seedN[b]);
                fitRows = std::max(fitRows, (size_t)fitN[b]);
                ctrlRows = std::max(ctrlRows, (size_t)npts[b]);
            }
            const size_t nSeed = (size_t)T * seedRows * 3, nFit = (size_t)T * fitRows * 3, nCtrl = (size_t)T * ctrlRows * 3;
            cut.resize(nSeed + nFit + nCtrl);
            if (!st.cut.alloc(cut.size())) return;
            if (!cutRows(st.cut.get(), dOut.seed, T, cap, seedRows) || !cutRows(st.cut.get() + nSeed, dOut.fit, T, cap, fitRows) ||
                !cutRows(st.cut.get() + nSeed + nFit, st.ctrl.get(), T, Ns, ctrlRows) || !st.cut.download(cut))
                return;
            seedPts = cut.data();
            fitPts = cut.data() + nSeed;
            ctrlCut = cut.data() + nSeed + nFit;
        } else if (!vigo_host::threadSync() || !st.out.download(outBlock)) {
            return;
        }
        parallelFor((size_t)T, [&](size_t b) {
            const size_t i = grp[b];
            if (status[b] == VIGO_SEED_DEFERRED || status[b] == VIGO_SEED_BAD_INPUT) return;
            SeedInfo& s = sb.info[i];
            s = SeedInfo();
            s.found = status[b] != VIGO_SEED_NO_SPACING;
            s.tries = tries[b];
            s.dt = dt[b];
            s.finalTime = finalTime[b];
            s.wrote = !(status[b] == VIGO_SEED_TOO_SHORT && seedN[b] == 0);
            s.prevOut = prevSeedOut[b];
            std::vector<Eigen::Vector3d> pts;
            for (int q = 0; q < seedN[b]; ++q) {
                const double* v = seedPts + ((size_t)b * seedRows + q) * 3;
                pts.push_back(Eigen::Vector3d(v[0], v[1], v[2]));
            }
            sb.seed[i].poses.clear();
            if (!pts.empty()) planners[i]->eigenPointsToPathMsg(pts, sb.seed[i]);
            sb.fitPts[i].clear();
            for (int q = 0; q < fitN[b]; ++q) {
                const double* v = fitPts + ((size_t)b * fitRows + q) * 3;
                sb.fitPts[i].push_back(Eigen::Vector3d(v[0], v[1], v[2]));
            }
            sb.okv[i] = status[b] == VIGO_SEED_OK ? 1 : 0;
            sb.wroteFit[i] = sb.okv[i];
            sb.prevFitOut[i] = prevFitOut[b];
            sb.onDevice[i] = 1;
            sb.devCtrl[i].clear();
            if (chain && status[b] == VIGO_SEED_OK && npts[b] == fitN[b] + 2 && planners[i]->controlPointsTs_ == lead->controlPointsTs_)
                sb.devCtrl[i].assign(ctrlCut + b * ctrlRows * 3, ctrlCut + (b * ctrlRows + (size_t)npts[b]) * 3);
        });
    });
}

std::vector<bool> bsplineTraj::seedPathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys,
                                             const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions,
                                             std::vector<nav_msgs::Path>* seeds, std::vector<SeedInfo>* info) {
    return seedPathBatch(planners, polys, startEndConditions, defaultBatchOptions(), nullptr, seeds, info);
}

std::vector<bool> bsplineTraj::seedPathBatch(const std::vector<bsplineTraj*>& planners, const std::vector<polyTrajOccMap*>& polys,
                                             const std::vector<std::vector<Eigen::Vector3d>>& startEndConditions, const BatchOptions& options,
                                             BatchStats* stats, std::vector<nav_msgs::Path>* seeds, std::vector<SeedInfo>* info) {
    const size_t n = planners.size();
    std::vector<bool> ok(n, false);
    BatchStats st;
    if (polys.size() != n || startEndConditions.size() != n) {
        reportBatchStats(st, stats);
        return ok;
    }
    SeedBatch sb(n, options.normalized());
    sb.conds = &startEndConditions;
    if (sb.o.deviceSeed) {
        for (size_t i = 0; i < n; ++i) {
            const polyTrajSolver* sol = polys[i]->getSolver();
            sb.eligible[i] = startEndConditions[i].size() == 4 && planners[i]->link_.map() && sol && sol->hasSolution() &&
                             !polys[i]->usesPwlFallback();
        }
        seedOnDevice(planners, polys, sb);
    }
    // The searches run as if every predecessor had left a previous path length not above the planner's own
    // max_path_length — then the value does not enter (BT.cpp:762) — and a serial pass in the reference's order (every
    // planner's search, then every planner's updatePath) hands the real value down and repeats, on the host and in
    // order, the rare planner for which it does enter: updatePathBatch's scheme, over both phases.
    parallelFor(n, [&](size_t i) {
        if (!sb.onDevice[i]) planners[i]->seedSearchWith(*polys[i], planners[i]->getInitTs(), sb.o.seedMaxTries, 0.0, sb.info[i], sb.seed[i]);
    });
    double prev = g_prevPathLength.load();
    std::vector<uint8_t> redone(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (sb.info[i].wrote && prev > planners[i]->maxPathLength_) {
            planners[i]->seedSearchWith(*polys[i], planners[i]->getInitTs(), sb.o.seedMaxTries, prev, sb.info[i], sb.seed[i]);
            redone[i] = 1;
        }
        if (sb.info[i].wrote) prev = sb.info[i].prevOut;
    }
    parallelFor(n, [&](size_t i) {
        if ((sb.onDevice[i] && !redone[i]) || startEndConditions[i].size() != 4) return;
        bool w = false;
        sb.okv[i] = planners[i]->prepareFitPointsWith(sb.seed[i], sb.fitPts[i], 0.0, sb.prevFitOut[i], w) ? 1 : 0;
        sb.wroteFit[i] = w ? 1 : 0;
    });
    std::vector<bool> ready(n, false);
    for (size_t i = 0; i < n; ++i) {
        if (startEndConditions[i].size() == 4 && sb.wroteFit[i] && prev > planners[i]->maxPathLength_) {
            bool w = false;
            sb.okv[i] = planners[i]->prepareFitPointsWith(sb.seed[i], sb.fitPts[i], prev, sb.prevFitOut[i], w) ? 1 : 0;
            redone[i] = 1;
        }
        if (sb.wroteFit[i]) prev = sb.prevFitOut[i];
        ready[i] = startEndConditions[i].size() == 4 && sb.okv[i] && sb.fitPts[i].size() > 3;
        if (sb.onDevice[i] && !redone[i]) {
            if (sb.okv[i]) planners[i]->clear();             // prepareFitPointsWith's clear() (BT.cpp:308), for the launch's own
            ++st.seedDecided;
        } else {
            ++st.seedHost;
        }
    }
    g_prevPathLength.store(prev);
    // the planners the launch decided and vigo_bspline_fit_mixed fitted behind it: their control points are down already;
    // a redone planner's were made of points the host has replaced and are dropped
    std::vector<size_t> fitted;
    for (size_t i = 0; i < n; ++i)
        if (ready[i] && sb.onDevice[i] && !redone[i] && sb.devCtrl[i].size() == (sb.fitPts[i].size() + 2) * 3) {
            fitted.push_back(i);
            ready[i] = false;
            ok[i] = true;
        }
    parallelFor(fitted.size(), [&](size_t k) {
        const size_t i = fitted[k];
        Eigen::MatrixXd controlPoints;
        controlPoints.resize(3, (long)sb.fitPts[i].size() + 2);
        std::memcpy(controlPoints.data(), sb.devCtrl[i].data(), sizeof(double) * sb.devCtrl[i].size());
        planners[i]->installControlPoints(controlPoints, sb.fitPts[i]);
    });
    fitGroups(planners, sb.fitPts, ready, startEndConditions, ok, sb.o.mixedFit);
    if (seeds) *seeds = sb.seed;
    if (info) *info = sb.info;
    reportBatchStats(st, stats);
    return ok;
}

}  // namespace trajPlanner
