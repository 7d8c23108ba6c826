// vigo_solver_plan.hpp — which k_optimize instantiations one vigo_optimize call launches, with what grid and how much LDS:
// the ONE statement of that rule.  Plain host C++17, nothing of HIP: vigo_solver.hip executes the plan, vigo_api.cpp asks it
// whether a shape fits, tests/test_solver_plan.py holds it against an independent restatement on a machine without a GPU.
#pragma once
#include <stddef.h>

#include "../../include/vigo.h"

namespace vigo {

constexpr int kWave = 64;
constexpr size_t kLdsPerWorkgroup = 160 * 1024;   // the LDS of a CU: the most one workgroup can ask for
constexpr size_t kLdsStaticLimit = 64 * 1024;     // dynamic LDS a kernel may be launched with before its limit is raised
constexpr int kMaxMem = VIGO_MAX_MEM_SIZE;
// Dynamic-obstacle table of the solve kernel: per trajectory, {predicted x, predicted y, threshold}
// of up to kObsTabEntries (obstacle, predicted step) pairs plus the obstacles' sizes, staged in LDS
// once per solve (they do not depend on the control points).  Sized so that the N = 32 and N = 64
// shapes keep four waves per CU (<= 40 KiB per wave, history slots with their zero column included):
// 8 obstacles x 11 predicted steps for two trajectories per wave, 3 x 11 for one.
constexpr int kObsTabObs = 16;
template <int GROUP> constexpr int kObsTabEntries = GROUP == 32 ? 88 : 33;
template <int GROUP> constexpr int kObsTabDoubles = 3 * kObsTabEntries<GROUP> + kObsTabObs;
// History pairs besides the newest that the level kernel keeps in registers on batches with more waves than SIMDs
// (1 = as everywhere), where LDS decides how many waves a CU holds.  N <= 32 (two trajectories per wave): 4 pairs,
// 24.4 -> 19.3 KB, six -> EIGHT waves per CU (256 VGPRs, no spills): 1.74 -> 1.47 ms at 16 384 x 32 (2 pairs: 1.60,
// 3: 1.61, 5: 1.54).  32 < N <= 64 (one per wave): 5 pairs, 26.8 -> 19.2 KB, six -> eight: 1.85 -> 1.54 ms at 8192 x 64
// (4 pairs, seven waves: 1.71; 6 pairs: 1.57).  Same arithmetic, same bits.
constexpr int kLevelRH = 4, kLevelRH64 = 5;
// (GROUP, PPL) for N control points: a trajectory owns GROUP lanes, a lane PPL consecutive control points.
// 32 x 1 up to 32, then 64 x {1, 2, 4}.
// (N <= 32 as 64 x 1 — one control point per lane, half the lanes idle, a sixth butterfly level in every reduction and
// no instruction saved — measured slower: 0.462 vs 0.445 ms at B = 1024, 6.40 vs 3.60 ms at B = 16384.  A 16-lane x
// 2-point shape saves one butterfly level but measured 22 % slower: 1.76 M vs 2.26 M/s.)
struct Shape { int group, ppl; };
constexpr Shape shape_for(int N) { return N <= 32 ? Shape{32, 1} : Shape{64, N <= 64 ? 1 : (N <= 128 ? 2 : 4)}; }
constexpr int default_rh(int ppl) { return ppl == 1 ? 1 : 0; }   // k_optimize's RH unless told otherwise
// sizeof(T), sizeof(HPair<T, D>) and sizeof(YSv<FAST>) of vigo_solver.hip (which asserts them against the types)
constexpr size_t elem_bytes_of(int precision) { return precision == VIGO_PREC_F32 ? 4 : 8; }
constexpr size_t hpair_bytes(size_t elem_bytes, int D) { return (2 * D * elem_bytes + 15) & ~(size_t)15; }
constexpr size_t ysv_bytes(bool fast) { return fast ? 8 : 16; }

// dynamic LDS of one k_optimize workgroup of elem_bytes-wide state (4: fp32, 8: fp64)
constexpr size_t optimize_lds_bytes(size_t elem_bytes, int group, bool fast, int D, int N, int m, int ppl, bool with_obstacles, int rh) {
    const int TPB = D == 1 ? 1 : kWave / group;   // D == 1, the axis-per-lane layout: one trajectory per wave ...
    const int COLS = kWave / group;               // ... and a 16-byte record per free control point and AXIS
    const int ms = ppl == 1 ? (m > rh + 1 ? m - (rh + 1) : 0) : m;   // REG1: ages 0 .. rh live in registers
    // per slot: one record per free control point + the zero column, then {ys, 1/ys} per trajectory (see k_optimize)
    const size_t slot = ((size_t)COLS * (N - 6) + 1) * hpair_bytes(elem_bytes, D) + (((size_t)TPB * ysv_bytes(fast) + 15) & ~(size_t)15);
    size_t h = (size_t)ms * slot;
    h += (size_t)m * TPB * sizeof(double);        // the alphas of the general two-loop
    if (with_obstacles) h += (size_t)TPB * (group == 32 ? kObsTabDoubles<32> : kObsTabDoubles<64>) * sizeof(double);
    return h;
}

// bytes of LDS one trajectory-solve workgroup needs at most (the general kernel with its obstacle table); the C ABI
// refuses N it cannot hold
constexpr size_t optimize_lds_requirement(int N, int mem_size, int precision) {
    const Shape sh = shape_for(N);
    return optimize_lds_bytes(elem_bytes_of(precision), sh.group, precision == VIGO_PREC_F64_FAST, 3, N, mem_size, sh.ppl, true, default_rh(sh.ppl));
}

// k_optimize<T, GROUP, PPL, FAST, WPS, OBS, D, RH>, (T, FAST) = (float, false) | (double, false) | (double, true) for
// VIGO_PREC_F32 | _F64 | _F64_FAST.  A key's index is its bit in the per-device "LDS limit raised" mask and its row in the
// kernel table that vigo_solver.hip expands from this list: part 0 of that file the rows without OBS, part 1 those with,
// and the order of the rows is the order of the kernels in the code objects.  Per arithmetic and
// shape: the general kernel (D = 3), with a two-waves-per-SIMD build where a lane owns one point; without
// OBS, before it, the level kernels (D = 2) of 32 x 1 and 64 x 1: the one with kLevelRH / kLevelRH64 register-held pairs
// (fp64 only; more than four waves per CU put two on a SIMD: the register-capped build, 256 VGPRs) and the plain ones;
// fp64 reference order, 32 x 1: the axis-per-lane kernel (D = 1) first.
struct OptimizeKey { int precision, group, ppl, wps; bool obs; int d, rh; };
constexpr int kF32 = VIGO_PREC_F32, kFast = VIGO_PREC_F64_FAST, kF64 = VIGO_PREC_F64;
constexpr OptimizeKey kOptimizeKeys[] = {
    {kF32, 32, 1, 2, false, 2, 1}, {kF32, 32, 1, 1, false, 2, 1}, {kF32, 32, 1, 2, false, 3, 1}, {kF32, 32, 1, 1, false, 3, 1},
    {kF32, 64, 1, 2, false, 2, 1}, {kF32, 64, 1, 1, false, 2, 1}, {kF32, 64, 1, 2, false, 3, 1}, {kF32, 64, 1, 1, false, 3, 1},
    {kF32, 64, 2, 1, false, 3, 0}, {kF32, 64, 4, 1, false, 3, 0},
    {kFast, 32, 1, 2, false, 2, kLevelRH}, {kFast, 32, 1, 2, false, 2, 1}, {kFast, 32, 1, 1, false, 2, 1}, {kFast, 32, 1, 2, false, 3, 1}, {kFast, 32, 1, 1, false, 3, 1},
    {kFast, 64, 1, 2, false, 2, kLevelRH64}, {kFast, 64, 1, 2, false, 2, 1}, {kFast, 64, 1, 1, false, 2, 1}, {kFast, 64, 1, 2, false, 3, 1}, {kFast, 64, 1, 1, false, 3, 1},
    {kFast, 64, 2, 1, false, 3, 0}, {kFast, 64, 4, 1, false, 3, 0},
    {kF64, 32, 1, 1, false, 1, 1},
    {kF64, 32, 1, 2, false, 2, kLevelRH}, {kF64, 32, 1, 2, false, 2, 1}, {kF64, 32, 1, 1, false, 2, 1}, {kF64, 32, 1, 2, false, 3, 1}, {kF64, 32, 1, 1, false, 3, 1},
    {kF64, 64, 1, 2, false, 2, kLevelRH64}, {kF64, 64, 1, 2, false, 2, 1}, {kF64, 64, 1, 1, false, 2, 1}, {kF64, 64, 1, 2, false, 3, 1}, {kF64, 64, 1, 1, false, 3, 1},
    {kF64, 64, 2, 1, false, 3, 0}, {kF64, 64, 4, 1, false, 3, 0},
    {kF32, 32, 1, 2, true, 3, 1}, {kF32, 32, 1, 1, true, 3, 1}, {kF32, 64, 1, 2, true, 3, 1}, {kF32, 64, 1, 1, true, 3, 1},
    {kF32, 64, 2, 1, true, 3, 0}, {kF32, 64, 4, 1, true, 3, 0},
    {kFast, 32, 1, 2, true, 3, 1}, {kFast, 32, 1, 1, true, 3, 1}, {kFast, 64, 1, 2, true, 3, 1}, {kFast, 64, 1, 1, true, 3, 1},
    {kFast, 64, 2, 1, true, 3, 0}, {kFast, 64, 4, 1, true, 3, 0},
    {kF64, 32, 1, 2, true, 3, 1}, {kF64, 32, 1, 1, true, 3, 1}, {kF64, 64, 1, 2, true, 3, 1}, {kF64, 64, 1, 1, true, 3, 1},
    {kF64, 64, 2, 1, true, 3, 0}, {kF64, 64, 4, 1, true, 3, 0},
};
constexpr int kOptimizeKeyCount = sizeof(kOptimizeKeys) / sizeof(kOptimizeKeys[0]);
constexpr int optimize_key_index(const OptimizeKey& k) {   // -1: no such instantiation
    for (int i = 0; i < kOptimizeKeyCount; ++i) {
        const OptimizeKey& c = kOptimizeKeys[i];
        if (c.precision == k.precision && c.group == k.group && c.ppl == k.ppl && c.wps == k.wps && c.obs == k.obs && c.d == k.d && c.rh == k.rh) return i;
    }
    return -1;
}

// a launch: the index into kOptimizeKeys, workgroups (of one wave), dynamic LDS bytes, its SolveArgs::level_waves_elsewhere
struct PlannedLaunch { int key, grid; size_t lds; int level_waves_elsewhere; };
// count launches, in order; -1: the shape does not fit the LDS
struct OptimizePlan { int count; PlannedLaunch launch[2]; };

// The launches of one vigo_optimize call of B > 0 trajectories of N control points.  simd_count: 4 per CU, 0 = unknown;
// allow_axis: false keeps the axis-per-lane kernel out of the plan (a switch of development builds).
inline OptimizePlan plan_optimize(int N, int B, int precision, bool has_obstacle_list, bool plan_in_z, bool strict_z, int mem_size, int simd_count, bool allow_axis) {
    const Shape sh = shape_for(N);
    const size_t eb = elem_bytes_of(precision);
    const bool fast = precision == VIGO_PREC_F64_FAST, f64 = precision == VIGO_PREC_F64;
    // Measured (tools/exp_solver.py, VIGO_EXP_MATRIX=1: N = 16 ... 200 x the three arithmetic modes): the instantiation
    // without obstacle code is 4 - 18 % faster everywhere except f64_fast at 32 < N <= 64 on batches with more
    // trajectories than SIMDs (8 % slower there): those keep the obstacle instantiation, which treats a missing list as
    // no obstacles.  (Only where the level instantiation cannot apply — z planning on: with it, level waves go to the
    // D = 2 kernel, 20 % faster than either, and the corner is not worth keeping them from it.)
    const bool obs = has_obstacle_list || (fast && N > 32 && N <= 64 && simd_count > 0 && B > simd_count && (plan_in_z || strict_z));
    const int grid = (B + kWave / sh.group - 1) / (kWave / sh.group);
    // a solver wavefront per SIMD (4 per CU) is full occupancy for these kernels: only a grid with more waves than SIMDs
    // takes a two-waves-per-SIMD build, and only where eight waves' LDS fit a CU; unknown SIMD count: never
    const bool crowded = grid > (simd_count > 0 ? simd_count : (1 << 30));
    auto lds_of = [&](int D, bool table, int rh) { return optimize_lds_bytes(eb, sh.group, fast, D, N, mem_size, sh.ppl, table, rh); };
    auto wps_for = [&](size_t lds) { return sh.ppl == 1 && crowded && lds <= kLdsPerWorkgroup / 8 ? 2 : 1; };
    OptimizePlan p{};
    auto add = [&](int wps, int D, int rh, int g, size_t lds, int lwe) {
        const int key = optimize_key_index(OptimizeKey{precision, sh.group, sh.ppl, wps, obs, D, rh});
        if (key < 0 || p.count < 0) p.count = -1;
        else p.launch[p.count++] = PlannedLaunch{key, g, lds, lwe};
    };
    // the general launch sizes its LDS by the list that is there, not by the instantiation (the redirect has no table)
    const size_t lds = lds_of(3, has_obstacle_list, default_rh(sh.ppl));
    if (lds > kLdsPerWorkgroup) return OptimizePlan{-1, {}};   // refused earlier by vigo_optimize
    // Calls that can hold level trajectories (no z planning) and have an instantiation for them (one point per lane, no
    // obstacles) are two launches: FIRST the level kernel, whose waves with a trajectory that is not level exit at once,
    // THEN the general kernel, whose waves of level trajectories do (after the axis-per-lane launch: whose GROUPS of a
    // level trajectory do).  The order matters: each launch decides from the control points it finds; a level
    // trajectory's z is untouched by the first launch, so the second still sees it level and skips it — the other way
    // round, a trajectory just outside the band that the general solve smooths into it would be solved a second time.
    int lwe = 0;
    if (sh.ppl == 1 && !obs && !plan_in_z && !strict_z) {
        lwe = 1;
        const int rh = sh.group == 32 ? kLevelRH : kLevelRH64;
        const size_t lds2 = lds_of(2, false, 1), lds3 = lds_of(2, false, rh);
        if (f64 && sh.group == 32 && simd_count > 0 && B <= simd_count && allow_axis) {
            // fp64 reference order, N <= 32, a batch with at most one trajectory per SIMD (two per wave leave half the
            // chip idle): the axis-per-lane instantiation, ONE trajectory per wave, solves every level trajectory of
            // the batch; the general kernel then skips them one by one (level_waves_elsewhere == 2).  Its LDS
            // (<= 12.2 KB) is below the static limit.
            add(1, 1, 1, B, lds_of(1, false, 1), lwe);
            lwe = 2;
        } else if (precision != VIGO_PREC_F32 && crowded && lds2 > kLdsPerWorkgroup / 8 && kLdsPerWorkgroup / lds3 > kLdsPerWorkgroup / lds2) {
            // fp64, more waves than SIMDs: keep rh pairs besides the newest in registers when that buys a further
            // resident wave per CU (N = 32, m = 16: 24.4 -> 22.7 KB, six -> seven)
            add(2, 2, rh, grid, lds3, lwe);
        } else {
            add(wps_for(lds2), 2, 1, grid, lds2, lwe);
        }
    }
    add(wps_for(lds), 3, default_rh(sh.ppl), grid, lds, lwe);
    return p;
}

// ---- the two launches of a small batch as one (k_optimize_fused) --------------------------------------------------
// A plan whose FIRST launch is the axis-per-lane kernel (D = 1; then the second is the general kernel of 32 x 1 with
// level_waves_elsewhere == 2, and B <= simd_count) runs as ONE launch of k_optimize_fused: B one-wave workgroups, each
// classifies its trajectory once and runs the axis body on a level one, the general body on any other, alone on lanes
// 0 .. 31.  Every other plan runs as planned.  A rule over the plan: plan_optimize, kOptimizeKeys and the bits of the
// "LDS limit raised" mask stay as they are; the fused kernel is no row of a table (one instantiation, vigo_solver.hip).
// LDS of the general body on ONE trajectory of N <= 32 control points, fp64 reference order, no obstacle table: per
// history slot in LDS (m - 2 of them) one 48-byte record per free control point plus the zero column and {ys, 1/ys},
// then m alphas — 14 x (27 x 48 + 16) + 128 = 18 496 B at N = 32, m = 16.
constexpr size_t solo_lds_bytes(int N, int m) {
    const int ms = m > 2 ? m - 2 : 0;
    return (size_t)ms * (((size_t)(N - 6) + 1) * hpair_bytes(8, 3) + ysv_bytes(false)) + (size_t)m * sizeof(double);
}
// fuse: the plan's launches run as one; grid workgroups of one wave with lds bytes, the larger of the two bodies' layouts
// (at most kLdsPerWorkgroup / 8 for every N <= 32 and mem_size <= kMaxMem: two batches in flight keep two waves on a SIMD)
struct FusedLaunch { bool fuse; int grid; size_t lds; };
inline FusedLaunch fuse_optimize(const OptimizePlan& p, int N, int mem_size) {
    if (p.count != 2 || kOptimizeKeys[p.launch[0].key].d != 1) return FusedLaunch{false, 0, 0};
    const size_t axis = p.launch[0].lds, solo = solo_lds_bytes(N, mem_size);
    return FusedLaunch{true, p.launch[0].grid, axis > solo ? axis : solo};
}

// ---- mixed control-point counts (vigo_*_mixed) --------------------------------------------------------------------
// k_optimize<.., MIXED = true>: trajectories of different counts in one launch, rows strided by Ns.  Only the general
// kernel (D = 3, OBS) is built that way — it treats a missing obstacle list as no obstacles and solves a level trajectory
// with its z terms masked, the same bits as the level / no-obstacle kernels — for the two shapes with one point per lane.
// A list of its own: kOptimizeKeys, its order and the bits of the "LDS limit raised" mask stay as they are; the index of a
// key here is its row in the mixed kernel table of vigo_solver.hip (part 2 of that file).
constexpr int kMixedMaxStride = 64;
constexpr OptimizeKey kOptimizeMixedKeys[] = {
    {kF32, 32, 1, 2, true, 3, 1}, {kF32, 32, 1, 1, true, 3, 1}, {kF32, 64, 1, 2, true, 3, 1}, {kF32, 64, 1, 1, true, 3, 1},
    {kFast, 32, 1, 2, true, 3, 1}, {kFast, 32, 1, 1, true, 3, 1}, {kFast, 64, 1, 2, true, 3, 1}, {kFast, 64, 1, 1, true, 3, 1},
    {kF64, 32, 1, 2, true, 3, 1}, {kF64, 32, 1, 1, true, 3, 1}, {kF64, 64, 1, 2, true, 3, 1}, {kF64, 64, 1, 1, true, 3, 1},
};
constexpr int kOptimizeMixedKeyCount = sizeof(kOptimizeMixedKeys) / sizeof(kOptimizeMixedKeys[0]);
constexpr int optimize_mixed_key_index(int precision, int group, int wps) {   // -1: no such instantiation
    for (int i = 0; i < kOptimizeMixedKeyCount; ++i) {
        const OptimizeKey& c = kOptimizeMixedKeys[i];
        if (c.precision == precision && c.group == group && c.wps == wps) return i;
    }
    return -1;
}
// every count of a mixed call lies in the shape class of its stride: all <= 32, or all in 33 .. 64
constexpr bool mixed_count_ok(int n, int Ns) { return n >= 7 && n <= Ns && Ns <= kMixedMaxStride && shape_for(n).group == shape_for(Ns).group; }

// The ONE launch of a vigo_optimize_mixed call of B > 0 trajectories in rows of Ns control points (key: the index into
// kOptimizeMixedKeys); count -1: Ns outside [7, 64].  The LDS is sized by Ns and always holds the obstacle table, with a
// list or without (has_obstacle_list does not enter: one kernel per (Ns, B, precision, mem_size), whatever the lists): at
// most 40.9 KB, below the static limit, so no instantiation needs its limit raised.
inline OptimizePlan plan_optimize_mixed(int Ns, int B, int precision, bool /*has_obstacle_list*/, int mem_size, int simd_count) {
    if (Ns < 7 || Ns > kMixedMaxStride) return OptimizePlan{-1, {}};
    const Shape sh = shape_for(Ns);
    const int grid = (B + kWave / sh.group - 1) / (kWave / sh.group);
    const bool crowded = grid > (simd_count > 0 ? simd_count : (1 << 30));
    const size_t lds = optimize_lds_bytes(elem_bytes_of(precision), sh.group, precision == VIGO_PREC_F64_FAST, 3, Ns, mem_size, 1, true, 1);
    const int key = optimize_mixed_key_index(precision, sh.group, crowded && lds <= kLdsPerWorkgroup / 8 ? 2 : 1);
    if (key < 0 || lds > kLdsStaticLimit) return OptimizePlan{-1, {}};
    return OptimizePlan{1, {PlannedLaunch{key, grid, lds, 0}, {}}};
}

}  // namespace vigo
