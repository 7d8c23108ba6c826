// vigo_solver.hip — batched ViGO cost/gradient and the whole-solve L-BFGS kernel for gfx950.
//
// Mapping (MI355X-first, no MFMA: there is no dense contraction on this path):
//   * one 64-lane wavefront per workgroup; a trajectory owns a lane GROUP of 32 (N <= 32, two
//     trajectories per wave) or 64 lanes; a lane owns PPL consecutive control points (1 for
//     N <= 64, 2 for N <= 128, 4 beyond), so the 4-point jerk stencil and the 2/3-point vel/acc
//     stencils are register renames plus DPP wave shifts (no LDS).
//   * x, g, xp, gp, d live in VGPRs (3 scalars per owned point each); the L-BFGS history
//     (m x {s,y}) lives in LDS, one 48-byte record per free control point and slot: HBM sees the
//     initial control points and the result only.
//   * every scalar of the More-Thuente search is replicated across the group's lanes; the two
//     groups of a wave diverge freely (exec masking), all cross-lane traffic stays inside a group.
//   * a trajectory whose control points all lie at one height (and no z planning) cannot move in z by more than
//     rounding noise: the LEVEL RULE (include/vigo.h) holds its z fixed, and waves of such trajectories run the
//     D = 2 instantiation of the solve kernel, which carries x and y only — 2/3 of the history, dots and stencils.
//     On fp64 reference-order batches of at most one trajectory per SIMD (N <= 32) every level trajectory gets a wave
//     of its own instead, one COORDINATE per lane (the D = 1 instantiation, "AXIS" below): twice the waves on a chip
//     that was half idle, every loop-carried vector one double per lane.
//   * per-trajectory sums (cost terms, dot products) are: a per-point partial, the lane's
//     points added in index order, then a butterfly all-reduce inside the group,
//     v += lane[i ^ m], m = 1,2,..,GROUP/2 — a fixed tree, so results are deterministic and
//     reproducible bit-for-bit by oracle/vigo_oracle.c's emulation mode.
//
// Arithmetic follows the reference expression by expression (bsplineTraj.cpp:802-1064 and
// solver/lbfgs.hpp:295-1349; see the citations on each block); the file is built with
// -ffp-contract=off so no FMA contraction changes a rounding.  Differences to the CPU
// reference are confined to: summation order of the reductions above, x*x / x*x*x instead
// of glibc pow(x,2|3), sqrt instead of pow(.,0.5).
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "vigo_exact_div.hpp"
#include "vigo_internal.hpp"
#include "vigo_linesearch.hpp"
#include "vigo_solver_plan.hpp"

// dev switches of the axis kernel's two short forms (vigo_exact_div.hpp; profiles/README.md, round 7): the stencil's
// divisions by ts_ctrl as Markstein's sequence, the convergence test behind the squared-norm filter
#ifndef VIGO_AXIS_TS_MARK
#define VIGO_AXIS_TS_MARK 1
#endif
#ifndef VIGO_AXIS_CONV_FILTER
#define VIGO_AXIS_CONV_FILTER 1
#endif
// dev switches of the axis kernel's paired reductions (pair_tree32 below; profiles/README.md, round 8): two sums in one
// 32-lane tree, one per half of the wave, in the evaluation's six sums and in the update's ys and yy
#ifndef VIGO_AXIS_PAIR_EVAL
#define VIGO_AXIS_PAIR_EVAL 1
#endif
#ifndef VIGO_AXIS_PAIR_UPDATE
#define VIGO_AXIS_PAIR_UPDATE 1
#endif
// dev switches of the axis kernel's line search (vigo_linesearch.hpp; profiles/README.md, round 9).  Any of them takes the
// axis kernel's search from the header, with a trial's set-up at the end of the trial before it, so that the first trial's
// set-up is text of its own in which brackt = 0 and xt = 0 are constants: FIRST_SETUP = 2, the shipped setting (+1.0 %).
// Measured and rejected, both off: FIRST_TESTS, the exit tests of a search's first trial behind a wave-uniform branch,
// without the bracket's (no gain of its own on top of the moved set-up, and one SGPR spill); FIRST_SETUP = 1, the bracket
// state formed only once that trial is rejected (the copies it puts on every later trial cost more than it saves).
#ifndef VIGO_AXIS_LS_FIRST_TESTS
#define VIGO_AXIS_LS_FIRST_TESTS 0
#endif
#ifndef VIGO_AXIS_LS_FIRST_SETUP
#define VIGO_AXIS_LS_FIRST_SETUP 2
#endif

namespace vigo {
namespace {

// ---- cross-lane primitives -----------------------------------------------------------

// DPP wave shifts (GFX9 family): lane i receives lane i-1 (wave_shr:1) / i+1 (wave_shl:1).
// Lane 0 (63) has no source and keeps an unspecified value: every consumer of a shifted value
// is guarded by the control-point index, so the wave edges (and the seam between the two
// 32-lane groups) are never read.
__device__ __forceinline__ int dpp_prev_i32(int v) {
    return __builtin_amdgcn_mov_dpp(v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ int dpp_next_i32(int v) {
    return __builtin_amdgcn_mov_dpp(v, 0x130, 0xF, 0xF, false);
}
__device__ __forceinline__ double from_prev(double v) {
    return __hiloint2double(dpp_prev_i32(__double2hiint(v)), dpp_prev_i32(__double2loint(v)));
}
__device__ __forceinline__ double from_next(double v) {
    return __hiloint2double(dpp_next_i32(__double2hiint(v)), dpp_next_i32(__double2loint(v)));
}
__device__ __forceinline__ float from_prev(float v) {
    return __int_as_float(dpp_prev_i32(__float_as_int(v)));
}
__device__ __forceinline__ float from_next(float v) {
    return __int_as_float(dpp_next_i32(__float_as_int(v)));
}

// Shift of a per-lane run of PPL consecutive control-point values by one point along the
// trajectory: o[q] = value of point (own + q + 1) resp. (own + q - 1).  Inside the lane that is
// a register rename, across lanes one DPP shift.
template <typename T, int PPL>
__device__ __forceinline__ void seq_next(const T (&a)[PPL], T (&o)[PPL]) {
    const T edge = from_next(a[0]);
#pragma unroll
    for (int q = 0; q + 1 < PPL; ++q) o[q] = a[q + 1];
    o[PPL - 1] = edge;
}
template <typename T, int PPL>
__device__ __forceinline__ void seq_prev(const T (&a)[PPL], T (&o)[PPL]) {
    const T edge = from_prev(a[PPL - 1]);
#pragma unroll
    for (int q = PPL - 1; q > 0; --q) o[q] = a[q - 1];
    o[0] = edge;
}

// Butterfly all-reduce of K independent values inside a GROUP-lane group, as VALU-speed DPP
// moves instead of ds_bpermute round trips.  The tree is the xor butterfly
// v += lane[i ^ m], m = 1, 2, 4, ..., GROUP/2:
//   m = 1, 2   quad_perm [1,0,3,2] / [2,3,0,1]
//   m = 4, 8   row_half_mirror / row_mirror: after the quad steps every lane of a quad holds the
//              quad sum, so pairing lane i with 7-i (15-i) adds the same two partial sums as
//              pairing it with i^4 (i^8) — identical bits, fp add being commutative;
//   m = 16     v_permlane16_swap (gfx950): rows 0/1 and 2/3 exchange, sum = even row + odd row;
//   m = 32     v_permlane32_swap: the two 32-lane halves exchange.
// All partners stay inside the group, so an exec-masked sibling group never contributes.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    // every source lane of these patterns lies in the reader's own row: no `old` value needed
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// The xor-16 level needs the value twice (v_permlane16_swap exchanges rows between TWO registers and clobbers
// both).  Instead of copying the result of the row_mirror level (two v_mov_b32), that level's add is issued twice:
// one VALU slot instead of two.  The second add is an asm statement so that it is not merged with the first (the
// compiler still sees its register definition and keeps the VALU-write -> permlane-read wait states after it).
__device__ __forceinline__ double add_f64_again(double a, double b) {
    double r;
    asm volatile("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (a == b bitwise, in two registers; the two halves of the result are returned so that a 64-lane group can issue the
// final add twice as well, for its xor-32 level)
__device__ __forceinline__ void xor16_parts(double a, double b, double& p0, double& p1) {
    const int alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
    auto l = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
    auto h = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
    p0 = __hiloint2double(h[0], l[0]);
    p1 = __hiloint2double(h[1], l[1]);
}
__device__ __forceinline__ double xor32_sum2(double a, double b) {
    const int alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
    auto l = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    auto h = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    return __hiloint2double(h[0], l[0]) + __hiloint2double(h[1], l[1]);
}
// AXIS layout (k_optimize with D == 1): lane l < 32 holds coordinate 0 of control point l, lane l + 32 coordinate 1
// of the same point.  v_permlane32_swap of a value with a copy of itself hands EVERY lane both: x = what the lower
// half holds, y = what the upper half holds, so x + y is the same add, operands in the same order, in both lanes.
__device__ __forceinline__ void xy_parts(double a, double b, double& x, double& y) {   // a == b bitwise, in two registers
    const int alo = __double2loint(a), ahi = __double2hiint(a), blo = __double2loint(b), bhi = __double2hiint(b);
    auto l = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
    auto h = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
    x = __hiloint2double(h[0], l[0]);
    y = __hiloint2double(h[1], l[1]);
}
__device__ __forceinline__ void xy_both(double v, double& x, double& y) { xy_parts(v, v, x, y); }
__device__ __forceinline__ double mul_f64_again(double a, double b) {   // as add_f64_again: the copy the swap needs
    double r;
    asm volatile("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a0 * b0 + a1 * b1 of a point whose two coordinates sit on lanes l and l + 32: dot3<false, T, 2> across the pair
__device__ __forceinline__ double dot_xy(double a, double b) { return xor32_sum2(a * b, mul_f64_again(a, b)); }

template <int GROUP, int K>
__device__ __forceinline__ void group_sum(double (&v)[K]) {
    static_assert(GROUP == 16 || GROUP == 32 || GROUP == 64, "group is a DPP row, half a wave or a wave");
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0xB1>(v[q]);   // quad_perm:[1,0,3,2]
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0x4E>(v[q]);   // quad_perm:[2,3,0,1]
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0x141>(v[q]);  // row_half_mirror
    if (GROUP >= 32) {
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const double t = dpp_f64<0x140>(v[q]);             // row_mirror
            const double a = v[q] + t;
            const double b = add_f64_again(v[q], t);
            double p0, p1;
            xor16_parts(a, b, p0, p1);
            if (GROUP == 64) v[q] = xor32_sum2(p0 + p1, add_f64_again(p0, p1));
            else v[q] = p0 + p1;
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0x140>(v[q]);  // row_mirror
}
template <int GROUP>
__device__ __forceinline__ double group_sum1(double v) {
    double a[1] = {v};
    group_sum<GROUP, 1>(a);
    return a[0];
}

// AXIS layout: TWO sums in one 32-lane tree.  There the xor-32 exchange of a dot product comes BEFORE the tree, so lanes
// l and l + 32 enter group_sum<32, K> with the same partial and the two halves of the wave run the same tree on the same
// operands — every tree twice.  Here the lower half carries the partials of sum A and the upper half those of sum B:
// v[q] = [A partial of point l | B partial of point l].  The five levels are those of group_sum<32, K>, control for
// control: the quad_perm and mirror patterns read inside the reader's own 16-lane row, v_permlane16_swap exchanges rows
// 0/1 and rows 2/3, and a half is rows 0-1 or rows 2-3 — so no lane reads a lane of the other half and each half runs
// exactly the tree it runs in group_sum, on the operands it has there: the same bits.  Only then the xor-32 exchange
// (xy_parts, on the twice-issued last add) hands every lane both totals: a[q] = what the lower half holds, b[q] = the upper.
template <int K>
__device__ __forceinline__ void pair_tree32(double (&v)[K], double (&a)[K], double (&b)[K]) {
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0xB1>(v[q]);   // quad_perm:[1,0,3,2]
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0x4E>(v[q]);   // quad_perm:[2,3,0,1]
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] += dpp_f64<0x141>(v[q]);  // row_half_mirror
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const double t = dpp_f64<0x140>(v[q]);                 // row_mirror
        double p0, p1;
        xor16_parts(v[q] + t, add_f64_again(v[q], t), p0, p1);
        xy_parts(p0 + p1, add_f64_again(p0, p1), a[q], b[q]);
    }
}
// The packed partials of two dot products of the AXIS layout, from the per-lane products u (sum A) and w (sum B) of a
// lane's coordinate: v_permlane32_swap gives [u of x | w of x] and [u of y | w of y], and their sum is
// [u_x + u_y | w_x + w_y] — in each half the add dot_xy() does, operands in the same order, for the sum that half carries.
__device__ __forceinline__ double pack_xy(double u, double w) {
    const int ulo = __double2loint(u), uhi = __double2hiint(u), wlo = __double2loint(w), whi = __double2hiint(w);
    auto l = __builtin_amdgcn_permlane32_swap(ulo, wlo, false, false);
    auto h = __builtin_amdgcn_permlane32_swap(uhi, whi, false, false);
    return __hiloint2double(h[0], l[0]) + __hiloint2double(h[1], l[1]);
}
// ys = y . s and yy = y . y of the update (LB:1264-1276) in the AXIS layout as one pair, y and s the lane's coordinate:
// what dot_lane<.., 1>, the + 0.0 of the level trajectory's z product and group_sum<32, 2> compute, ys in the lower half
// and yy in the upper.  The + 0.0 follows the exchange add, as it does there, and is applied to both halves: yy's
// partial is a sum of two squares, +0 or above or NaN, never -0, and x + 0.0 is x for every such x.
__device__ __forceinline__ void ys_yy_axis(double y, double s, double& ys, double& yy) {
    double v[1] = {pack_xy(y * s, y * y) + 0.0}, a[1], b[1];
    pair_tree32<1>(v, a, b);
    ys = a[0];
    yy = b[0];
}

// min and max of a value over the lanes of a group (the same xor butterfly; order is irrelevant for min / max)
template <int GROUP>
__device__ __forceinline__ void group_minmax(double& mn, double& mx) {
    static_assert(GROUP == 32 || GROUP == 64, "half a wave or a wave");
    auto step = [&](double omn, double omx) { mn = fmin(mn, omn); mx = fmax(mx, omx); };
    step(dpp_f64<0xB1>(mn), dpp_f64<0xB1>(mx));
    step(dpp_f64<0x4E>(mn), dpp_f64<0x4E>(mx));
    step(dpp_f64<0x141>(mn), dpp_f64<0x141>(mx));
    step(dpp_f64<0x140>(mn), dpp_f64<0x140>(mx));
    {
        double a0, a1, b0, b1;
        xor16_parts(mn, mn, a0, a1);
        xor16_parts(mx, mx, b0, b1);
        mn = fmin(a0, a1);
        mx = fmax(b0, b1);
    }
    if (GROUP == 64) {
        const int nlo = __double2loint(mn), nhi = __double2hiint(mn), xlo = __double2loint(mx), xhi = __double2hiint(mx);
        auto l = __builtin_amdgcn_permlane32_swap(nlo, nlo, false, false);
        auto h = __builtin_amdgcn_permlane32_swap(nhi, nhi, false, false);
        mn = fmin(__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1]));
        auto l2 = __builtin_amdgcn_permlane32_swap(xlo, xlo, false, false);
        auto h2 = __builtin_amdgcn_permlane32_swap(xhi, xhi, false, false);
        mx = fmax(__hiloint2double(h2[0], l2[0]), __hiloint2double(h2[1], l2[1]));
    }
}

__device__ __forceinline__ double sum3(double a, double b, double c) { return (a + b) + c; }

// FAST (VIGO_PREC_F64_FAST): explicit fused multiply-adds in the dot products, axpys, stencils
// and the weight combination — what GCC's default -ffp-contract=fast does to the reference on
// its ARM targets — plus one reciprocal per history pair instead of a division per two-loop
// step.  Every fma below is mirrored by oracle/vigo_oracle.c's fast emulation, bit for bit.
__device__ __forceinline__ double fmaT(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fmaT(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// D = the number of leading coordinates that MOVE: 3, or 2 for a level trajectory (see k_optimize): the z components of
// g, d, s, y are then exactly zero, their products contribute +-0 to every sum and are left out
template <bool FAST, typename T, int D = 3>
__device__ __forceinline__ double dot3(const T (&a)[3], const T (&b)[3]) {
    if (D == 2) {
        if (FAST) return fmaT((double)a[1], (double)b[1], (double)a[0] * (double)b[0]);
        return (double)a[0] * (double)b[0] + (double)a[1] * (double)b[1];
    }
    if (FAST)
        return fmaT((double)a[2], (double)b[2], fmaT((double)a[1], (double)b[1], (double)a[0] * (double)b[0]));
    return sum3((double)a[0] * (double)b[0], (double)a[1] * (double)b[1], (double)a[2] * (double)b[2]);
}
// lane partial of a dot product: the lane's first point, then its other points in index order
template <bool FAST, typename T, int PPL, int D = 3>
__device__ __forceinline__ double dot_lane(const T (&a)[PPL][3], const T (&b)[PPL][3]) {
    if constexpr (D == 1) {   // AXIS: the lane's one coordinate, then the xor-32 exchange — the add dot3<.., 2> does
        static_assert(!FAST && PPL == 1, "the axis-per-lane layout is reference order, one point per lane pair");
        return dot_xy((double)a[0][0], (double)b[0][0]);
    } else {
        double s = dot3<FAST, T, D>(a[0], b[0]);
#pragma unroll
        for (int q = 1; q < PPL; ++q) s += dot3<FAST, T, D>(a[q], b[q]);
        return s;
    }
}

// ys of a history pair as the two-loop uses it (LB:1300, :1312 divide by it).  FAST keeps only the
// reciprocal in v.  The reference-order mode keeps ys in v and its correctly rounded reciprocal in
// r (YSv<false>): the steady-state two-loop divides with Markstein's sequence q = a*r, e = fma(-q, ys, a),
// q' = fma(e, r, q) — the correctly rounded a/ys, the same bits as the 13-instruction fp64
// division, whenever r = RN(1/ys) and nothing over/underflows (Markstein 1990; checked against
// 4e8 random divisions incl. all-ones significands).  r is NaN for a ys outside 2^+-500, the
// dividends' magnitudes are tracked with one max and one min per step, and a two-loop that saw a
// dividend outside 2^+-500 (or produced a NaN) is repeated with true divisions.
template <bool FAST>
struct YSv {            // reference-order mode
    double v, r;
};
template <>
struct YSv<true> {      // FAST: the reciprocal only
    double v;
};
__device__ __forceinline__ bool exp_in_safe_range(double a) {
    const unsigned e = ((unsigned)__double2hiint(a) >> 20) & 0x7ffu;
    return (e - 523u) < 1000u;
}
__device__ __forceinline__ YSv<true> make_ys(double ys, YSv<true>*) { return YSv<true>{1.0 / ys}; }
__device__ __forceinline__ YSv<false> make_ys(double ys, YSv<false>*) {
    return YSv<false>{ys, exp_in_safe_range(ys) ? 1.0 / ys : __builtin_nan("")};
}
template <bool MARK>
__device__ __forceinline__ double over_ys(double a, const YSv<true>& y, double&, double&) { return a * y.v; }
template <bool MARK>
__device__ __forceinline__ double over_ys(double a, const YSv<false>& y, double& amin, double& amax) {
    if (!MARK) return a / y.v;
    const double q = a * y.r;
    const double e = __builtin_fma(-q, y.v, a);
    amin = fmin(amin, fabs(a));
    amax = fmax(amax, fabs(a));
    return __builtin_fma(e, y.r, q);
}

// Which two-loop recursion k_optimize's `two_loop` runs: STEADY (value) = the history is full, straight-line code; MARK =
// it divides by ys with Markstein's sequence and reports whether it has to be repeated with true divisions.
template <bool STEADY, bool MARK>
struct TwoLoopTag {
    static constexpr bool value = STEADY;
};
template <bool FAST, bool STEADY>
constexpr bool two_loop_mark(std::integral_constant<bool, STEADY>) { return STEADY && !FAST; }
template <bool FAST, bool STEADY, bool MARK>
constexpr bool two_loop_mark(TwoLoopTag<STEADY, MARK>) { return MARK; }

// one L-BFGS history pair of one control point as it sits in LDS (48 B in fp64: three
// conflict-free ds_read_b128 per lane, one address register)
template <typename T, int D = 3>
struct alignas(16) HPair {
    T s[D];
    T y[D];
};

// per-lane view of one trajectory's inputs
template <typename T, int PPL>
struct LaneProblem {
    // guide pairs per control point kept in VGPRs (more: re-read from HBM/L2 every evaluation)
    static constexpr int kGuideRegs = (PPL == 1) ? 2 : 0;
    static constexpr int kGuideDim = kGuideRegs > 0 ? kGuideRegs : 1;
    int N;
    // LEVEL RULE (include/vigo.h): plan_in_z off and all N control points at one height to 2^-40 relative — the z
    // coordinate then feels only the smoothness and feasibility terms of values that differ by rounding noise; those
    // z terms are taken as exactly zero (cost and gradient), so z never moves.  Group-uniform; set by set_level().
    bool level;
    int p0;                   // first control point of this lane
    bool has_pt[PPL];         // p0 + q < N
    bool interior[PPL];       // 3 <= p0 + q <= N-4 (a free control point)
    int g_begin[PPL], g_end[PPL];
    const double* gpv;
    const uint8_t* gunk;
    T gq[kGuideDim][6];       // (PPL == 1) the first pairs, loaded once per solve: they never move
    bool gqu[kGuideDim];
    int o_begin, o_end;       // this trajectory's obstacles
    const double* obs;
    // (whole-solve kernel) the first o_tab obstacles of this trajectory as a table in LDS:
    // obs_tab[3 * (j * o_steps + s)] = {x, y, threshold} at predicted step n = 2 s, then the sizes
    // at obs_tab[3 * entries + j].  Staged once per solve: nothing in it depends on the control
    // points, and a global load per obstacle per evaluation is a ~2 us round trip on the critical path
    const double* obs_tab;
    const double* obs_size;
    int o_tab, o_steps;
    double w[4];
};

// The constants an L-BFGS iteration uses, for the iteration loop of k_optimize and the helpers it calls — the type KC
// below.  It is DevConst itself, in memory, wherever the kernel sits at the register limit (every instantiation but
// AXIS): a uniform address, scalar loads at the use sites, not 100+ live SGPRs.  The AXIS kernel has a wave alone on
// its SIMD and registers to spare, and there every one of those loads is a scalar-cache round trip that nothing else
// covers (profiles/README.md): it reads the fields ONCE, at entry, into a HotConst.  The same field names, so one text
// serves both; the same values, so the same bits.  Read from the device copy at every launch: vigo_set_params between
// two solves takes effect as before.
__device__ __forceinline__ void hold_in_reg(double& v) { asm volatile("" : "+v"(v)); }   // opaque from here on: the compiler
__device__ __forceinline__ void hold_in_reg(int& v) { asm volatile("" : "+s"(v)); }      // cannot go back to memory for it
// v becomes a register of unspecified content, at no cost: for a variable of an iteration's scope that is written before
// it is read, but not on every path — without this its value of the iteration before stays live across the whole loop
__device__ __forceinline__ void fresh_reg(double& v) { asm volatile("" : "=v"(v)); }
__device__ __forceinline__ void fresh_reg(int& v) { asm volatile("" : "=s"(v)); }
struct HotConst {
    double dth, da, db, dc, unc_factor;                          // distance term
    double ts_ctrl, ts_inv_sqr;                                  // stencils
    double g_epsilon, min_step, max_step, ftol, gtol, xtol;      // L-BFGS and the line search
    int max_iterations, max_linesearch;
    // derived once at entry (vigo_exact_div.hpp): RN(1 / ts_ctrl) and the bound below which the velocity stencil's first
    // dividend lets both of its divisions take Markstein's sequence (ConstDiv's lim2; NaN and 0 for a ts_ctrl outside
    // 2^+-500); RN(g_epsilon^2) and whether the convergence filter may decide at all
    double ts_rcp, ts_lim, g_eps2;
    int conv_ok;
    __device__ __forceinline__ explicit HotConst(const DevConst& K)
        : dth(K.dth), da(K.da), db(K.db), dc(K.dc), unc_factor(K.unc_factor), ts_ctrl(K.ts_ctrl), ts_inv_sqr(K.ts_inv_sqr),
          g_epsilon(K.g_epsilon), min_step(K.min_step), max_step(K.max_step), ftol(K.ftol), gtol(K.gtol), xtol(K.xtol),
          max_iterations(K.max_iterations), max_linesearch(K.max_linesearch) {
        hold_in_reg(dth); hold_in_reg(da); hold_in_reg(db); hold_in_reg(dc); hold_in_reg(unc_factor);
        hold_in_reg(ts_ctrl); hold_in_reg(ts_inv_sqr);
        hold_in_reg(g_epsilon); hold_in_reg(min_step); hold_in_reg(max_step); hold_in_reg(ftol); hold_in_reg(gtol); hold_in_reg(xtol);
        hold_in_reg(max_iterations); hold_in_reg(max_linesearch);
        const ConstDiv cd = make_const_div(ts_ctrl);
        const ConvFilter cf = make_conv_filter(g_epsilon);
        ts_rcp = cd.r; ts_lim = cd.lim2; g_eps2 = cf.eps2;
        conv_ok = __builtin_amdgcn_readfirstlane((int)cf.ok);   // (from g_epsilon in a vector register: the same in every lane)
        hold_in_reg(ts_rcp); hold_in_reg(ts_lim); hold_in_reg(g_eps2); hold_in_reg(conv_ok);
    }
};
template <bool HOT>
using LoopConst = std::conditional_t<HOT, HotConst, const DevConst&>;

// One guide pair's contribution, BT.cpp:839-895.  e == dthresh takes the cubic branch (first
// else-if wins); the "too far" branch is never scaled by the unknown factor.
// the penalty at signed distance `dist` from the pair's plane: cost ct, gradient factor k along the pair's direction,
// and whether the unknown factor scales both; false in the no-penalty band
template <typename T, class KC>
__device__ __forceinline__ bool guide_penalty(const KC& K, T dist, bool unk, T& ct, T& k, bool& scale) {
    const T dth = (T)K.dth, da = (T)K.da, db = (T)K.db, dcc = (T)K.dc;
    const T e = dth - dist;
    scale = false;
    if (e <= -dth) {
        const T ne = -e;
        ct = (ne * ne) * ne;
        k = T(3.0) * (ne * ne);
    } else if (e > T(0) && e <= dth) {
        ct = (e * e) * e;
        k = T(-3.0) * (e * e);
        scale = unk;
    } else if (e >= dth) {
        ct = (da * (e * e) + db * e) + dcc;
        k = -((T(2) * da) * e + db);
        scale = unk;
    } else {
        return false;  // -dthresh < e <= 0 (or NaN): no penalty
    }
    return true;
}
template <bool FAST, typename T>
__device__ __forceinline__ void guide_pair_term(const DevConst& K, const T (&c)[3], T px, T py, T pz, T vx,
                                                T vy, T vz, bool unk, double& cd, T (&Gd)[3]) {
    const T uf = (T)K.unc_factor;
    const T dist = FAST ? fmaT(c[2] - pz, vz, fmaT(c[1] - py, vy, (c[0] - px) * vx))
                        : ((c[0] - px) * vx + (c[1] - py) * vy) + (c[2] - pz) * vz;
    T ct, k;
    bool scale;
    if (!guide_penalty<T>(K, dist, unk, ct, k, scale)) return;
    T gx = k * vx, gy = k * vy, gz = k * vz;
    if (scale) { ct *= uf; gx *= uf; gy *= uf; gz *= uf; }
    if (!K.plan_in_z) gz = T(0.0);
    cd += (double)ct;
    Gd[0] += gx; Gd[1] += gy; Gd[2] += gz;
}
// The same term in the AXIS layout (level trajectory, reference order): c, p, v are THIS lane's coordinate of the
// point, of the pair's position and of its direction.  Each lane forms its own product, the xor-32 exchange adds the
// two in the order above, the z product follows; both lanes of a point then hold the same dist, take the same branch
// and count the same cost (callers reduce it over one half of the wave only), and each scales its own v for the gradient.
// Must be reached by both lanes of a point together: the exchange reads the partner lane.
template <class KC>
__device__ __forceinline__ void guide_pair_term_axis(const KC& K, double c, double cz, double p, double pz, double v, double vz,
                                                     bool unk, double& cd, double& Gd) {
    const double uf = K.unc_factor;
    const double dist = dot_xy(c - p, v) + (cz - pz) * vz;
    double ct, k;
    bool scale;
    if (!guide_penalty<double>(K, dist, unk, ct, k, scale)) return;
    double gc = k * v;
    if (scale) { ct *= uf; gc *= uf; }
    cd += ct;
    Gd += gc;
}

// One dynamic obstacle's contribution to one control point, BT.cpp:1011-1059: the obstacle at its
// predicted positions n = 0, 2, .., predictionNum (skipFactor = 2, BT.cpp:1006).
template <typename T>
__device__ __forceinline__ void obstacle_term(const DevConst& K, const T (&c)[3], T opx, T opy, T ovx, T ovy, T size,
                                              double& co, T (&Go)[3]) {
    const T thr0 = (T)K.thr_dyn, oa = (T)K.oa, ob = (T)K.ob, oc = (T)K.oc;
    for (int n = 0; n <= K.pred_num; n += 2) {
        const T tn = (T)((double)n * K.ts);
        const T px = opx + tn * ovx, py = opy + tn * ovy;
        // integer division n/predictionNum, BT.cpp:1020
        const T thr = (T(1) - (T)(n / K.pred_num) * T(0.2)) * thr0;
        const T dx = c[0] - px, dy = c[1] - py, dz = T(0.0);
        const T nrm = sqrt((dx * dx + dy * dy) + dz * dz);
        const T e = thr - (nrm - size);
        // BT.cpp:1030-1058: e <= 0 no punishment; 0 < e <= thr cubic; e >= thr quadratic.  The two
        // penalty branches share their tail — grad = diff / |diff| (BT.cpp:1025) and the
        // accumulation — so a wave whose lanes split between them pays the three fp64 divisions
        // once, and a far step pays none.
        if (e > T(0)) {
            const bool cubic = e <= thr;
            const T ct = cubic ? (e * e) * e : (oa * (e * e) + ob * e) + oc;
            const T k = cubic ? T(-3.0) * (e * e) : -((T(2) * oa) * e + ob);
            co += (double)ct;
            Go[0] += k * (dx / nrm); Go[1] += k * (dy / nrm);
            // diff.z = 0 (BT.cpp:1022): for a finite positive |diff| the z term is k * (+0) = +-0 and
            // leaves the +0 (or NaN) accumulator as it is, so its fp64 division is only issued in
            // the degenerate cases (control point exactly on the predicted centre, NaN/inf input)
            if (__builtin_expect(!(nrm > T(0) && nrm < (T)INFINITY), 0)) Go[2] += k * (dz / nrm);
        }
    }
}

// The same term with the per-step operands {px, py, thr} read from the solve kernel's LDS table
// (they were computed there by the expressions above, so the bits are the same).
template <typename T>
__device__ __forceinline__ void obstacle_term_tab(const DevConst& K, const T (&c)[3], const double* tab, int steps,
                                                  T size, double& co, T (&Go)[3]) {
    const T oa = (T)K.oa, ob = (T)K.ob, oc = (T)K.oc;
    for (int s = 0; s < steps; ++s) {
        const T px = (T)tab[3 * s + 0], py = (T)tab[3 * s + 1], thr = (T)tab[3 * s + 2];
        const T dx = c[0] - px, dy = c[1] - py, dz = T(0.0);
        const T nrm = sqrt((dx * dx + dy * dy) + dz * dz);
        const T e = thr - (nrm - size);
        if (e > T(0)) {
            const bool cubic = e <= thr;
            const T ct = cubic ? (e * e) * e : (oa * (e * e) + ob * e) + oc;
            const T k = cubic ? T(-3.0) * (e * e) : -((T(2) * oa) * e + ob);
            co += (double)ct;
            Go[0] += k * (dx / nrm); Go[1] += k * (dy / nrm);
            if (__builtin_expect(!(nrm > T(0) && nrm < (T)INFINITY), 0)) Go[2] += k * (dz / nrm);
        }
    }
}

// The axis kernel's convergence test, G = g.g and X = x.x of the last evaluation (LB:1154-1157 on the first trip,
// LB:1200-1225 per iteration): conv_filter decides from the squared norms wherever its guard band allows; undecided —
// every lane holds the same sums, so the branch is the wave's — it is the reference expression, as in every other kernel.
__device__ __forceinline__ bool axis_converged(const HotConst& K, double G, double X) {
    const int f = conv_filter(G, X, ConvFilter{K.g_eps2, K.conv_ok != 0});
    if (__builtin_expect(!__any(f < 0), 1)) return f != 0;
    double xnorm = sqrt(X);
    const double gnorm = sqrt(G);
    if (xnorm < 1.0) xnorm = 1.0;
    return gnorm / xnorm <= K.g_epsilon;
}

// The smoothness and feasibility stencils of ONE coordinate, C = that coordinate of the lane's points: jerk, velocity
// and acceleration terms (jj, vv, aa: the cost partials of the term whose first point is the lane's) and the gradient
// columns Gs, Gf of the lane's points.  no_terms: the z coordinate of a level trajectory in the general kernel.
template <typename T, int PPL, bool FAST, class KC>
__device__ __forceinline__ void stencil_axis(const KC& K, const T (&C)[PPL], bool no_terms, double (&jj)[PPL],
                                             double (&vv)[PPL], double (&aa)[PPL], T (&Gs)[PPL], T (&Gf)[PPL]) {
    const T ts = (T)K.ts_ctrl, tis = (T)K.ts_inv_sqr;
    auto excess = [](T v) -> T { return v > T(1.0) ? v - T(1.0) : (v < T(-1.0) ? v + T(1.0) : T(0.0)); };
    T P1[PPL], P2[PPL], P3[PPL];
    seq_next<T, PPL>(C, P1);
    seq_next<T, PPL>(P1, P2);
    seq_next<T, PPL>(P2, P3);
    T gt0[PPL], gv[PPL], ga[PPL];
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        // smoothness, BT.cpp:934-950
        T J0 = FAST ? fmaT(T(3), P1[q], fmaT(T(-3), P2[q], P3[q])) - C[q]
                    : ((P3[q] - 3 * P2[q]) + 3 * P1[q]) - C[q];
        if (no_terms) J0 = T(0);                                       // level rule: no z terms
        gt0[q] = T(2.0) * J0;                                          // gradTemp
        jj[q] = (double)(J0 * J0);
        // feasibility, BT.cpp:952-999 (limits hard-coded to 1.0, :955-956)
        // AXIS (HotConst, fp64): both divisions by ts_ctrl as ConstDiv's quotient (vigo_exact_div.hpp) on the reciprocal
        // taken at entry, behind ONE wave-uniform test of the first dividend: usable2 answers for the second dividend
        // too, which is 2 excess(the first quotient).  A wave with a lane that fails it (NaN, infinite, too large, or
        // ts_ctrl outside 2^+-500) divides twice.  What each quotient may rely on:
        //   the first feeds excess() alone, which asks only whether it passes 1 in magnitude and returns the literal
        //   +0.0 otherwise — what ConstDiv guarantees for EVERY usable dividend, -0 and the ones below 2^-500 included
        //   (the lanes without a point hold a zero here, and no zero sends the wave to the division);
        //   the second dividend is +0.0, in almost every lane, or 2 (|v| - 1) with |v| > 1: never -0 and never below
        //   2^-51 in magnitude, so its quotient has the division's bits, the sign of the zero included.
        constexpr bool kMark = VIGO_AXIS_TS_MARK && std::is_same_v<KC, HotConst> && std::is_same_v<T, double>;
        T evP, gq = T(0);                                              // velocity i; (2 evP) / ts
        if constexpr (kMark) {
            const ConstDiv cd{K.ts_ctrl, K.ts_rcp, K.ts_lim, K.ts_lim};
            T a = P1[q] - C[q];
            if (__builtin_expect(__any(!cd.usable2(a)), 0)) {
                hold_in_reg(a);   // keeps the divisions behind the branch: hoisted and selected, they are issued every time
                evP = excess(a / ts);
                if (no_terms) evP = T(0);
                gq = (T(2) * evP) / ts;
            } else {
                evP = excess(cd.quotient(a));
                if (no_terms) evP = T(0);
                gq = cd.quotient(T(2) * evP);
            }
        } else {
            evP = excess((P1[q] - C[q]) / ts);
        }
        T eaP = excess((FAST ? fmaT(T(-2), P1[q], P2[q]) + C[q]
                             : (P2[q] - 2 * P1[q]) + C[q]) * tis);     // acceleration i
        if (no_terms) { evP = T(0); eaP = T(0); }
        // gradient(j,i+1) += 2(v-vmax)/ts*tsInvSqr, gradient(j,i) += the negation (exactly)
        if constexpr (!kMark) gq = (T(2) * evP) / ts;
        gv[q] = gq * tis;
        // gradient(j,i), (j,i+2) += 2(a-amax)*tsInvSqr; gradient(j,i+1) += -4(..) = -2x that (exactly)
        ga[q] = (T(2) * eaP) * tis;
        vv[q] = (double)((evP * evP) * tis);
        aa[q] = (double)(eaP * eaP);
    }
    T gt1[PPL], gt2[PPL], gt3[PPL], gvM[PPL], gaM1[PPL], gaM2[PPL];
    seq_prev<T, PPL>(gt0, gt1);
    seq_prev<T, PPL>(gt1, gt2);
    seq_prev<T, PPL>(gt2, gt3);
    seq_prev<T, PPL>(gv, gvM);
    seq_prev<T, PPL>(ga, gaM1);
    seq_prev<T, PPL>(gaM1, gaM2);
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        T acc = gt3[q];                    // i-3: col(i+3) += gradTemp
        if (FAST) {
            acc = fmaT(T(-3.0), gt2[q], acc);
            acc = fmaT(T(3.0), gt1[q], acc);
        } else {
            acc += T(-3.0) * gt2[q];       // i-2: col(i+2) += -3*gradTemp
            acc += T(3.0) * gt1[q];        // i-1: col(i+1) += 3*gradTemp
        }
        acc += -gt0[q];                    // i  : col(i)   += -gradTemp
        Gs[q] = acc;
        T fcc = gvM[q];                    // i-1: gradient(j,i+1)
        fcc += -gv[q];                     // i  : gradient(j,i)
        fcc += gaM2[q];                    // i-2: gradient(j,i+2)
        fcc += -(T(2) * gaM1[q]);          // i-1: gradient(j,i+1)
        fcc += ga[q];                      // i  : gradient(j,i)
        Gf[q] = fcc;
    }
}

// ---- cost + gradient at the points held in c (BT.cpp:802-821) ---------------------------
// T is the element type of points/gradients; sums are fp64.  g receives the weighted gradient
// of the free points, 0 elsewhere.  ONE 7-value group reduction returns
//   sums[0..3] = un-weighted distance / smoothness / feasibility / dynamic costs,
//   sums[4] = g.d, sums[5] = x.x over the free points, sums[6] = g.g
// (the line search needs g.d after every evaluation, LB:829, and the norms after the last one,
// LB:1200-1201; fusing them costs three more DPP chains instead of two more reductions).
// Returns the weighted total cost (group-uniform).
template <typename T, int GROUP, int PPL, bool FAST, bool OBS = true, int D = 3>
__device__ __forceinline__ double eval_cost_grad(const DevConst& K, const LaneProblem<T, PPL>& Q,
                                                 const T (&c)[PPL][3], const T (&d)[PPL][3], T (&g)[PPL][3],
                                                 double (&sums)[7]) {
    using LP = LaneProblem<T, PPL>;
    const int N = Q.N;
    T Gd[PPL][3], Gs[PPL][3], Gf[PPL][3], Go[PPL][3];
    double pt_s[PPL], pt_f[PPL], pt_d[PPL], pt_o[PPL];  // per-point cost partials
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        pt_s[q] = pt_f[q] = pt_d[q] = pt_o[q] = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) Gd[q][a] = Go[q][a] = T(0);
    }

    // Every point evaluates the stencil term whose FIRST point it is (index i = its own): jerk_i,
    // velocity_i, acceleration_i and their gradient magnitudes.  A control point's gradient is the
    // reference's scatter-add seen from the receiving column: the terms of i-3..i, which are the
    // SAME expressions evaluated at the points below, fetched with register renames / DPP shifts —
    // identical bits, no recomputation (and half the fp64 divisions by ts).
    {
        double jj[PPL][3], vv[PPL][3], aa[PPL][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a >= D) {   // a level trajectory: these stencil terms and their gradients are exactly zero (checked at entry)
#pragma unroll
                for (int q = 0; q < PPL; ++q) { jj[q][a] = vv[q][a] = aa[q][a] = 0.0; Gs[q][a] = Gf[q][a] = T(0); }
                continue;
            }
            T C[PPL], GsA[PPL], GfA[PPL];
            double jjA[PPL], vvA[PPL], aaA[PPL];
#pragma unroll
            for (int q = 0; q < PPL; ++q) C[q] = c[q][a];
            stencil_axis<T, PPL, FAST>(K, C, a == 2 && Q.level, jjA, vvA, aaA, GsA, GfA);
#pragma unroll
            for (int q = 0; q < PPL; ++q) { jj[q][a] = jjA[q]; vv[q][a] = vvA[q]; aa[q][a] = aaA[q]; Gs[q][a] = GsA[q]; Gf[q][a] = GfA[q]; }
        }
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int p = Q.p0 + q;
            if (Q.has_pt[q] && p <= N - 4) pt_s[q] = sum3(jj[q][0], jj[q][1], jj[q][2]);
            // velocity i (x,y,z) then acceleration i (x,y,z)
            double cf = 0.0;
            if (Q.has_pt[q] && p <= N - 2) cf = (vv[q][0] + vv[q][1]) + vv[q][2];
            if (Q.has_pt[q] && p <= N - 3) { cf += aa[q][0]; cf += aa[q][1]; cf += aa[q][2]; }
            pt_f[q] = cf;
        }
    }

    // ---- guide-point distance, BT.cpp:823-932 ----
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        if (Q.interior[q]) {
            double cd = 0.0;
            const int cnt = Q.g_end[q] - Q.g_begin[q];
#pragma unroll
            for (int j = 0; j < LP::kGuideRegs; ++j) {
                if (j < cnt)
                    guide_pair_term<FAST, T>(K, c[q], Q.gq[j][0], Q.gq[j][1], Q.gq[j][2], Q.gq[j][3], Q.gq[j][4], Q.gq[j][5],
                                       Q.gqu[j], cd, Gd[q]);
            }
            for (int j = Q.g_begin[q] + LP::kGuideRegs; j < Q.g_end[q]; ++j) {
                const double* pv = Q.gpv + 6 * (size_t)j;
                guide_pair_term<FAST, T>(K, c[q], (T)pv[0], (T)pv[1], (T)pv[2], (T)pv[3], (T)pv[4], (T)pv[5],
                                   Q.gunk ? (Q.gunk[j] != 0) : false, cd, Gd[q]);
            }
            if (K.plan_in_z) {
                // BT.cpp:897-930, reproduced with its x-row gradient and heightDistMax band test
                const T hth = (T)K.hth, ha = (T)K.ha, hb = (T)K.hb, hc = (T)K.hc;
                const T hmin = c[q][2] - (T)K.min_h, hmax = c[q][2] - (T)K.max_h;
                if (hmin < T(0)) {
                    const T e = hth - hmin;
                    cd += (double)((ha * (e * e) + hb * e) + hc);
                    Gd[q][0] += -((T(2) * ha) * e + hb) * T(-1.0);
                } else if (hmin >= T(0) && hmax < hth) {
                    const T e = hth - hmin;
                    cd += (double)((e * e) * e);
                    Gd[q][0] += T(-3.0) * (e * e) * T(-1.0);
                }
                if (hmax > T(0)) {
                    const T e = hth + hmax;
                    cd += (double)((ha * (e * e) + hb * e) + hc);
                    Gd[q][0] += -((T(2) * ha) * e + hb) * T(1.0);
                } else if (hmax <= T(0) && hmax >= -hth) {
                    const T e = hth + hmax;
                    cd += (double)((e * e) * e);
                    Gd[q][0] += T(-3.0) * (e * e) * T(1.0);
                }
            }
            pt_d[q] = cd;
        }
    }

    // ---- dynamic obstacles, BT.cpp:1001-1064 (OBS == false: an instantiation for calls without an obstacle list) ----
    if (OBS && Q.o_end > Q.o_begin) {
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            if (!Q.interior[q]) continue;
            double co = 0.0;
            // the obstacles staged in LDS by the solve kernel first (same order as the list) ...
            for (int j = 0; j < Q.o_tab; ++j)
                obstacle_term_tab<T>(K, c[q], Q.obs_tab + 3 * j * Q.o_steps, Q.o_steps, (T)Q.obs_size[j], co, Go[q]);
            // ... then the rest (all of them for the standalone cost/gradient kernel) from HBM/L2
            for (int j = Q.o_begin + Q.o_tab; j < Q.o_end; ++j) {
                const double* o = Q.obs + 9 * (size_t)j;
                const T hx = (T)o[6] / 2, hy = (T)o[7] / 2;
                obstacle_term<T>(K, c[q], (T)o[0], (T)o[1], (T)o[3], (T)o[4], sqrt(hx * hx + hy * hy), co, Go[q]);
            }
            pt_o[q] = co;
        }
    }

    const T w0 = (T)Q.w[0], w1 = (T)Q.w[1], w2 = (T)Q.w[2], w3 = (T)Q.w[3];
    double part[7];  // lane partials: the lane's first point, then its other points in index order
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
            g[q][a] = (!Q.interior[q] || a >= D || (a == 2 && Q.level)) ? T(0)
                      : (FAST ? fmaT(w3, Go[q][a], fmaT(w2, Gf[q][a], fmaT(w1, Gs[q][a], w0 * Gd[q][a])))
                              : ((w0 * Gd[q][a] + w1 * Gs[q][a]) + w2 * Gf[q][a]) + w3 * Go[q][a]);
        const double v4 = dot3<FAST, T, D>(g[q], d[q]);
        const double v5 = Q.interior[q] ? dot3<FAST, T>(c[q], c[q]) : 0.0;     // (x.x: the level coordinate counts)
        const double v6 = dot3<FAST, T, D>(g[q], g[q]);
        if (q == 0) {
            part[0] = pt_d[0]; part[1] = pt_s[0]; part[2] = pt_f[0]; part[3] = pt_o[0];
            part[4] = v4; part[5] = v5; part[6] = v6;
        } else {
            part[0] += pt_d[q]; part[1] += pt_s[q]; part[2] += pt_f[q]; part[3] += pt_o[q];
            part[4] += v4; part[5] += v5; part[6] += v6;
        }
    }
    if (OBS) {
        group_sum<GROUP, 7>(part);
    } else {
        // no obstacles: the dynamic cost is a sum of zeros — 0.0, as the reduction would return — so it stays out of it
        double p6[6] = {part[0], part[1], part[2], part[4], part[5], part[6]};
        group_sum<GROUP, 6>(p6);
        part[0] = p6[0]; part[1] = p6[1]; part[2] = p6[2]; part[3] = 0.0; part[4] = p6[3]; part[5] = p6[4]; part[6] = p6[5];
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) sums[q] = part[q];
    return ((Q.w[0] * part[0] + Q.w[1] * part[1]) + Q.w[2] * part[2]) + Q.w[3] * part[3];
}

// The same evaluation in the AXIS layout: a level trajectory (fp64 reference order, no obstacles) on one whole wave,
// lane l < 32 holding coordinate 0 of control point l and lane l + 32 coordinate 1 (axis = lane >> 5).  c[0][0], d[0][0],
// g[0][0] are the lane's coordinate, c[0][2] the point's z (both lanes hold it; it never moves); Q.gq[j][0] / [3] hold
// the lane's coordinate of the register-held pairs (axis_guides()).  The stencils run on the lane's axis alone, inside its
// half of the wave.  Wherever eval_cost_grad<.., D = 2> adds the x term and the y term of a point, the xor-32 exchange
// hands both lanes both terms and they add them in that order; what follows (the exact-zero z terms, the 32-lane tree)
// is then the same in both halves, which end with the same bits in every sum — and so with the same line-search scalars.
// VIGO_AXIS_PAIR_EVAL: the six sums go through three trees as pairs, one sum per half (pair_tree32), whose last exchange
// hands every lane both totals: the same bits in every sum, in both halves, as before.
template <class KC>
__device__ __forceinline__ double eval_cost_grad_axis(const KC& K, const LaneProblem<double, 1>& Q, int axis,
                                                      const double (&c)[1][3], const double (&d)[1][3], double (&g)[1][3],
                                                      double (&sums)[7]) {
    using LP = LaneProblem<double, 1>;
    const int N = Q.N, p = Q.p0;
    const double C[1] = {c[0][0]};
    const double cz = c[0][2];
    double jj[1], vv[1], aa[1], Gs[1], Gf[1];
    stencil_axis<double, 1, false>(K, C, false, jj, vv, aa, Gs, Gf);
    // (the trailing zeros are the z terms of eval_cost_grad<.., D = 2>, kept where it adds them)
    double pt_s = 0.0, pt_f = 0.0, pt_d = 0.0;
    double pt_sf = 0.0;   // PAIR_EVAL: [pt_s | pt_f], the smoothness partial in the lower half, the feasibility one in the upper
    if constexpr (VIGO_AXIS_PAIR_EVAL) {
        // pack_xy(jj, vv) = [j0 + j1 | v0 + v1]: the first add of sum3(j0, j1, 0.0) and of (v0 + v1) + 0.0, each in the half
        // that carries it; the + 0.0 that follows is the same statement in both.  The acceleration terms belong to pt_f
        // alone: they are added in the upper half only, after the velocity terms, in the order below.
        double a0, a1;
        xy_both(aa[0], a0, a1);
        const double t = pack_xy(jj[0], vv[0]) + 0.0;
        if (Q.has_pt[0] && p <= (axis ? N - 2 : N - 4)) pt_sf = t;
        if (axis && Q.has_pt[0] && p <= N - 3) { pt_sf += a0; pt_sf += a1; pt_sf += 0.0; }
    } else {
        double j0, j1, v0, v1, a0, a1;
        xy_both(jj[0], j0, j1);
        xy_both(vv[0], v0, v1);
        xy_both(aa[0], a0, a1);
        if (Q.has_pt[0] && p <= N - 4) pt_s = sum3(j0, j1, 0.0);
        if (Q.has_pt[0] && p <= N - 2) pt_f = (v0 + v1) + 0.0;
        if (Q.has_pt[0] && p <= N - 3) { pt_f += a0; pt_f += a1; pt_f += 0.0; }
    }

    // ---- guide-point distance: both lanes of a point enter together (interior and the pair range are per point) ----
    double Gd = 0.0;
    if (Q.interior[0]) {
        double cd = 0.0;
        const int cnt = Q.g_end[0] - Q.g_begin[0];
#pragma unroll
        for (int j = 0; j < LP::kGuideRegs; ++j) {
            if (j < cnt) guide_pair_term_axis(K, C[0], cz, Q.gq[j][0], Q.gq[j][2], Q.gq[j][3], Q.gq[j][5], Q.gqu[j], cd, Gd);
        }
        for (int j = Q.g_begin[0] + LP::kGuideRegs; j < Q.g_end[0]; ++j) {
            const double* pv = Q.gpv + 6 * (size_t)j;
            guide_pair_term_axis(K, C[0], cz, pv[axis], pv[2], pv[3 + axis], pv[5], Q.gunk ? (Q.gunk[j] != 0) : false, cd, Gd);
        }
        pt_d = cd;
    }

    const double w0 = Q.w[0], w1 = Q.w[1], w2 = Q.w[2], w3 = Q.w[3];
    const double Go = 0.0;
    g[0][0] = !Q.interior[0] ? 0.0 : ((w0 * Gd + w1 * Gs[0]) + w2 * Gf[0]) + w3 * Go;
    g[0][1] = g[0][2] = 0.0;
    if constexpr (VIGO_AXIS_PAIR_EVAL) {
        const double xx = dot_xy(C[0], C[0]) + cz * cz;                      // (x.x: the level coordinate counts)
        // six sums as three pairs, one sum per half of the wave (pair_tree32): [pt_d | x.x], [pt_s | pt_f], [g.d | g.g].
        // pt_d and x.x are the same in both lanes of a point: each half keeps the one it carries.  g.d and g.g are
        // dot_xy() of per-lane products: pack_xy() forms both exchange adds at once.
        double v3[3], lo[3], hi[3];
        v3[0] = axis ? (Q.interior[0] ? xx : 0.0) : pt_d;
        v3[1] = pt_sf;
        v3[2] = pack_xy(g[0][0] * d[0][0], g[0][0] * g[0][0]);
        pair_tree32<3>(v3, lo, hi);
        sums[0] = lo[0]; sums[1] = lo[1]; sums[2] = hi[1]; sums[3] = 0.0; sums[4] = lo[2]; sums[5] = hi[0]; sums[6] = hi[2];
    } else {
        double p6[6];
        p6[0] = pt_d; p6[1] = pt_s; p6[2] = pt_f;
        p6[3] = dot_xy(g[0][0], d[0][0]);
        const double xx = dot_xy(C[0], C[0]) + cz * cz;                      // (x.x: the level coordinate counts)
        p6[4] = Q.interior[0] ? xx : 0.0;
        p6[5] = dot_xy(g[0][0], g[0][0]);
        group_sum<32, 6>(p6);
        sums[0] = p6[0]; sums[1] = p6[1]; sums[2] = p6[2]; sums[3] = 0.0; sums[4] = p6[3]; sums[5] = p6[4]; sums[6] = p6[5];
    }
    return ((Q.w[0] * sums[0] + Q.w[1] * sums[1]) + Q.w[2] * sums[2]) + Q.w[3] * sums[3];
}

// AXIS layout: keep this lane's coordinate of the register-held guide pairs where eval_cost_grad_axis() reads it
__device__ __forceinline__ void axis_guides(LaneProblem<double, 1>& Q, int axis) {
#pragma unroll
    for (int j = 0; j < LaneProblem<double, 1>::kGuideDim; ++j) {
        Q.gq[j][0] = axis ? Q.gq[j][1] : Q.gq[j][0];
        Q.gq[j][3] = axis ? Q.gq[j][4] : Q.gq[j][3];
    }
}

// MIXED (vigo_*_mixed): A.N is the row STRIDE of ctrl, guide_off and the outputs, trajectory b has A.n_pts[b] control
// points.  The count is device data: one outside [7, A.N], or of the other shape class than the launch's (shape_for:
// GROUP lanes per trajectory), gives a problem WITHOUT points — Q.N = 0: no lane has a point, none is free, nothing of
// the row is read or written — and false; the caller reports it and leaves.
// (the count array is a field of MixedSolveArgs, not of SolveArgs: the kernel arguments of every other instantiation,
// and with them the offsets their code loads from, stay what they were)
template <bool MIXED> using SolveArgsOf = std::conditional_t<MIXED, MixedSolveArgs, SolveArgs>;
template <typename T, int GROUP, int PPL, bool MIXED = false>
__device__ __forceinline__ bool load_problem(const SolveArgsOf<MIXED>& A, const DevConst& K, int b, int lane_in_group,
                                             LaneProblem<T, PPL>& Q) {
    using LP = LaneProblem<T, PPL>;
    int N = A.N;
    bool valid = true;
    if constexpr (MIXED) {
        static_assert(PPL == 1, "mixed counts: one control point per lane (Ns <= 64)");
        const int n = A.n_pts[b];
        valid = n >= 7 && n <= A.N && shape_for(n).group == GROUP;
        N = valid ? n : 0;
    }
    Q.N = N;
    Q.level = false;
    Q.p0 = lane_in_group * PPL;
    Q.gpv = A.guide_pv;
    Q.gunk = A.guide_unk;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        const int p = Q.p0 + q;
        Q.has_pt[q] = p < N;
        Q.interior[q] = (p >= 3) && (p <= N - 4);
        Q.g_begin[q] = Q.g_end[q] = 0;
        if (Q.interior[q] && A.guide_off && A.guide_pv) {   // offsets without pairs: no guides
            Q.g_begin[q] = A.guide_off[(size_t)b * (MIXED ? A.N : N) + p];
            Q.g_end[q] = A.guide_off[(size_t)b * (MIXED ? A.N : N) + p + 1];
        }
    }
#pragma unroll
    for (int j = 0; j < LP::kGuideDim; ++j) {
        Q.gqu[j] = false;
#pragma unroll
        for (int q = 0; q < 6; ++q) Q.gq[j][q] = T(0);
        if (j < LP::kGuideRegs && Q.g_begin[0] + j < Q.g_end[0]) {
            const double* pv = A.guide_pv + 6 * (size_t)(Q.g_begin[0] + j);
#pragma unroll
            for (int q = 0; q < 6; ++q) Q.gq[j][q] = (T)pv[q];
            Q.gqu[j] = A.guide_unk ? (A.guide_unk[Q.g_begin[0] + j] != 0) : false;
        }
    }
    Q.obs = A.obs;
    Q.obs_tab = Q.obs_size = nullptr;
    Q.o_tab = Q.o_steps = 0;
    if (!A.obs) {                    // offsets (or a shared count) without the list: no obstacles
        Q.o_begin = Q.o_end = 0;
    } else if (A.obs_off) {
        Q.o_begin = A.obs_off[b];
        Q.o_end = A.obs_off[b + 1];
    } else {
        Q.o_begin = 0;
        Q.o_end = A.obs ? A.n_obs_shared : 0;
    }
    if (A.weights) {
#pragma unroll
        for (int q = 0; q < 4; ++q) Q.w[q] = A.weights[4 * (size_t)b + q];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) Q.w[q] = K.w[q];
    }
    return valid;
}

template <typename T, int PPL>
__device__ __forceinline__ void load_points(const SolveArgs& A, int b, const LaneProblem<T, PPL>& Q, T (&x)[PPL][3]) {
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        x[q][0] = x[q][1] = x[q][2] = T(0);
        if (Q.has_pt[q]) {
            const double* src = A.ctrl + ((size_t)b * A.N + Q.p0 + q) * 3;
            x[q][0] = (T)src[0]; x[q][1] = (T)src[1]; x[q][2] = (T)src[2];
        }
    }
}

// the level rule's test on the control points a group holds (every lane of the group gets the same answer)
template <typename T, int GROUP, int PPL>
__device__ __forceinline__ void set_level(const DevConst& K, LaneProblem<T, PPL>& Q, const T (&x)[PPL][3]) {
    double mn = INFINITY, mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        if (Q.has_pt[q]) { mn = fmin(mn, (double)x[q][2]); mx = fmax(mx, (double)x[q][2]); }
    }
    group_minmax<GROUP>(mn, mx);
    Q.level = !K.plan_in_z && !K.strict_z && (mx - mn) <= 0x1p-40 * fmax(1.0, fmax(fabs(mn), fabs(mx)));
}

template <typename T, int PPL>
__device__ __forceinline__ void store_points(const SolveArgs& A, int b, const LaneProblem<T, PPL>& Q, const T (&x)[PPL][3]) {
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        if (Q.has_pt[q]) {
            double* dst = A.ctrl + ((size_t)b * A.N + Q.p0 + q) * 3;
            dst[0] = (double)x[q][0]; dst[1] = (double)x[q][1]; dst[2] = (double)x[q][2];
        }
    }
}

// AXIS layout (k_optimize, D == 1): each lane stores the coordinate it holds, the lane of coordinate 0 the point's z too
// (as it was loaded — the level rule — unless a two-loop coefficient was not finite, see dz in k_optimize)
__device__ __forceinline__ void store_point_axis(const SolveArgs& A, int b, const LaneProblem<double, 1>& Q, int axis, double v, double z) {
    if (!Q.has_pt[0]) return;
    double* dst = A.ctrl + ((size_t)b * A.N + Q.p0) * 3;
    dst[axis] = v;
    if (axis == 0) dst[2] = z;
}

// ---- standalone cost/gradient kernel (vigo_cost_grad) ----------------------------------
template <typename T, int GROUP, int PPL, bool FAST, bool MIXED = false>
__global__ void __launch_bounds__(kWave) k_cost_grad(SolveArgsOf<MIXED> A, const DevConst* __restrict__ Kp) {
    const DevConst& K = *Kp;  // uniform address: scalar loads at the use sites, not 100+ live SGPRs
    constexpr int TPB = kWave / GROUP;
    const int lane = threadIdx.x;
    const int b = blockIdx.x * TPB + lane / GROUP;
    if (b >= A.B) return;
    LaneProblem<T, PPL> Q;
    if (!load_problem<T, GROUP, PPL, MIXED>(A, K, b, lane % GROUP, Q)) {   // (MIXED) a bad count: NaN cost, nothing else
        if (lane % GROUP == 0 && A.out_cost) A.out_cost[b] = __builtin_nan("");
        return;
    }
    T c[PPL][3], g[PPL][3], zero[PPL][3];
    load_points<T, PPL>(A, b, Q, c);
    set_level<T, GROUP, PPL>(K, Q, c);
#pragma unroll
    for (int q = 0; q < PPL; ++q) zero[q][0] = zero[q][1] = zero[q][2] = T(0);
    double sums[7];
    const double f = eval_cost_grad<T, GROUP, PPL, FAST>(K, Q, c, zero, g, sums);
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
        if (Q.interior[q] && A.out_grad) {
            double* dst = A.out_grad + ((size_t)b * (A.N - 6) + (Q.p0 + q - 3)) * 3;
            dst[0] = (double)g[q][0]; dst[1] = (double)g[q][1]; dst[2] = (double)g[q][2];
        }
    }
    if (lane % GROUP == 0) {
        if (A.out_cost) A.out_cost[b] = f;
        if (A.out_terms) {
#pragma unroll
            for (int q = 0; q < 4; ++q) A.out_terms[4 * (size_t)b + q] = sums[q];
        }
    }
}

// ---- whole-solve kernel (vigo_optimize): BT.cpp:687-718 + LB:1024-1349 -------------------
// LDS: hist[slot][ROW] of HPair<T> with ROW = TPB*(N-6) columns (each lane reads and writes only
//      the columns of its own points: LDS is a per-lane register extension here, no cross-lane
//      traffic and no barriers), then ys[slot][TPB] and alpha[age][TPB] doubles.
// Control flow: an outer trip per L-BFGS iteration (trip 0 = the initial evaluation) with ONE
// evaluation site inside the line-search loop, so the two groups of a wave re-converge at every
// iteration boundary and run the (dominant) two-loop recursion together.
// dev builds only (-DVIGO_PROFILE_SECTIONS=1, tools/exp_sections.py): shader-clock totals of the sections of an
// iteration, written over out_x[b][0..9] — never defined in the shipped library
#ifndef VIGO_PROFILE_SECTIONS
#define VIGO_PROFILE_SECTIONS 0
#endif
#if VIGO_PROFILE_SECTIONS
#define VIGO_TICK(acc)                                                   \
    do {                                                                 \
        __builtin_amdgcn_sched_barrier(0);                               \
        const long long now_ = (long long)__builtin_readcyclecounter();  \
        __builtin_amdgcn_sched_barrier(0);                               \
        acc += (double)(now_ - tick_);                                   \
        tick_ = now_;                                                    \
    } while (0)
#else
#define VIGO_TICK(acc) do { } while (0)
#endif

// WPS = waves per SIMD the register budget is cut for.  1 (512 registers per lane, no scratch) unless the batch
// has more waves than the chip has SIMDs AND the history leaves room for eight waves in a CU's LDS (fp32 state,
// or fp64 trajectories of up to ~21 control points): capping the registers at 256 (a few hundred bytes of
// scratch per lane) then lets two waves share a SIMD's issue slots — +17 % for fp32 at 65 536 x 32, +36 % for
// fp64 at 16 384 x 16 — but costs 6 % when every wave has a SIMD to itself anyway.  Same arithmetic, same bits.
// OBS == false: the instantiation the launcher picks for calls without an obstacle list (A.obs == nullptr): no staging
// code, no obstacle loop, six sums per evaluation instead of seven — the same bits, fewer live registers
// RH = history pairs besides the newest that stay in registers (ages 1 .. RH; 0 for more than one point per lane: all in
// LDS): 1 normally; 4 or 5 in the level instantiations launched on batches that fill the chip (kLevelRH, vigo_solver_plan.hpp):
// fewer ring slots in LDS are more resident waves per CU
// MIXED: trajectories of different counts in one launch (load_problem); A.N, the row stride, sizes the LDS layout.  Only
// the general kernel has such an instantiation (D = 3, OBS): it treats a missing obstacle list as no obstacles and
// solves a level trajectory with its z terms masked, the same bits as the kernels a uniform call launches for them.
template <typename T, int GROUP, int PPL, bool FAST, int WPS = 1, bool OBS = true, int D = 3, int RH = (PPL == 1 ? 1 : 0), bool MIXED = false>
__global__ void __launch_bounds__(kWave, WPS) k_optimize(SolveArgsOf<MIXED> A, const DevConst* __restrict__ Kp) {
    // The text of the solve, vigo_solver_optimize.inc, is INCLUDED here, not called: as the body of an always-inline
    // function it comes out as other instructions in every instantiation (measured: not one kernel of the 65 kept its
    // code object digest), and the schedules of these kernels are what their rounds of measurements were spent on.
    constexpr bool SOLO = false;
#define VIGO_OPTIMIZE_ENTRY 1
#include "vigo_solver_optimize.inc"
#undef VIGO_OPTIMIZE_ENTRY
}

// The same text as a function, behind the problem load: trajectory b as the caller has loaded and classified it.
// SOLO (D = 3): ONE trajectory on lanes 0 .. 31 of a wave whose other half has returned, and an LDS layout for one: one
// history column per free control point plus the zero column, {ys, 1/ys} and the alphas of one trajectory
// (solo_lds_bytes, vigo_solver_plan.hpp).  The same operations in the same order as a group of the paired layout that
// goes on alone (see solved_elsewhere): the same bits.
template <typename T, int GROUP, int PPL, bool FAST, bool OBS, int D, bool SOLO>
__device__ __forceinline__ void optimize_loaded(const SolveArgs& A, const DevConst& K, const LoopConst<D == 1>& KL, const int b,
                                                LaneProblem<T, PPL>& Q, T (&x)[PPL][3]) {
    constexpr int RH = 1;
    constexpr bool MIXED = false;
    const bool valid_n = true;
#define VIGO_OPTIMIZE_ENTRY 0
#include "vigo_solver_optimize.inc"
#undef VIGO_OPTIMIZE_ENTRY
}

// ONE launch for the calls that plan_optimize answers with [axis-per-lane (D = 1), general (D = 3)] (fuse_optimize,
// vigo_solver_plan.hpp: fp64 reference order, N <= 32, no obstacle list, no z planning, at most one trajectory per SIMD):
// a grid of B one-wave workgroups, workgroup b loads trajectory b as the axis-per-lane kernel does and classifies it
// ONCE, from the control points as loaded.  A level trajectory goes on into the axis body; of any other, lanes 32 .. 63
// — which hold the same control points as lanes 0 .. 31 — return, and lanes 0 .. 31 run the general no-obstacle body on
// it alone (SOLO).  Both classes sit on the chip at once, one wave per SIMD, and no launch is paid whose waves all leave
// at entry.  The level flag is the same in every lane (set_level): the branch is the wave's, taken through an SGPR, so
// neither body's values stay live across the other.  Two waves per SIMD (256 registers), as two batches in flight
// need them; the LDS of either layout is at most kLdsPerWorkgroup / 8.
// The general body of k_optimize_fused, kept OUT of line: inlined next to the axis body under the 256 registers of two
// waves per SIMD, the two are allocated as one function and the axis path spills (63 VGPRs, scratch traffic all through
// its loop).  Called, each keeps the allocation it has alone: the axis path 235 registers and no scratch, this one no
// spills either; the call itself passes the loaded problem through scratch once per solve (about 90 stores and loads).
// VIGO_FUSED_JOIN, how the general body is joined (profiles/README.md, "One launch for a small batch"; 0 ships, 1 and 2
// are switches of development builds): 0, called with the kernel's own A, K and b as ordinary arguments; 1, inlined;
// 2, called, and the callee reads A and K as constant memory at a uniform address.  What a function is called with
// arrives in vector registers, and a pointer there is no uniform address: under 0 every K.field of the general body is
// a vector load on its dependent chain where the kernels have scalar loads, and a batch WITHOUT level trajectories
// pays 15 % for it; 2 has the kernel pass the address of its argument segment (the callee cannot ask for it: outside a
// kernel that pointer is null), takes it and b through SGPRs and copies the problem into locals, and is 3 % faster
// than two launches on such a batch — but the axis path, the same source, comes out scheduled 0.8 % slower next to
// that call, and the flagship gain falls below its bar.  An open end.
#ifndef VIGO_FUSED_JOIN
#define VIGO_FUSED_JOIN 0
#endif
#if VIGO_FUSED_JOIN == 2
struct FusedKernArgs { SolveArgs A; const DevConst* Kp; };   // the argument segment of k_optimize_fused
template <class P>
__device__ __forceinline__ const P& uniform_constant(const void* p) {   // *p, p the same in every lane and constant memory
    const unsigned long long u = (unsigned long long)p;
    const unsigned long long lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
    const unsigned long long hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    typedef const P __attribute__((address_space(4))) * CP;
    return *(const P*)(CP)((hi << 32) | lo);
}
__device__ __noinline__ void optimize_solo(const void* kernargs, const int b_in, const LaneProblem<double, 1>& Q_in, const double (&x_in)[1][3]) {
    const FusedKernArgs& F = uniform_constant<FusedKernArgs>(kernargs);
    const DevConst& K = uniform_constant<DevConst>(F.Kp);
    const int b = __builtin_amdgcn_readfirstlane(b_in);
    LaneProblem<double, 1> Q = Q_in;
    double x[1][3] = {{x_in[0][0], x_in[0][1], x_in[0][2]}};
    optimize_loaded<double, 32, 1, false, false, 3, true>(F.A, K, K, b, Q, x);
}
#elif VIGO_FUSED_JOIN == 0
__device__ __noinline__ void optimize_solo(const SolveArgs& A, const DevConst* Kp, const int b, LaneProblem<double, 1>& Q, double (&x)[1][3]) {
    optimize_loaded<double, 32, 1, false, false, 3, true>(A, *Kp, *Kp, b, Q, x);
}
#endif
template <int WPS>   // (a template: emitted by the one part of this file that launches it)
__global__ void __launch_bounds__(kWave, WPS) k_optimize_fused(SolveArgs A, const DevConst* __restrict__ Kp) {
    const DevConst& K = *Kp;
    const HotConst KL(K);
    const int lane = threadIdx.x;
    const int grp = lane / 32;
    int b = blockIdx.x;
    if (A.active_idx) {                       // vigo_rebound_rounds: the compacted active set
        if (b >= *A.active_count) return;
        b = A.active_idx[b];
    } else if (b >= A.B) {
        return;
    }
    LaneProblem<double, 1> Q;
    load_problem<double, 32, 1>(A, K, b, lane % 32, Q);
    double x[1][3];
    load_points<double, 1>(A, b, Q, x);
    set_level<double, 32, 1>(K, Q, x);
    if (__builtin_amdgcn_readfirstlane((int)Q.level)) {
        x[0][0] = grp ? x[0][1] : x[0][0];
        axis_guides(Q, grp);
        optimize_loaded<double, 32, 1, false, false, 1, false>(A, K, KL, b, Q, x);
    } else {
        if (grp) return;
#if VIGO_FUSED_JOIN == 1
        optimize_loaded<double, 32, 1, false, false, 3, true>(A, K, K, b, Q, x);
#else
        // (copies: what the call takes the address of lives in memory, and the axis path's A, Q and x must not)
#if VIGO_FUSED_JOIN == 0
        SolveArgs A2 = A;
#endif
        LaneProblem<double, 1> Q2 = Q;
        double x2[1][3] = {{x[0][0], x[0][1], x[0][2]}};
#if VIGO_FUSED_JOIN == 2
        optimize_solo((const void*)__builtin_amdgcn_kernarg_segment_ptr(), b, Q2, x2);
#else
        optimize_solo(A2, Kp, b, Q2, x2);
#endif
#endif
    }
}

}  // namespace

#ifndef VIGO_SOLVER_PART
#define VIGO_SOLVER_PART 0
#endif

using SolveKernel = void (*)(SolveArgs, const DevConst*);
using MixedSolveKernel = void (*)(MixedSolveArgs, const DevConst*);

#if VIGO_SOLVER_PART == 0
DevConst make_dev_const(const vigo_params_t& P) {
    DevConst K{};
    K.dth = P.dthresh;
    K.da = 3.0 * P.dthresh;
    K.db = -3.0 * pow(P.dthresh, 2);
    K.dc = pow(P.dthresh, 3);
    K.unc_factor = P.uncertain_factor;
    K.hth = 0.2;
    K.ha = 3.0 * K.hth;
    K.hb = -3 * pow(K.hth, 2);
    K.hc = pow(K.hth, 3);
    K.min_h = P.min_height;
    K.max_h = P.max_height;
    K.ts_ctrl = P.ts_ctrl;
    K.ts_inv_sqr = 1 / pow(P.ts_ctrl, 2);
    K.ts = P.ts;
    K.thr_dyn = P.dist_thresh_dynamic;
    K.oa = 3.0 * P.dist_thresh_dynamic;
    K.ob = -3 * pow(P.dist_thresh_dynamic, 2);
    K.oc = pow(P.dist_thresh_dynamic, 3);
    K.pred_num = (int)(P.pred_horizon / P.ts);
    K.plan_in_z = P.plan_in_z;
    K.strict_z = P.strict_z != 0;
    K.w[0] = P.w_distance; K.w[1] = P.w_smoothness; K.w[2] = P.w_feasibility; K.w[3] = P.w_dynamic;
    K.mem_size = P.mem_size;
    K.max_iterations = P.max_iterations;
    K.max_linesearch = P.max_linesearch;
    K.g_epsilon = P.g_epsilon;
    K.min_step = P.min_step;
    K.max_step = P.max_step;
    K.ftol = P.f_dec_coeff;
    K.gtol = P.s_curv_coeff;
    K.xtol = P.xtol;
    return K;
}

int launch_cost_grad(hipStream_t s, const SolveArgs& a, const DevConst&, const DevConst* kd, int precision) {
    if (a.B <= 0) return hipSuccess;
    // rows: fp32, fp64 fast, fp64; columns: the shapes 32 x 1, 64 x 1, 64 x 2, 64 x 4
    static constexpr SolveKernel kernels[3][4] = {
        {&k_cost_grad<float, 32, 1, false>, &k_cost_grad<float, 64, 1, false>, &k_cost_grad<float, 64, 2, false>, &k_cost_grad<float, 64, 4, false>},
        {&k_cost_grad<double, 32, 1, true>, &k_cost_grad<double, 64, 1, true>, &k_cost_grad<double, 64, 2, true>, &k_cost_grad<double, 64, 4, true>},
        {&k_cost_grad<double, 32, 1, false>, &k_cost_grad<double, 64, 1, false>, &k_cost_grad<double, 64, 2, false>, &k_cost_grad<double, 64, 4, false>}};
    const Shape sh = shape_for(a.N);
    const int tpb = kWave / sh.group;
    const SolveKernel kernel = kernels[precision == VIGO_PREC_F32 ? 0 : (precision == VIGO_PREC_F64_FAST ? 1 : 2)]
                                      [sh.ppl == 1 ? sh.group / 64 : sh.ppl / 2 + 1];
    hipLaunchKernelGGL(kernel, dim3((a.B + tpb - 1) / tpb), dim3(kWave), 0, s, a, kd);
    return (int)hipGetLastError();
}
#endif  // VIGO_SOLVER_PART == 0

// This file is compiled TWICE (csrc/Makefile).  VIGO_SOLVER_PART == 1: only the k_optimize instantiations for calls WITH
// an obstacle list, built with machine LICM (their inner obstacle loops want their invariants hoisted: 1.85 vs 1.92 ms on
// config 5a); VIGO_SOLVER_PART == 0: everything else, built without it (-3 % on configs 2 and 4).

// The kernel table, expanded from kOptimizeKeys (vigo_solver_plan.hpp): row I is that key's instantiation in the part
// that builds it, nullptr in the other.
template <int I>
static constexpr SolveKernel optimize_kernel_of() {
    constexpr OptimizeKey k = kOptimizeKeys[I];
    if constexpr (VIGO_SOLVER_PART <= 1 && k.obs == (VIGO_SOLVER_PART == 1)) {
        using T = std::conditional_t<k.precision == VIGO_PREC_F32, float, double>;
        constexpr bool FAST = k.precision == VIGO_PREC_F64_FAST;
        static_assert(sizeof(T) == elem_bytes_of(k.precision) && sizeof(HPair<T, k.d>) == hpair_bytes(sizeof(T), k.d) &&
                          sizeof(YSv<FAST>) == ysv_bytes(FAST), "optimize_lds_bytes computes these sizes by arithmetic");
        return &k_optimize<T, k.group, k.ppl, FAST, k.wps, k.obs, k.d, k.rh>;
    }
    return nullptr;
}
template <class Rows> struct OptimizeKernelTable;
template <int... I> struct OptimizeKernelTable<std::integer_sequence<int, I...>> { static constexpr SolveKernel row[] = {optimize_kernel_of<I>()...}; };
static SolveKernel optimize_kernel(int key) { return OptimizeKernelTable<std::make_integer_sequence<int, kOptimizeKeyCount>>::row[key]; }

// VIGO_SOLVER_PART == 2, a third object: the MIXED instantiations (vigo_*_mixed), one per row of kOptimizeMixedKeys, and
// k_cost_grad's for the same arithmetics and groups.  No existing instantiation is built from different text for them.
#if VIGO_SOLVER_PART == 2
template <int I>
static constexpr MixedSolveKernel optimize_mixed_kernel_of() {
    constexpr OptimizeKey k = kOptimizeMixedKeys[I];
    using T = std::conditional_t<k.precision == VIGO_PREC_F32, float, double>;
    constexpr bool FAST = k.precision == VIGO_PREC_F64_FAST;
    static_assert(sizeof(T) == elem_bytes_of(k.precision) && sizeof(HPair<T, k.d>) == hpair_bytes(sizeof(T), k.d) &&
                      sizeof(YSv<FAST>) == ysv_bytes(FAST), "optimize_lds_bytes computes these sizes by arithmetic");
    return &k_optimize<T, k.group, k.ppl, FAST, k.wps, k.obs, k.d, k.rh, true>;
}
template <class Rows> struct OptimizeMixedKernelTable;
template <int... I> struct OptimizeMixedKernelTable<std::integer_sequence<int, I...>> { static constexpr MixedSolveKernel row[] = {optimize_mixed_kernel_of<I>()...}; };
MixedSolveKernel optimize_mixed_kernel(int key) { return OptimizeMixedKernelTable<std::make_integer_sequence<int, kOptimizeMixedKeyCount>>::row[key]; }
MixedSolveKernel cost_grad_mixed_kernel(int precision, int group) {
    // rows: fp32, fp64 fast, fp64; columns: the shapes 32 x 1, 64 x 1
    static constexpr MixedSolveKernel kernels[3][2] = {
        {&k_cost_grad<float, 32, 1, false, true>, &k_cost_grad<float, 64, 1, false, true>},
        {&k_cost_grad<double, 32, 1, true, true>, &k_cost_grad<double, 64, 1, true, true>},
        {&k_cost_grad<double, 32, 1, false, true>, &k_cost_grad<double, 64, 1, false, true>}};
    return kernels[precision == VIGO_PREC_F32 ? 0 : (precision == VIGO_PREC_F64_FAST ? 1 : 2)][group / 64];
}
#elif VIGO_SOLVER_PART == 1
SolveKernel optimize_kernel_with_obstacles(int key) { return optimize_kernel(key); }
#else
SolveKernel optimize_kernel_with_obstacles(int key);
MixedSolveKernel optimize_mixed_kernel(int key);
MixedSolveKernel cost_grad_mixed_kernel(int precision, int group);
// dev builds only (-DVIGO_EXP_AXIS_SWITCH=1, tools/exp_solver.py): VIGO_EXP_AXIS=0 in the environment, read at every
// launch, keeps the axis-per-lane level kernel out of the dispatch, so that one process times both — never defined
// in the shipped library
#ifndef VIGO_EXP_AXIS_SWITCH
#define VIGO_EXP_AXIS_SWITCH 0
#endif
static inline bool axis_dispatch_on() {
#if VIGO_EXP_AXIS_SWITCH
    const char* e = getenv("VIGO_EXP_AXIS");
    return !(e && e[0] == '0');
#else
    return true;
#endif
}
// the same builds: VIGO_EXP_FUSE=0 keeps the two launches of a plan that fuse_optimize would run as one
static inline bool fused_dispatch_on() {
#if VIGO_EXP_AXIS_SWITCH
    const char* e = getenv("VIGO_EXP_FUSE");
    return !(e && e[0] == '0');
#else
    return true;
#endif
}

// Executes plan_optimize's launches, or (fuse_optimize) the one launch that stands for both.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: the "already raised"
// bits live in the handle (LaunchState, one per handle = per device), never in function statics, so a second device of
// the same process gets its own.
int launch_optimize(hipStream_t s, const SolveArgs& a_in, const DevConst& k, const DevConst* kd, int precision, LaunchState& L) {
    static_assert(kOptimizeKeyCount <= 8 * (int)sizeof(L.lds_attr_set), "one bit per k_optimize instantiation");
    if (a_in.B <= 0) return hipSuccess;
    const OptimizePlan plan = plan_optimize(a_in.N, a_in.B, precision, a_in.obs != nullptr, k.plan_in_z != 0, k.strict_z != 0,
                                            k.mem_size, L.simd_count, axis_dispatch_on());
    if (plan.count < 0) return (int)hipErrorInvalidValue;
    SolveArgs a = a_in;
    if (const FusedLaunch f = fuse_optimize(plan, a_in.N, k.mem_size); f.fuse && fused_dispatch_on()) {
        static_assert(solo_lds_bytes(32, kMaxMem) <= kLdsPerWorkgroup / 8, "two waves of the fused kernel per SIMD");
        a.level_waves_elsewhere = 0;   // (read by neither body of the fused kernel)
        hipLaunchKernelGGL(k_optimize_fused<2>, dim3(f.grid), dim3(kWave), f.lds, s, a, kd);
        return (int)hipGetLastError();
    }
    for (int i = 0; i < plan.count; ++i) {
        const PlannedLaunch& p = plan.launch[i];
        const SolveKernel kernel = kOptimizeKeys[p.key].obs ? optimize_kernel_with_obstacles(p.key) : optimize_kernel(p.key);
        const uint64_t bit = 1ull << p.key;
        if (p.lds > kLdsStaticLimit && !(L.lds_attr_set & bit)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerWorkgroup);
            if (e != hipSuccess) return (int)e;
            L.lds_attr_set |= bit;
        }
        a.level_waves_elsewhere = p.level_waves_elsewhere;
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(kWave), p.lds, s, a, kd);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    }
    return (int)hipSuccess;
}

// The mixed-count entries: a.N is the row stride Ns (7 .. 64, checked by the C ABI), a.n_pts the counts.  ONE launch of
// the general kernel (plan_optimize_mixed); its LDS stays below the static limit, so no attribute is raised.
int launch_cost_grad_mixed(hipStream_t s, const MixedSolveArgs& a, const DevConst* kd, int precision) {
    if (a.B <= 0) return hipSuccess;
    const Shape sh = shape_for(a.N);
    if (sh.ppl != 1 || !a.n_pts) return (int)hipErrorInvalidValue;
    const int tpb = kWave / sh.group;
    hipLaunchKernelGGL(cost_grad_mixed_kernel(precision, sh.group), dim3((a.B + tpb - 1) / tpb), dim3(kWave), 0, s, a, kd);
    return (int)hipGetLastError();
}
int launch_optimize_mixed(hipStream_t s, const MixedSolveArgs& a_in, const DevConst& k, const DevConst* kd, int precision, LaunchState& L) {
    if (a_in.B <= 0) return hipSuccess;
    const OptimizePlan plan = plan_optimize_mixed(a_in.N, a_in.B, precision, a_in.obs != nullptr, k.mem_size, L.simd_count);
    if (plan.count != 1 || !a_in.n_pts) return (int)hipErrorInvalidValue;
    const PlannedLaunch& p = plan.launch[0];
    MixedSolveArgs a = a_in;
    a.level_waves_elsewhere = p.level_waves_elsewhere;
    hipLaunchKernelGGL(optimize_mixed_kernel(p.key), dim3(p.grid), dim3(kWave), p.lds, s, a, kd);
    return (int)hipGetLastError();
}
#endif  // VIGO_SOLVER_PART

}  // namespace vigo
