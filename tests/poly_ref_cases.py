"""Named, seeded cases for the compiled reference's polynomial side (oracle/_ref/libref_poly.so: polyTrajSolver.cpp,
polyTrajOccMap.cpp, piecewiseLinearTraj.cpp as they are), the certified QP solutions its stand-in OSQP hands back, and the
runners that turn a case into plain arrays.  tests/golden/make_poly_golden.py stores what the runners return in
tests/golden/poly_ref.npz; tests/test_oracle_ref_poly.py runs them again where the library is built and holds this
project's restatements, oracle and host facades to the stored arrays; tests/test_gpu_poly_reference_golden.py holds the
kernels to them.

WHERE THE SOLUTION COMES FROM.  The stand-in solver does not optimise: it asks `QpHook` below for the minimiser of the
QP the reference built,  min 1/2 x'Px  s.t.  l <= Ax <= u.  certify() answers in three steps:
  1. a guess of the active set (a float64 working-set iteration; nothing rests on it);
  2. the equality-constrained problem on [rows with l == u; active rows] as one KKT system, solved to 50 digits in mpmath
     (float64 LU as preconditioner, residuals and corrections in mpmath until the residual is below 1e-45 of the
     right-hand side), rows scaled by the power of two next to their largest entry as minsnap_ref.closed_form scales;
  3. acceptance only if every multiplier of an active row has the right sign and is not zero, and every inactive row is
     strictly inside its bounds.  Anything else (guess wrong, dependent active rows, zero multiplier, singular KKT matrix:
     minimiser not unique) drops the case by name.
A solution accepted this way satisfies the KKT conditions of the reference's own matrices; for a convex QP with a
non-singular KKT matrix that is the unique minimiser, whoever guessed the active set.
Infeasible QPs: a scaled phase-one LP (scipy's HiGHS) gives the largest margin s by which all inequality rows can be met
together with the equality rows; s < -1e-6 is infeasible (the hook returns 1: the reference's solver-error path),
s > 1e-6 feasible, in between the case is dropped."""
import hashlib
import math

import numpy as np

import oracle_lib as ol

DEG = 7
D1 = DEG + 1
DPS = 50
ORIGIN = np.array([-3.0, -3.0, 0.0])
RES = 0.1
PLAN_KEYS = ["polynomial_degree", "differential_degree", "continuity_degree", "desired_velocity", "desired_acceleration",
             "initial_radius", "timeout", "corridor_res", "shrinking_factor", "soft_constraint", "constraint_radius",
             "sample_delta_time", "maximum_iteration_num", "use_pwl_failsafe"]
FACE_MARGIN = 1e-5      # 100 x the 1e-7 position bound of the comparisons: two exact solvers cannot flip a lookup
BOTH = (0.1, 0.037)     # the two sample steps
DROP_CAP = 0.1          # at most one seeded random case in ten may be dropped


class Dropped(Exception):
    """the case cannot be certified (degenerate, not unique, on a voxel face): dropped by name"""


# ---------------------------------------------------------------- the certified minimiser
def _pow2(v):
    return 2.0 ** math.floor(math.log2(v)) if v > 0 else 1.0


def _split(A, l, u):
    zero = ~(A != 0).any(axis=1)
    if (l > u).any() or (zero & ((l > 0) | (u < 0))).any():
        return None
    return np.where((l == u) & ~zero)[0], np.where((l < u) & ~zero)[0]


def _margin(A, l, u, eq, ineq):
    """largest s with  l + s <= Ax <= u - s  on the inequality rows (unit rows) and Ax = l on the equality rows"""
    from scipy.optimize import linprog
    n = A.shape[1]
    sc = np.abs(A).max(axis=1)
    Ai, li, ui = A[ineq] / sc[ineq, None], l[ineq] / sc[ineq], u[ineq] / sc[ineq]
    one = np.ones((len(ineq), 1))
    r = linprog(np.concatenate([np.zeros(n), [-1.0]]), A_ub=np.block([[Ai, one], [-Ai, one]]), b_ub=np.concatenate([ui, -li]),
                A_eq=np.hstack([A[eq] / sc[eq, None], np.zeros((len(eq), 1))]), b_eq=l[eq] / sc[eq],
                bounds=[(None, None)] * n + [(None, 1.0)], method="highs")
    if r.status == 2:
        return -1.0, None
    if r.status != 0:
        raise Dropped(f"phase-one LP: {r.message}")
    return float(r.x[-1]), r.x[:n]


def _guess(P, A, l, u, eq, ineq, x_feas):
    """the active set {row: +1 upper / -1 lower} by the primal active-set method on the null space of the equality rows,
    from the strictly feasible point of the phase-one LP.  float64: a guess, checked afterwards"""
    if not len(ineq):
        return {}
    sc = np.abs(A[eq]).max(axis=1)
    Ae, be = A[eq] / sc[:, None], l[eq] / sc
    _, sv, Vt = np.linalg.svd(Ae)
    rank = int((sv > sv[0] * 1e-12).sum())
    Z = Vt[rank:].T
    xp = np.linalg.lstsq(Ae, be, rcond=None)[0]
    nf = Z.shape[1]
    if nf == 0:
        return {}
    H, g = Z.T @ P @ Z, Z.T @ P @ xp
    H = 0.5 * (H + H.T)
    if np.linalg.eigvalsh(H)[0] <= 1e-12 * np.abs(H).max():
        raise Dropped("reduced Hessian singular: no unique minimiser")
    C = A[ineq]
    G = np.vstack([C @ Z, -C @ Z])
    h = np.concatenate([u[ineq] - C @ xp, -(l[ineq] - C @ xp)])
    y = Z.T @ (x_feas - xp)
    if (G @ y - h).max() > 1e-9:
        raise Dropped("no feasible start")
    hs = np.abs(H).max()
    H, g = H / hs, g / hs
    W, at_min = [], False
    for _ in range(20 * len(h) + 100):
        Gw = G[W]
        k = len(W)
        K = np.block([[H, Gw.T], [Gw, np.zeros((k, k))]])
        sol = np.linalg.lstsq(K, np.concatenate([-(H @ y + g), np.zeros(k)]), rcond=None)[0]
        p, mu = sol[:nf], sol[nf:]
        if at_min or np.abs(p).max() <= 1e-11 * max(1.0, np.abs(y).max()):   # a full step ended on this set's minimiser
            at_min = False
            if k == 0 or mu.min() >= 0:
                m = len(ineq)
                return {int(ineq[r % m]): (1 if r < m else -1) for r in W}
            W.pop(int(np.argmin(mu)))
            continue
        Gp = G @ p
        slack = h - G @ y
        cand = [r for r in range(len(h)) if r not in W and Gp[r] > 1e-14]
        alpha, block = 1.0, -1
        for r in cand:
            a = max(slack[r], 0.0) / Gp[r]
            if a < alpha:
                alpha, block = a, r
        y = y + alpha * p
        at_min = block < 0
        if block >= 0:
            W.append(block)
    raise Dropped("no active set found")


def _kkt_mp(P, Aw, bw):
    """[P Aw'; Aw 0] [x; lam] = [0; bw] to DPS digits: (x, lam) as mpmath vectors"""
    import mpmath
    from scipy.linalg import lu_factor, lu_solve
    n, m = P.shape[0], Aw.shape[0]
    s = np.array([_pow2(v) for v in np.abs(Aw).max(axis=1)])
    ps = _pow2(np.abs(P).max())
    K = np.block([[P / ps, (Aw / s[:, None]).T], [Aw / s[:, None], np.zeros((m, m))]])      # exact scalings
    rhs = np.concatenate([np.zeros(n), bw / s])
    sv = np.linalg.svd(K, compute_uv=False)
    if sv[-1] < 1e-11 * sv[0]:
        raise Dropped(f"KKT matrix singular to {sv[-1] / sv[0]:.1e}: dependent active rows or no unique minimiser")
    lu = lu_factor(K)
    with mpmath.workdps(DPS + 10):
        Km = mpmath.matrix(K.tolist())
        bm = mpmath.matrix(rhs.tolist())
        z = mpmath.matrix(n + m, 1)
        bn = max(abs(v) for v in bm) or mpmath.mpf(1)
        for _ in range(40):
            r = bm - Km * z
            rn = max(abs(v) for v in r)
            if rn <= bn * mpmath.mpf(10) ** (-DPS + 5):
                break
            dz = lu_solve(lu, np.array([float(v / rn) for v in r]))
            z = z + mpmath.matrix(dz.tolist()) * rn
        else:
            raise Dropped("mpmath refinement did not converge")
        x = [z[i] for i in range(n)]
        lam = [z[n + i] * ps / mpmath.mpf(float(s[i])) for i in range(m)]
    return x, lam


def certify(P, A, l, u):
    """('ok', x [n] float64 rounding of the 50-digit minimiser, active {row: side}) or ('infeasible', None, None); Dropped"""
    import mpmath
    sp = _split(A, l, u)
    if sp is None:
        return "infeasible", None, None
    eq, ineq = sp
    x_feas = None
    if len(ineq):
        s, x_feas = _margin(A, l, u, eq, ineq)
        if s < -1e-6:
            return "infeasible", None, None
        if s < 1e-6:
            raise Dropped(f"feasibility margin {s:.2e}")
    W = _guess(P, A, l, u, eq, ineq, x_feas)
    rows = sorted(W)
    Aw = np.vstack([A[eq], A[rows]])
    bw = np.concatenate([l[eq], [u[r] if W[r] > 0 else l[r] for r in rows]])
    x, lam = _kkt_mp(P, Aw, bw)
    with mpmath.workdps(DPS + 10):
        tol = mpmath.mpf(10) ** -9
        lscale = max([abs(v) for v in lam] + [mpmath.mpf(1)])
        for k, r in enumerate(rows):
            if W[r] * lam[len(eq) + k] <= tol * lscale * mpmath.mpf(10) ** -3:
                raise Dropped(f"multiplier of active row {r} is {float(lam[len(eq) + k]):.2e} for side {W[r]}")
        for r in ineq:
            if r in W:
                continue
            ax = sum(mpmath.mpf(float(A[r, j])) * x[j] for j in np.nonzero(A[r])[0])
            sc = mpmath.mpf(float(np.abs(A[r]).max()))
            if not (mpmath.mpf(float(l[r])) + tol * sc < ax < mpmath.mpf(float(u[r])) - tol * sc):
                raise Dropped(f"inactive row {r} is not strictly inside its bounds")
        return "ok", np.array([float(v) for v in x]), W


def digest(P, A, l, u):
    h = hashlib.sha256()
    for a in (P, A, l, u):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        h.update(str(a.shape).encode())
    return h.hexdigest()[:24]


class QpHook:
    """the stand-in OSQP's hook.  cache: {digest: x or None (infeasible)} — certified answers already known (the fixture's,
    when a test runs the library again); force: call numbers (0-based since reset()) that report infeasible whatever the
    QP says; calls: [(digest, 'ok' | 'infeasible' | 'forced')]; dropped: the first reason a QP could not be certified (the
    hook then reports infeasible, and the runner raises Dropped)."""

    def __init__(self, cache=None):
        self.cache = {} if cache is None else cache
        self.fn = ol.QP_HOOK_FN(self._call)
        self.reset()

    def reset(self, force=()):
        self.force, self.calls, self.dropped, self.active = set(force), [], None, []

    def _call(self, n, m, P, q, A, l, u, x_out):
        P, A = np.ctypeslib.as_array(P, (n, n)).copy(), np.ctypeslib.as_array(A, (m, n)).copy()
        l, u = np.ctypeslib.as_array(l, (m,)).copy(), np.ctypeslib.as_array(u, (m,)).copy()
        assert not np.ctypeslib.as_array(q, (n,)).any()
        key = digest(P, A, l, u)
        if len(self.calls) in self.force:
            self.calls.append((key, "forced"))
            return 1
        if key not in self.cache:
            try:
                st, x, W = certify(P, A, l, u)
            except Dropped as e:
                self.dropped = self.dropped or str(e)
                self.calls.append((key, "dropped"))
                return 1
            self.cache[key] = x
        x = self.cache[key]
        self.calls.append((key, "ok" if x is not None else "infeasible"))
        if x is None:
            return 1
        np.ctypeslib.as_array(x_out, (n,))[:] = x
        return 0


# ---------------------------------------------------------------- case lists
def random_path(rng, W):
    wp = np.zeros((W, 3))
    wp[0] = rng.uniform(-5, 5, size=3) * [1, 1, 0.2] + [0, 0, 1]
    for i in range(1, W):
        step = rng.normal(size=3) * [1, 1, 0.15]
        wp[i] = wp[i - 1] + step * rng.uniform(1.0, 3.5) / np.linalg.norm(step)
    return wp


def dropped_last_box(n):
    """updateCorridorParam's t += 1/n passes 1 before its (n+1)-th box"""
    t, k = 0.0, 0
    while t <= 1.0:
        k += 1
        t += 1.0 / n
    return k == n


def clock(delT, k):
    t = 0.0
    for _ in range(k):
        t += delT
    return t


def staircase(counts, vel, cres, z=1.03):
    """axis-aligned legs whose duration x corridor_res is counts[i] - 0.5: ceil() gives counts[i] box spacings"""
    wp = [np.array([0.0, 0.0, z])]
    for i, n in enumerate(counts):
        step = np.zeros(3)
        step[i % 2] = (n - 0.5) / cres * vel
        wp.append(wp[-1] + step)
    return np.array(wp)


def clock_legs(ks, delT=0.1, z=1.03):
    """axis-aligned legs at velocity 1 whose knots are the sample clock's own values after ks[0], ks[0] + ks[1], ...
    steps, where the float arithmetic allows it (the runner counts the hits)"""
    wp, t = [np.array([0.0, 0.0, z])], 0.0
    for i, k in enumerate(ks):
        t2 = clock(delT, sum(ks[:i + 1]))
        step = np.zeros(3)
        step[i % 2] = t2 - t
        wp.append(wp[-1] + step)
        t = t2
    return np.array(wp)


def _solver_case(name, wp, diff=4, cont=4, vel=1.0, conds=None, soft=None, corridor=None, cres=5.0, second=None, force=(),
                 delT=(0.1,)):
    return dict(name=name, wp=np.asarray(wp, np.float64), diff=diff, cont=cont, vel=vel, conds=conds, soft=soft, corridor=corridor,
                cres=cres, second=second, force=tuple(force), delT=tuple(delT))


def solver_cases():
    """[case]: named ones first, then the seeded random ones (name 'rand_*')"""
    out = []
    rng = np.random.default_rng(20240607)
    cd = lambda: rng.normal(0.0, 0.4, size=(4, 3))
    # QP construction: waypoint counts, continuity degree, differential degree, velocity, end conditions
    for W, cont, diff, vel, with_conds in [(2, 2, 4, 1.0, 0), (2, 4, 3, 0.25, 1), (3, 3, 4, 1.0, 1), (3, 6, 4, 2.0, 0),
                                           (4, 4, 4, 1.0, 0), (4, 5, 3, 1.0, 1), (5, 2, 3, 2.0, 1), (5, 4, 4, 0.25, 0),
                                           (5, 6, 4, 1.0, 1), (8, 3, 4, 1.0, 0), (8, 4, 3, 2.0, 1), (8, 5, 4, 1.0, 0),
                                           (11, 3, 4, 1.0, 1), (11, 4, 4, 0.25, 0), (11, 3, 3, 2.0, 0)]:
        out.append(_solver_case(f"qp_W{W}_c{cont}_d{diff}_v{vel}_{'conds' if with_conds else 'zero'}", random_path(rng, W), diff,
                                cont, vel, cd() if with_conds else None,
                                delT=BOTH if W in (2, 3, 5) else (0.1,)))
    out.append(_solver_case("qp_cont1_raised", random_path(rng, 4), cont=1))
    out.append(_solver_case("qp_cont0_raised_corridor", random_path(rng, 3), cont=0, corridor=[2.0, 2.0]))
    # corridors
    zig = np.array([[0.0, 0.0, 1.03], [1.6, 1.1, 1.13], [2.9, -0.4, 0.97], [4.4, 0.9, 1.07], [5.8, -0.2, 1.03]])
    out.append(_solver_case("cor_res5_generous", zig, cont=3, corridor=[3.0] * 4, cres=5.0, delT=BOTH))
    out.append(_solver_case("cor_res8_tight", zig, cont=3, corridor=[0.12] * 4, cres=8.0))
    out.append(_solver_case("cor_res5_tight_conds", zig, cont=4, conds=cd(), corridor=[0.15, 0.2, 0.15, 0.2], cres=5.0))
    out.append(_solver_case("cor_zero_segment", zig, cont=3, corridor=[0.2, 0.0, 0.2, 0.0], cres=5.0, delT=BOTH))
    drop = next(n for n in range(3, 60) if dropped_last_box(n))
    keep = next(n for n in range(drop + 1, 60) if not dropped_last_box(n))
    out.append(_solver_case("cor_dropped_and_kept_last_box", staircase([drop, keep, 3], 1.0, 5.0), cont=3, corridor=[0.4] * 3,
                            cres=5.0))
    out.append(_solver_case("cor_second_round_shrunk", zig, cont=3, corridor=[0.3] * 4, cres=5.0,
                            second=[0.3 * 0.8, 0.3, 0.3 * 0.8, 0.3]))
    out.append(_solver_case("cor_second_round_forced_infeasible", zig, cont=3, corridor=[0.3] * 4, cres=5.0,
                            second=[0.3 * 0.8] * 4, force=(3, 4, 5)))
    out.append(_solver_case("cor_second_round_y_forced_infeasible", zig, cont=3, corridor=[0.3] * 4, cres=5.0,
                            second=[0.3 * 0.8] * 4, force=(4,)))
    # soft waypoint boxes
    out.append(_solver_case("soft_one_radius", zig, cont=3, soft=(1, [0.3])))
    out.append(_solver_case("soft_two_radii", zig, cont=4, soft=(2, [0.3, 0.2])))
    out.append(_solver_case("soft_three_radii", zig, cont=3, soft=(3, [0.3, 0.2, 0.07])))
    # (equal radii on both sides of a soft waypoint make the two boxes at the junction one constraint stated twice:
    # dependent active rows, which certify() refuses; hence the alternating radii)
    out.append(_solver_case("soft_as_makeplan_passes_it", zig, cont=3, soft=(-3, []), corridor=[0.4, 0.5, 0.4, 0.5], cres=5.0))
    # sampling: knots on the sample clock, the clock past the last knot by ulps, the clock ending on the last knot
    out.append(_solver_case("samp_knots_on_the_clock", clock_legs([5, 8, 7]), cont=3, delT=BOTH))
    out.append(_solver_case("samp_clock_ends_on_last_knot", clock_legs([4, 4]), cont=3, delT=BOTH))
    out.append(_solver_case("samp_clock_passes_last_knot_by_ulps", np.array([[0.0, 0.0, 1.03], [0.3, 0.0, 1.03]]), delT=BOTH))
    out.append(_solver_case("samp_last_knot_an_ulp_above_the_clock", np.array([[0.0, 0.0, 1.03], [np.nextafter(clock(0.1, 3), 1.0), 0.0, 1.03]]), delT=BOTH))
    # seeded random: corridors of random tightness, conditions, both resolutions
    for k in range(20):
        W = int(rng.integers(2, 7))
        wp = random_path(rng, W)
        out.append(_solver_case(f"rand_{k:02d}", wp, diff=int(rng.choice([3, 4])), cont=int(rng.choice([3, 4])),
                                vel=float(rng.choice([0.5, 1.0, 2.0])), conds=cd() if k % 2 else None,
                                corridor=list(rng.uniform(0.15, 0.6, size=W - 1)), cres=float(rng.choice([5.0, 8.0]))))
    return out


def pillar_world(seed):
    """tests/test_gpu_occmap_batch.pillar_world: 60 x 60 x 20 voxels of 0.1 m from (-3, -3, 0)"""
    rng = np.random.default_rng(seed)
    vox = np.zeros((60, 60, 20), np.uint8)
    for _ in range(25):
        c = rng.integers(3, 57, size=2)
        s = rng.integers(1, 4, size=2)
        vox[c[0] - s[0]:c[0] + s[0], c[1] - s[1]:c[1] + s[1], :] |= int(rng.choice([1, 3, 3]))
    for _ in range(6):
        c = rng.integers(5, 55, size=3)
        vox[c[0] - 4:c[0] + 4, c[1] - 4:c[1] + 4, max(c[2] % 20 - 4, 0):c[2] % 20 + 4] |= 2
    return vox


def block_world(bits):
    """a pillar of `bits` over x in [-0.9, -0.5), y in [-0.1, 0.3): on the first leg of BLOCK_WP"""
    vox = np.zeros((60, 60, 20), np.uint8)
    vox[21:25, 29:33, :] |= bits
    return vox


def corner_world():
    """one column of inflated and unknown voxels, x in [1.1, 1.2), y in [0.6, 0.7): 0.2 m off BLOCK_WP's second leg, where the
    trajectory of the 0.5 m corridor swings out after the corner; two shrinking rounds pull it clear"""
    vox = np.zeros((60, 60, 20), np.uint8)
    vox[41, 36, :] |= 3
    return vox


BLOCK_WP = np.array([[-2.03, -1.02, 1.03], [0.52, 0.93, 1.07], [2.04, -0.61, 1.03]])
WORLDS = {"empty": lambda: np.zeros((60, 60, 20), np.uint8), "corner": corner_world, "full": lambda: np.full((60, 60, 20), 3, np.uint8), "block3": lambda: block_world(3), "block1": lambda: block_world(1),
          "pillar1": lambda: pillar_world(1), "pillar2": lambda: pillar_world(2), "pillar3": lambda: pillar_world(3)}


def _plan_case(name, world, wp, mode=1, conds=None, **cfg):
    return dict(name=name, world=world, wp=np.asarray(wp, np.float64), mode=mode, conds=conds, cfg={"timeout": 100.0, **cfg})


def plan_cases():
    out = []
    rng = np.random.default_rng(20240608)
    out.append(_plan_case("plan_valid_at_once", "empty", BLOCK_WP, maximum_iteration_num=4))
    out.append(_plan_case("plan_valid_after_shrinking", "corner", BLOCK_WP, maximum_iteration_num=9, shrinking_factor=0.8))
    out.append(_plan_case("plan_inflated_but_known_is_no_collision", "block1", BLOCK_WP, maximum_iteration_num=4))
    out.append(_plan_case("plan_out_of_iterations", "empty", [[-2.03, 0.03, 1.03], [3.52, 0.03, 1.03]], maximum_iteration_num=2,
                          shrinking_factor=0.75))
    out.append(_plan_case("plan_out_of_iterations_pwl", "empty", [[-2.03, 0.03, 1.03], [0.52, 1.43, 1.07], [3.52, 0.03, 1.03]], maximum_iteration_num=2,
                          use_pwl_failsafe=1))
    out.append(_plan_case("plan_valid_with_pwl_configured", "corner", BLOCK_WP, maximum_iteration_num=9, use_pwl_failsafe=1))
    out.append(_plan_case("plan_one_waypoint", "empty", [[0.53, 0.51, 1.03]]))
    out.append(_plan_case("plan_no_corridor_mode", "full", BLOCK_WP, mode=0))      # every sample collides, and nobody looks
    out.append(_plan_case("plan_without_bool", "block3", BLOCK_WP, mode=2, maximum_iteration_num=9))
    out.append(_plan_case("plan_soft_constraint", "block3", [[-2.03, -1.02, 1.03], [-0.52, -0.63, 1.21], [0.51, -0.93, 0.83], [2.04, -0.61, 1.03]],
                          soft_constraint=1, constraint_radius=0.25, maximum_iteration_num=6))
    out.append(_plan_case("plan_waypoint_on_the_edge", "pillar1", [[-2.63, 0.33, 1.03], [0.22, -0.71, 1.11], [2.98, 0.47, 0.93]],
                          maximum_iteration_num=5, shrinking_factor=0.75))
    # a long first leg from rest through a pillar with small boxes: they shrink on that leg, round after round, until no
    # degree-7 polynomial that starts at rest stays within them (Markov's inequality bounds its slope at 0 by 98 radii)
    out.append(_plan_case("plan_infeasible_while_shrinking", "block3", BLOCK_WP, maximum_iteration_num=9, shrinking_factor=0.75,
                          initial_radius=0.3))
    for k in range(30):
        W = int(rng.integers(2, 7))
        p = np.column_stack([np.linspace(-2.63, 2.57, W) * rng.choice([-1, 1]), rng.uniform(-2.6, 2.6, W), rng.uniform(0.4, 1.6, W)])
        if k % 5 == 0:
            p[-1, 0] = 2.98 * np.sign(p[-1, 0])
        conds = rng.uniform(-0.4, 0.4, size=(4, 3)) if k % 3 else None
        out.append(_plan_case(f"rand_plan_{k:02d}", f"pillar{1 + k % 3}", p, mode=int(rng.choice([1, 1, 1, 0, 2])), conds=conds,
                              maximum_iteration_num=int(rng.integers(2, 10)), shrinking_factor=float(rng.choice([0.75, 0.8])),
                              use_pwl_failsafe=int(k % 7 == 0)))
        out[-1]["keep_get_trajectory"] = k % 3 == 0
    return out


def pwl_cases():
    """the shapes of tests/test_pwl_restatement.py: (name, wp [n][4], overload, use_yaw, vel)"""
    rng = np.random.default_rng(20240609)
    out = []
    shapes = {"two_points": np.array([[0.0, 0.0, 1.0, 0.3], [2.0, 1.0, 1.2, -0.4]]),
              "turn_back": np.array([[0.0, 0.0, 1.0, 3.0], [1.0, 0.0, 1.0, -3.0], [0.0, 0.1, 1.0, 0.5]]),
              "repeated_point": np.array([[0.0, 0.0, 1.0, 0.0], [1.0, 1.0, 1.0, 1.0], [1.0, 1.0, 1.0, 2.0], [2.0, 0.0, 1.5, -1.0]]),
              "random5": np.column_stack([rng.uniform(-3, 3, size=(5, 2)), rng.uniform(0.5, 1.5, 5), rng.uniform(-3.1, 3.1, 5)])}
    for nm, wp in shapes.items():
        for overload, use_yaw, vel in [(0, 0, 0.0), (0, 1, 0.0), (1, 0, 2.0), (1, 1, 0.5), (2, 0, 0.0), (3, 1, 1.5)]:
            out.append(dict(name=f"pwl_{nm}_o{overload}_y{use_yaw}", wp=wp, overload=overload, use_yaw=use_yaw, vel=vel))
    return out


# ---------------------------------------------------------------- the fixture's layout
def pack(arrays, meta):
    """{'kind/case/field' | 'world/name' | 'qp/digest': array} -> the npz members: one float64 vector per case (every field
    raveled, one after the other; the integers it holds are small), one for all QP answers, the worlds as they are, and
    'meta' with the index {member: [[field, dtype, shape, offset], ...]}"""
    import json
    out, index, groups = {}, {}, {}
    for key, a in arrays.items():
        if key.startswith("world/"):
            out[key] = a
            continue
        member, field = key.rsplit("/", 1) if not key.startswith("qp/") else ("qp", key[3:])
        groups.setdefault(member, []).append((field, np.asarray(a)))
    for member, fields in groups.items():
        off, parts, idx = 0, [], []
        for field, a in fields:
            idx.append([field, str(a.dtype), list(a.shape), off])
            parts.append(a.astype(np.float64).ravel())
            off += a.size
        out[member] = np.concatenate(parts) if parts else np.zeros(0)
        index[member] = idx
    out["meta"] = np.array(json.dumps({**meta, "index": index}, sort_keys=True))
    return out


class Fixture:
    """tests/golden/poly_ref.npz: case(kind, name) -> {field: array}; qp_cache() -> {digest: x or None}"""

    def __init__(self, path):
        import json
        self.z = np.load(path)
        self.meta = json.loads(str(self.z["meta"]))

    def _member(self, member):
        flat = self.z[member]
        return {f: flat[off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape).astype(dt)
                for f, dt, shape, off in self.meta["index"][member]}

    def case(self, kind, name):
        return self._member(f"{kind}/{name}")

    def world(self, name):
        return self.z[f"world/{name}"]

    def qp_cache(self):
        return {k: (v if v.size else None) for k, v in self._member("qp").items()}


DIGEST_FROM_K = 7       # paths of eight waypoints or more: digests of P and A in the fixture, not the matrices


def matrix_digest(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.frombuffer(hashlib.sha256(str(a.shape).encode() + a.tobytes()).digest(), dtype=np.uint8).copy()


def eq_rows(K, cont):
    """equality rows of the QP: position 2 + 2 (K - 1), velocity and acceleration 2 + (K - 1) each, (K - 1) per higher order"""
    return (2 + 2 * (K - 1)) + 2 * (2 + (K - 1)) + (K - 1) * (cont - 2)


def matrices(c):
    """the reference's (P, A) of a stored solver case.  Stored as they are for the small shapes.  For the large ones the
    fixture holds their digests: they are rebuilt from tests/minsnap_ref.py — equality rows up to snap continuity, the
    boxes in the stored order of the reference's unordered_map, then the rows the reference leaves empty above continuity
    degree 4 — and returned only if the digests agree, i.e. if minsnap_ref states them bit for bit"""
    if "A" in c:
        return c["P"], c["A"]
    from minsnap_ref import corridor_rows, minsnap_matrices
    diff, _, vel, cres = c["in_params"]
    wp, cont = c["in_wp"], int(c["cont_after"])
    K = len(wp) - 1
    P, Aeq, _, T = minsnap_matrices(wp, DEG, int(diff), cont, float(vel), c["in_conds"] if c["in_conds"].size else None)
    rows = [Aeq[:eq_rows(K, min(cont, 4))]]
    if c["in_corridor"].size:
        Cm, _, _ = corridor_rows(wp, T, c["in_corridor"], float(cres))
        at = {(int(np.nonzero(r)[0][0]) // D1, float(r[(int(np.nonzero(r)[0][0]) // D1) * D1 + 1])): r for r in Cm}
        rows.append(np.array([at[(int(s), float(t))] for s, t in zip(c["box_seg"], c["box_t"])]).reshape(-1, K * D1))
    rows.append(np.zeros((max(cont - 4, 0) * (K - 1), K * D1)))
    A = np.vstack(rows)
    assert np.array_equal(matrix_digest(P), c["P_digest"]) and np.array_equal(matrix_digest(A), c["A_digest"]), \
        "tests/minsnap_ref.py does not state the reference's matrices bit for bit"
    return P, A


# ---------------------------------------------------------------- runners
def _P(a):
    return None if a is None else ol._d(np.ascontiguousarray(a, dtype=np.float64))


def pow_mask(knots, delT, n):
    """per sample of getTrajectory's clock: does libm's pow (math.pow: the same libm the compiled reference calls) differ
    from the correctly rounded power for any exponent getPose uses?  (the endpoint, sample n - 1, is not a polynomial)"""
    O = ol.oracle()
    mask = np.zeros(n, dtype=np.uint8)
    t = 0.0
    for j in range(n - 1):
        s = next((i for i in range(len(knots) - 1) if knots[i] <= t <= knots[i + 1]), -1)
        if s >= 0:
            tt = t - knots[s]
            mask[j] = any(math.pow(tt, d) != O.vgo_pow_exact(tt, d) for d in range(D1))
        t += delT
    return mask


def _solver_state(L, s, K, hook, first_call):
    n = K * D1
    out = {}
    kn = np.zeros(K + 1)
    assert L.rps_solver_knots(s, _P(kn), K + 1) == K + 1
    out["knots"] = kn
    sol = np.zeros((3, n))
    for a in range(3):
        assert L.rps_solver_solution(s, a, ol._d(sol[a]), n) == n
    out["sol"] = sol
    log = ol.ref_poly_log(L)[first_call:]
    assert len(log) == 3
    out["P"], out["A"] = log[0]["P"], log[0]["A"]
    assert all(np.array_equal(r["P"], out["P"]) and np.array_equal(r["A"], out["A"]) for r in log)
    out["l"], out["u"] = np.stack([r["l"] for r in log]), np.stack([r["u"] for r in log])
    out["x"] = np.stack([r["x"] for r in log])
    out["tag"] = np.array([r["tag"] for r in log], np.int32)
    out["status"] = np.array([r["status"] for r in log], np.int32)
    cap = 4096
    seg, t, cen = np.zeros(cap, np.int32), np.zeros(cap), np.zeros((cap, 3))
    nb = L.rps_solver_corridor_order(s, ol._i(seg), ol._d(t), ol._d(cen), cap)
    out["box_seg"], out["box_t"], out["box_centre"] = seg[:nb].copy(), t[:nb].copy(), cen[:nb].copy()
    return out


def _sample_state(L, s, kn, delTs):
    out = {}
    cap = 8192
    for d in delTs:
        tr = np.zeros((cap, 4))
        n = L.rps_solver_trajectory(s, float(d), ol._d(tr), cap)
        assert 0 < n <= cap
        out[f"traj_{d}"] = tr[:n].copy()
        out[f"powmask_{d}"] = pow_mask([float(v) for v in kn], float(d), n)
    K = len(kn) - 1
    ts = [0.0] + [float(kn[i]) for i in range(1, K + 1)] + [float(0.5 * (kn[i] + kn[i + 1])) for i in range(K)]
    ts += [float(np.nextafter(kn[i], 0.0)) for i in range(1, K + 1)] + [float(np.nextafter(kn[i], np.inf)) for i in range(1, K)]
    ts = np.array(ts)
    ev = np.zeros((len(ts), 13))
    L.rps_solver_eval(s, len(ts), ol._d(ts), ol._d(ev))
    out["eval_t"], out["eval"] = ts, ev
    return out


def run_solver_case(L, hook, case):
    """-> {field: array}; raises Dropped.  Two rounds when the case has a second corridor: fields of the second round carry
    the suffix '_2'"""
    wp = case["wp"]
    K = len(wp) - 1
    hook.reset(case["force"])
    L.rps_set_hook(hook.fn)
    L.rps_log_clear()
    dup0 = L.rps_duplicate_inserts()
    s = L.rps_solver_create(DEG, case["diff"], case["cont"], case["vel"])
    try:
        L.rps_solver_set_path(s, len(wp), _P(wp))
        out = {"cont_after": np.int32(L.rps_solver_continuity(s))}
        if case["conds"] is not None:
            L.rps_solver_set_conds(s, _P(case["conds"]))
        if case["corridor"] is not None:
            L.rps_solver_set_corridor(s, K, _P(case["corridor"]), case["cres"])
        if case["soft"] is not None:
            L.rps_solver_set_soft(s, case["soft"][0], _P(np.array(list(case["soft"][1]) + [0.0] * 3)))
        out["m"] = np.int32(L.rps_solver_constraints(s))
        rc = L.rps_solver_solve(s)
        if hook.dropped:
            raise Dropped(hook.dropped)
        if rc == ol.REF_POLY_UNDEFINED:
            raise Dropped("solver error before any solution exists: the reference would read an empty xSol_")
        out.update(_solver_state(L, s, K, hook, 0))
        out.update(_sample_state(L, s, out["knots"], case["delT"]))
        if case["second"] is not None:
            L.rps_solver_set_corridor(s, K, _P(case["second"]), case["cres"])
            rc = L.rps_solver_solve(s)
            if hook.dropped:
                raise Dropped(hook.dropped)
            assert rc == 0
            second = _solver_state(L, s, K, hook, 3)
            second.update(_sample_state(L, s, out["knots"], case["delT"][:1]))
            # updateProblem hands OSQP bounds only: the recorded A is the first round's, which is stored once
            out["A_2_same"] = np.int32(np.array_equal(second["A"], out["A"]) and np.array_equal(second["P"], out["P"]))
            out.update({k + "_2": v for k, v in second.items() if k not in ("P", "A")})
        out["dup"] = np.int64(L.rps_duplicate_inserts() - dup0)
        if K >= DIGEST_FROM_K:
            # the large shapes: SHA-256 of the matrices' bytes, not the matrices; matrices() rebuilds them from
            # tests/minsnap_ref.py and accepts them only if these digests agree, which is the bit-for-bit comparison
            out["P_digest"], out["A_digest"] = matrix_digest(out.pop("P")), matrix_digest(out.pop("A"))
        return out
    finally:
        L.rps_solver_destroy(s)


def face_margin(samples):
    """smallest distance of any sample to a voxel face, per axis"""
    g = (np.asarray(samples) - ORIGIN) / RES
    return (np.abs(g - np.round(g)) * RES).min(axis=0) if len(g) else np.full(3, np.inf)


def plan_cfg(case):
    return np.array([float(case["cfg"].get(k, np.nan)) for k in PLAN_KEYS])


def run_plan_case(L, hook, case):
    wp = case["wp"]
    W = len(wp)
    K = max(W - 1, 1)
    vox = np.ascontiguousarray(WORLDS[case["world"]]())
    hook.reset()
    L.rps_set_hook(hook.fn)
    L.rps_log_clear()
    h = L.rps_occ_create(_P(plan_cfg(case)))
    try:
        L.rps_occ_set_map(h, *vox.shape, _P(ORIGIN), RES, ol._u(vox))
        L.rps_occ_set_path(h, W, _P(wp), _P(case["conds"]))
        cap = 8192
        tr, n = np.zeros((cap, 4)), np.zeros(1, np.int32)
        verdict = L.rps_occ_make_plan(h, case["mode"], ol._d(tr), cap, ol._i(n))
        if hook.dropped:
            raise Dropped(hook.dropped)
        if verdict == ol.REF_POLY_UNDEFINED:
            raise Dropped("the first solve fails: the reference would read an empty xSol_")
        assert verdict in (0, 1), verdict
        out = {"verdict": np.int32(verdict), "traj": tr[:n[0]].copy(), "valid": np.int32(L.rps_occ_valid(h)),
               "duration": np.float64(L.rps_occ_duration(h))}
        log = ol.ref_poly_log(L)
        out["solves"] = np.int32(len(log) // 3)
        out["qp_status"] = np.array([r["status"] for r in log], np.int32).reshape(-1, 3)
        out["qp_tag"] = np.array([r["tag"] for r in log], np.int32).reshape(-1, 3)
        sizes = np.zeros((64, K))
        nr = L.rps_occ_rounds(h, K, ol._d(sizes), 64)
        assert nr == out["solves"]
        out["rounds"] = sizes[:nr].copy()
        margins = [face_margin(tr[:n[0], :3])]
        for r in range(nr):
            rt = np.zeros((cap, 3))
            k = L.rps_occ_round_traj(h, r, ol._d(rt), cap)
            assert k > 0
            margins.append(face_margin(rt[:k]))
            if r == nr - 1:
                out["poly_traj"] = rt[:k].copy()
        out["face_margin"] = np.min(margins, axis=0)
        if W > 1 and nr and out["face_margin"].min() < FACE_MARGIN:
            raise Dropped(f"a sample lies {out['face_margin'].min():.1e} from a voxel face")
        if W > 1:
            s = L.rps_occ_solver(h)
            out.update(_solver_state(L, s, W - 1, hook, len(log) - 3))
            for k in ("P", "A", "l", "u", "x", "box_t", "box_centre", "box_seg", "tag", "status"):
                del out[k]                                    # the QP matrices are pinned by the solver cases
            delT = float(case["cfg"].get("sample_delta_time", 0.1))
            seg, ns = np.zeros(64, np.int32), np.zeros(1, np.int32)
            out["check_flag"] = np.int32(L.rps_occ_check(h, len(out["poly_traj"]), _P(out["poly_traj"]), delT, ol._i(seg), 64, ol._i(ns)))
            out["check_seg"] = seg[:ns[0]].copy()
            out["powmask"] = pow_mask([float(v) for v in out["knots"]], delT, len(out["poly_traj"]))
            dur = float(out["duration"])
            gt = np.zeros((cap, 3))
            ng = L.rps_occ_trajectory(h, 0.1, ol._d(gt), cap)
            out["get_trajectory_n"] = np.int32(ng)
            if case.get("keep_get_trajectory", True):
                out["get_trajectory"] = gt[:ng].copy()
            pdur = float(out["knots"][-1])
            ts = np.array([0.0, 0.5 * min(dur, pdur), float(out["knots"][1]), min(dur, pdur), dur, dur + 0.5, dur + 100.0])
            ev = np.zeros((len(ts), 16))
            L.rps_occ_eval(h, len(ts), ol._d(ts), ol._d(ev))
            if dur > pdur:                                     # PWL duration beyond the polynomial's knots: getPos / getVel /
                ev[ts > pdur, 7:] = np.nan                     # getAcc return an uninitialised Vector3d there; not recorded
            out["eval_t"], out["eval"] = ts, ev
            if np.array_equal(out["poly_traj"], out["traj"][:, :3]):
                del out["poly_traj"]                           # stored only where the PWL replaced the list: poly_traj()
        return out
    finally:
        L.rps_occ_destroy(h)


def poly_traj(c):
    """the polynomial's samples of a planner case's last round"""
    return c["poly_traj"] if "poly_traj" in c else c["traj"][:, :3]


def run_pwl_case(L, case, delT=0.1):
    wp = np.ascontiguousarray(case["wp"], dtype=np.float64)
    cap = 4096
    tr, kn, nk, dur = np.zeros((cap, 4)), np.zeros(4 * len(wp)), np.zeros(1, np.int32), np.zeros(1)
    # (makePlan's poses are getPose's; getPose through polyTrajOccMap is recorded by the planner cases with use_pwl_failsafe)
    n = L.rps_pwl(len(wp), ol._d(wp), case["overload"], case["use_yaw"], case["vel"], delT, ol._d(tr), cap, ol._d(kn), ol._i(nk),
                  ol._d(dur), 0, None, None)
    assert 0 < n <= cap
    return {"traj": tr[:n].copy(), "knots": kn[:nk[0]].copy(), "duration": np.float64(dur[0])}
