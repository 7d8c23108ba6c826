"""numpy statement of the min-snap QP of polyTrajSolver (PS.cpp:241-846) used by the tests: the
matrices in normalised segment time, polynomial evaluation, and an algorithm-independent optimality
check (KKT conditions) for a candidate solution."""
import math

import numpy as np


def minsnap_matrices(wp, deg, diff, cont, vel, conds=None):
    """numpy statement of the QP (normalised time) for the equality-constrained case.  conds [4][3]: right-hand
    sides of the endpoint rows -- initial velocity, final velocity, initial acceleration, final acceleration, as
    derivatives in normalised segment time (PS.cpp, vigo_minsnap); None = zeros"""
    cd = np.zeros((4, 3)) if conds is None else np.asarray(conds, dtype=np.float64).reshape(4, 3)
    K = len(wp) - 1
    D = deg + 1
    T = np.concatenate([[0], np.cumsum(np.linalg.norm(np.diff(wp, axis=0), axis=1) / vel)])
    n = K * D
    P = np.zeros((n, n))
    for s in range(K):
        for i in range(diff, D):
            for j in range(diff, D):
                f = 1.0
                for d in range(diff):
                    f *= (i - d) * (j - d)
                P[s * D + i, s * D + j] = f / (i + j - 2 * diff + 1)

    def dv(d, order, t):
        if d < order:
            return 0.0
        f = 1.0
        for k in range(order):
            f *= d - k
        return f * t ** (d - order)

    rows, rhs = [], []

    def row(entries, b):
        r = np.zeros(n)
        for c, v in entries:
            r[c] += v
        rows.append(r)
        rhs.append(b)

    last = (K - 1) * D
    row([(d, dv(d, 0, 0.0)) for d in range(D)], wp[0])
    row([(last + d, dv(d, 0, 1.0)) for d in range(D)], wp[-1])
    for i in range(K - 1):
        row([(i * D + d, dv(d, 0, 1.0)) for d in range(D)], wp[i + 1])
    for i in range(K - 1):
        row([(i * D + d, dv(d, 0, 1.0)) for d in range(D)] + [((i + 1) * D + d, -dv(d, 0, 0.0)) for d in range(D)], np.zeros(3))
    for order in (1, 2):
        row([(d, dv(d, order, 0.0)) for d in range(D)], cd[2 * order - 2])
        row([(last + d, dv(d, order, 1.0)) for d in range(D)], cd[2 * order - 1])
        for i in range(K - 1):
            dl, dr = T[i + 1] - T[i], T[i + 2] - T[i + 1]
            row([(i * D + d, dv(d, order, 1.0) * dr ** order) for d in range(D)] +
                [((i + 1) * D + d, -dv(d, order, 0.0) * dl ** order) for d in range(D)], np.zeros(3))
    for order in range(3, cont + 1):
        for i in range(K - 1):
            dl, dr = T[i + 1] - T[i], T[i + 2] - T[i + 1]
            row([(i * D + d, dv(d, order, 1.0) * dr ** order) for d in range(D)] +
                [((i + 1) * D + d, -dv(d, order, 0.0) * dl ** order) for d in range(D)], np.zeros(3))
    return P, np.array(rows), np.array(rhs), T


def closed_form(P, A, b):
    """the equality-constrained optimum per axis: least-squares solution of the KKT system, [3, n].  The rows of A are
    scaled to unit infinity norm and P to a unit largest entry first (same minimiser): the continuity rows carry
    dt^order factors, up to ~1e8 at long segments and high continuity degree, and P's entries reach ~1e5, which the
    unscaled system loses to rounding (lstsq then misses waypoints by up to 1e-3 at continuity degree 6)"""
    s = np.abs(A).max(axis=1)
    A, b = A / s[:, None], b / s[:, None]
    P = P / np.abs(P).max()
    n, m = P.shape[0], A.shape[0]
    KKT = np.block([[P, A.T], [A, np.zeros((m, m))]])
    rhs = np.concatenate([np.zeros((n, 3)), b], axis=0)
    return np.linalg.lstsq(KKT, rhs, rcond=None)[0][:n].T


def assert_matches_closed_form(c, wp, diff, cont, vel, conds=None, deg=7, n_eval=25):
    """coefficients c [3, K*(deg+1)] in un-normalised local time (host layout) against the closed form: equality rows
    1e-10 relative to each row's own scale (continuity rows carry dt^order factors), objective 1e-7, trajectory 1e-6"""
    P, A, b, Tk = minsnap_matrices(wp, deg, diff, cont, vel, conds)
    D = deg + 1
    K = len(wp) - 1
    sol = closed_form(P, A, b)
    scale = np.concatenate([(Tk[s + 1] - Tk[s]) ** np.arange(D) for s in range(K)])
    ts = np.linspace(0, Tk[-1], n_eval)
    seg = np.clip(np.searchsorted(Tk, ts, side="right") - 1, 0, K - 1)
    lt = ts - Tk[seg]
    for a in range(3):
        x = c[a] * scale
        res = (np.abs(A @ x - b[:, a]) / np.abs(A).max(axis=1)).max()
        assert res < 1e-10, (a, res)
        obj, ref = x @ P @ x, sol[a] @ P @ sol[a]
        assert abs(obj - ref) <= 1e-7 * max(1.0, ref), (a, obj, ref)
        for i in range(n_eval):
            s = seg[i]
            pk = (sol[a, s * D:(s + 1) * D] / (Tk[s + 1] - Tk[s]) ** np.arange(D)) @ (lt[i] ** np.arange(D))
            got = c[a, s * D:(s + 1) * D] @ (lt[i] ** np.arange(D))
            assert abs(got - pk) < 1e-6 * max(1.0, abs(pk)), (a, ts[i], got, pk)
    return Tk


def evaluate(coeffs, knots, t, deg=7):
    i = min(np.searchsorted(knots, t, side="right") - 1, len(knots) - 2)
    i = max(i, 0)
    lt = t - knots[i]
    c = coeffs[:, i * (deg + 1):(i + 1) * (deg + 1)]
    return c @ (lt ** np.arange(deg + 1))



def corridor_rows(wp, T, corridor, cres, deg=7):
    """PS.cpp:985-1012 + :565-576, :823-837: (row, centre[3], radius) per box, rows in normalised time"""
    D = deg + 1
    K = len(wp) - 1
    rows, cen, rad = [], [], []
    for i in range(K):
        if corridor[i] == 0.0:
            continue
        num = int(np.ceil((T[i + 1] - T[i]) * cres))
        dt = 1.0 / num
        t = 0.0
        while t <= 1.0:
            r = np.zeros(K * D)
            r[i * D:(i + 1) * D] = [math.pow(t, d) for d in range(D)]   # libm's pow, as PS.cpp:570: numpy's array power
            #                                                              differs from it in the last bit at some t
            rows.append(r)
            cen.append(wp[i] + (wp[i + 1] - wp[i]) * t)
            rad.append(corridor[i])
            t += dt
    return np.array(rows).reshape(-1, K * D), np.array(cen).reshape(-1, 3), np.array(rad)


def kkt_violation(P, Aeq, beq, C, lo, hi, x, active_tol=1e-7):
    """max violation of the KKT conditions of  min 1/2 x'Px  s.t.  Aeq x = beq, lo <= C x <= hi  at x:
    (primal infeasibility, stationarity residual with sign-feasible multipliers on the active boxes).
    Algorithm independent: multipliers are found by non-negative least squares on the active set."""
    from scipy.optimize import nnls
    prim = (np.abs(Aeq @ x - beq) / np.abs(Aeq).max(axis=1)).max()   # rows carry dt^order factors
    if len(C):
        cx = C @ x
        prim = max(prim, (lo - cx).max(), (cx - hi).max())
        act_lo = np.where(np.abs(cx - lo) <= active_tol)[0]
        act_hi = np.where(np.abs(cx - hi) <= active_tol)[0]
    else:
        act_lo = act_hi = np.array([], dtype=int)
    # stationarity: P x + Aeq' nu - C_lo' mu_lo + C_hi' mu_hi = 0, mu >= 0; nu free -> split nu = nu+ - nu-
    cols = [Aeq.T, -Aeq.T]
    if len(act_lo):
        cols.append(-C[act_lo].T)
    if len(act_hi):
        cols.append(C[act_hi].T)
    G = np.concatenate(cols, axis=1)
    scale = max(1.0, np.abs(P @ x).max())
    _, resid = nnls(G, -(P @ x), maxiter=50 * G.shape[1])
    return prim, resid / scale


def eq_kkt_violation(P, Aeq, beq, x):
    """the KKT conditions of  min 1/2 x'Px  s.t.  Aeq x = beq  at x, for any minimiser, unique or not: (primal
    infeasibility relative to each row's scale, reduced gradient Z'Px relative to max|P| max|x|) with Z an orthonormal
    basis of null(Aeq) from the SVD of the row-scaled matrix.  Unlike kkt_violation this needs no multipliers, which
    the dt^order factors of the continuity rows make ill-determined at high continuity degree, and it scales the
    gradient by what rounding leaves of it: at differential degree 5..7 the optimum's |Px| is often 1e-13 of
    |P||x|, so a solution exact to 1e-12 still shows a gradient of 1e-6 relative to |Px|"""
    s = np.abs(Aeq).max(axis=1)
    prim = (np.abs(Aeq @ x - beq) / s).max()
    _, sv, Vt = np.linalg.svd(Aeq / s[:, None])
    rank = int((sv > sv[0] * 1e-13).sum())
    Z = Vt[rank:].T
    g = P @ x
    return prim, np.abs(Z.T @ g).max(initial=0.0) / max(np.abs(P).max() * np.abs(x).max(), 1e-300)
