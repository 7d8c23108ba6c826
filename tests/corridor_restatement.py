"""k_corridor's per-segment arithmetic and routing restated in numpy (csrc/vigo_corridor_core.hpp: the prologue of the
kernel — Tu, E, base, lipd, the lattice-count range and its dividing line — and the block-uniform predicates that choose
a route, the certificate's key test and the float filter).  Plain numpy, no oracle, no GPU: shared by
tests/corridor_cases.py (which scales segments to the routing thresholds), tests/test_corridor_certificates.py,
tests/test_corridor_cases.py, tests/test_gpu_corridor_cases.py and tools/fuzz_corridor.py."""
import numpy as np

U40 = 1.0 + 2.0 ** -40


def bernstein_abs_max_of_derivative(c, Tu):
    deg = len(c) - 1
    best = 0.0
    for i in range(deg):
        bi, ratio, pw = c[1], 1.0, 1.0
        for k in range(1, i + 1):
            ratio *= (i - k + 1) / (deg - k)
            pw *= Tu
            bi += ratio * ((k + 1) * c[k + 1]) * pw
        best = max(best, abs(bi))
    return best


def axis_constants(c, n, dT, box_a, map_res, traj=None):
    """One axis of k_corridor's prologue (the thread `tid < 3` block), operation for operation: Tu, E, base, lipd, the
    range [nlo, nhi] of the lattice count with its dividing line thr, and the two bits of s_span_ok (`ok`: span
    certificates, `thr_ok`: counts by compare).  traj = (kb, ke): trajectory mode — Tu from the segment's knots and the
    drift of the subtracted clock fl(t - kb)."""
    deg = len(c) - 1
    if traj is None:
        Tu = (n - 1) * dT * (1.0 + 2.0 ** -20) if n > 0 else 0.0
    else:
        kb, ke = traj
        Tu = (ke - kb) * (1.0 + 2.0 ** -20)
    Tm = abs(Tu)
    A = A1 = 0.0
    pw = 1.0
    for d in range(deg + 1):
        A += abs(c[d]) * pw
        if d < deg:
            A1 += (d + 1) * abs(c[d + 1]) * pw
        pw *= Tm
    E = 2.0 ** -46 * A + 2.0 ** -1000
    L = (bernstein_abs_max_of_derivative(c, Tu) if deg > 0 else 0.0) + 2.0 ** -40 * A1
    if traj is None:
        drift = n * 2.0 ** -52 * (Tm + abs(dT))
    else:
        drift = (2.0 * Tm + n * (abs(traj[1]) * (1.0 + 2.0 ** -20) + abs(dT))) * 2.0 ** -52
    base = (2.0 * E + L * drift) * U40
    lipd = L * abs(dT) * U40
    h = box_a / 2
    Mx = A * (1.0 + 2.0 ** -20) + abs(h)
    dl = 2.0 ** -50 * (Mx + abs(h))
    ql, qh = (box_a - dl) / map_res, (box_a + dl) / map_res
    ql -= abs(ql) * 2.0 ** -50
    qh += abs(qh) * 2.0 ** -50
    ok = bool(ql > -1.0 and qh < 4.0 and base < 1e300 and lipd < 1e300)          # false for NaN
    # (the kernel zeroes the range when `ok` fails; the range and its dividing line are stated for any finite quotient,
    # boxes of more than 3 cells included: the counts obligation of the test below does not depend on kAxisMax)
    finite = bool(abs(ql) < 1e9 and abs(qh) < 1e9)
    nlo, nhi = (int(ql), int(qh)) if finite else (0, 0)
    thr, thr_ok = -1.0, finite and nhi - nlo <= 1
    if thr_ok and nhi != nlo:
        cnt = lambda d: int(d / map_res)
        cc = nhi * map_res
        guard = 0
        while guard < 8 and cnt(float(np.nextafter(cc, -np.inf))) >= nhi:
            cc = float(np.nextafter(cc, -np.inf))
            guard += 1
        while guard < 16 and cnt(cc) < nhi:
            cc = float(np.nextafter(cc, np.inf))
            guard += 1
        thr_ok = cnt(cc) >= nhi > cnt(float(np.nextafter(cc, -np.inf)))
        thr = cc
    return dict(Tu=Tu, E=E, base=base, lipd=lipd, nlo=nlo, nhi=nhi, thr=thr, ok=ok, thr_ok=bool(ok and thr_ok), thr_search=bool(thr_ok))


def segment_constants(c, n, dT, box_a, map_res):
    """per axis: E, base, lipd, nlo, nhi, thr — the arithmetic of k_corridor's prologue"""
    k = axis_constants(c, n, dT, box_a, map_res)
    assert k["nhi"] == k["nlo"] or k["thr_search"]          # the search for the dividing line succeeded
    return k["Tu"], k["E"], k["base"], k["lipd"], k["nlo"], k["nhi"], k["thr"]


def fast_form(c, t):
    x, pw = 0.0, 1.0
    for d in range(len(c)):
        x += c[d] * pw
        pw *= t
    return x


def keys_of(f, h, i, map_res, rf):
    """lattice point i of an axis from the pose's float: (float)(f - h + i * map_res), floor(rf * q) (vectorised)"""
    q = (f.astype(np.float64) - h + i * map_res).astype(np.float32)
    return q, np.floor(rf * q.astype(np.float64)).astype(np.int64)


# ---- k_corridor's routing, restated (block-uniform predicates of the kernel; tests/test_corridor_cases.py is the census) ----
K_PARALLEL_MAX = 512                                             # kParallelMax: above it, certified spans
K_QUEUE_CAP = 512                                                # kQueueCap
TILE_WORDS_CAP = (((160 * 1024) // 4 - 22 * 1024) & ~255) // 4   # launch_corridor_check2 / launch_traj_corridor


def fast_form_vec(c, t):
    """fast_form on an array of clock values (numpy rounds each operation once, like the kernel under -ffp-contract=off)"""
    t = np.asarray(t, dtype=np.float64)
    x, pw = np.zeros_like(t), np.ones_like(t)
    for d in range(len(c)):
        x = x + c[d] * pw
        pw = pw * t
    return x


def accumulated_clock(dT, n):
    """t_0 .. t_{n-1} of the literal loop `t += delT` (np.cumsum adds left to right, one rounding per step)"""
    steps = np.full(max(n, 1), dT, dtype=np.float64)
    steps[0] = 0.0
    return np.cumsum(steps)[:n]


def tile_words(coeffs, Tu, n, box, map_res, grid):
    """words of the LDS tile k_corridor sizes from the Bernstein hull of the positions over [0, Tu]; grid = (dims, origin, res)"""
    dims, origin, res = grid
    if n <= 0:
        return 0
    rf = 1.0 / res
    ext = []
    with np.errstate(all="ignore"):
        for a in range(3):
            c = [float(x) for x in coeffs[a]]
            deg = len(c) - 1
            lo = hi = c[0]
            for i in range(1, deg + 1):
                bi, ratio, pw = c[0], 1.0, 1.0
                for k in range(1, i + 1):
                    ratio *= (i - k + 1) / (deg - k + 1)
                    pw *= Tu
                    bi += ratio * c[k] * pw
                lo, hi = float(np.fmin(lo, bi)), float(np.fmax(hi, bi))
            if not lo <= hi:
                if a == 0:
                    return 0                                     # `any` is false: no tile, every lookup in the planes
                fmin_, fmax_ = np.float32(np.nan), np.float32(np.nan)
            else:
                pad = 1e-6 * (1.0 + max(abs(lo), abs(hi)))
                fmin_ = np.float32(np.float32(lo - pad) - np.float32(1e-6))
                fmax_ = np.float32(np.float32(hi + pad) + np.float32(1e-6))
            key0 = int(np.floor(origin[a] / res + 0.5))
            l = np.floor(rf * (float(fmin_) - box[a] / 2)) - key0 - 1
            h = np.floor(rf * (float(fmax_) + box[a] / 2 + map_res)) - key0 + 1
            l, h = float(np.fmax(l, 0.0)), float(np.fmin(h, dims[a] - 1.0))
            if not h >= l:
                return 0
            ext.append((int(l), int(h)))
    tx, ty = ext[0][1] - ext[0][0] + 1, ext[1][1] - ext[1][0] + 1
    tw = (ext[2][1] >> 5) - (ext[2][0] >> 5) + 1
    return tx * ty * tw


def segment_route(coeffs, n, dT, box, map_res, grid, traj=None, table=None):
    """Where k_corridor sends one segment (or, with traj = (kb, ke), one run of a trajectory): the predicates `table`,
    `counts`, `n > kParallelMax`, S1 from lipmax against a quarter voxel and the tile against its cap, in the kernel's
    order.  -> dict(route, S1, in_lds, words, K = the three axis_constants, nlo_ne_nhi = axes whose count can vary).
    route: 'empty' | 'pass1:clock' | 'pass1:box' | 'pass1:nonfinite' | 'pass1:speed' | 'lane' | 'span64' | 'span32' |
    'span16' (+ '+L2' when the tile does not fit the LDS).  table: trajectory mode passes its trajectory's."""
    dims, origin, res = grid
    with np.errstate(all="ignore"):
        K = [axis_constants([float(x) for x in coeffs[a]], n, dT, box[a], map_res, traj) for a in range(3)]
        if table is None:
            # build_clock_table: a normal clock (d in [2^-1000, 1e300), t below 1e300) of at most kClockCap = 128 pieces;
            # at most 4 pieces per binade crossed, and a clock of n <= 2^24 steps crosses at most 25
            table = n > 0 and 2.0 ** -1000 <= dT < 1e300 and (n - 1) * dT < 1e300
        counts = all(k["thr_ok"] for k in K)
        lipmax = float(np.fmax(K[0]["lipd"], np.fmax(K[1]["lipd"], K[2]["lipd"])))
        cell = 0.25 / (1.0 / res)
        S1 = 0
        if K_PARALLEL_MAX < n <= (1 << 24):
            S1 = 64 if lipmax * 32.0 <= cell else 32 if lipmax * 16.0 <= cell else 16 if lipmax * 8.0 <= cell else 0
        words = tile_words(coeffs, K[0]["Tu"], n, box, map_res, grid)
    in_lds = 0 < words <= TILE_WORDS_CAP
    if n <= 0:
        route = "empty"
    elif not table:
        route = "pass1:clock"
    elif not counts:
        # a box of more than 3 map cells on some axis fails the count range whatever the positions are; anything else that
        # fails it is the size of the coefficients (NaN, infinity, or positions so large that the range opens up)
        nominal = all(axis_constants([0.0], 1, 1.0, box[a], map_res)["thr_ok"] for a in range(3))
        route = "pass1:nonfinite" if nominal else "pass1:box"
    elif n <= K_PARALLEL_MAX:
        route = "lane"
    elif S1 == 0:
        route = "pass1:speed"
    else:
        route = f"span{S1}"
    if route in ("lane", "span64", "span32", "span16") and not in_lds:
        route += "+L2"
    return dict(route=route, S1=S1 if route.startswith("span") else 0, in_lds=in_lds, words=words, K=K, lipmax=lipmax, cell=cell,
                nlo_ne_nhi=sum(k["nhi"] != k["nlo"] for k in K) if counts else 0)


def _span_fails(coeffs, K, ts, hs, box, map_res, grid, bounds):
    """certify_span() == 0 for pieces centred on clock values ts with half lengths hs — the part of the certificate that does
    not look at voxels: it fails unless every lattice point keeps its key (`constant`) or some point is surely outside."""
    dims, origin, res = grid
    rf = 1.0 / res
    bmin, bmax = bounds
    constant = np.ones(len(ts), bool)
    out = np.zeros(len(ts), bool)
    finite = np.ones(len(ts), bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            p = fast_form_vec([float(x) for x in coeffs[a]], ts)
            R = (K[a]["base"] + K[a]["lipd"] * hs) * U40
            flo, fhi = (p - R).astype(np.float32), (p + R).astype(np.float32)
            finite &= (np.abs(flo) <= np.float32(3.402823466e38)) & (np.abs(fhi) <= np.float32(3.402823466e38))
            h = box[a] / 2
            key0 = int(np.floor(origin[a] / res + 0.5))
            for i in range(K[a]["nhi"] + 1):
                q0, k0 = keys_of(flo, h, i, map_res, rf)
                q1, k1 = keys_of(fhi, h, i, map_res, rf)
                k0, k1 = k0 - key0, k1 - key0
                both = (q0 >= bmin[a]) & (q0 <= bmax[a]) & (q1 >= bmin[a]) & (q1 <= bmax[a])
                constant &= both & (k0 == k1) & (k0 >= 0) & (k0 < dims[a])
                if i <= K[a]["nlo"]:
                    out |= (q1 < bmin[a]) | (q0 > bmax[a]) | (both & ((k1 < 0) | (k0 >= dims[a])))
    return np.where(out, ~finite, ~constant)


def per_sample_mask(coeffs, n, dT, S1, K, box, map_res, grid, bounds, tau=None):
    """The samples PASS 0 leaves to its per-sample path when it certifies spans of S1: those whose span, quarter and
    sixteenth (as far as the kernel cuts: 64/16/4, 32/8, 16/4) all fail the certificate.  A lower bound of the device's
    set: a full item queue marks pieces early, and pieces whose verdict hangs on the lattice counts (s_fbits) pass
    through the filter too.  tau: the run's local clock values in trajectory mode (centres are samples there)."""
    mask = np.zeros(n, bool)
    k0 = np.arange(0, n, S1)
    ln = np.minimum(S1, n - k0)
    for phase in range(3):
        if len(k0) == 0:
            break
        child = (S1 >> 2) >> (2 * phase)
        c = k0 + (ln >> 1)
        hs = np.maximum(c - k0, k0 + ln - 1 - c).astype(np.float64)
        ts = tau[c] if tau is not None else np.minimum(np.maximum(c * dT, 0.0), K[0]["Tu"])
        fails = _span_fails(coeffs, K, ts, hs, box, map_res, grid, bounds)
        nk, nl = [], []
        for kk, ll in zip(k0[fails], ln[fails]):
            if phase == 2 or child < 2 or ll <= child:
                mask[kk:kk + ll] = True
                continue
            for o in range(0, ll, child):
                l = min(child, ll - o)
                if l > 2:
                    nk.append(kk + o)
                    nl.append(l)
                else:
                    mask[kk + o:kk + o + l] = True
        k0, ln = np.array(nk, dtype=np.int64), np.array(nl, dtype=np.int64)
    return mask


def filter_rejects(coeffs, K, t):
    """(float)(fast - E) != (float)(fast + E) on some axis, per clock value: the samples sample_f32_fast() hands to the
    exact-power chain (true for NaN, as in the kernel).  Also the three certified floats."""
    rej = np.zeros(len(t), bool)
    f = np.zeros((len(t), 3), np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            p = fast_form_vec([float(x) for x in coeffs[a]], t)
            lo, hi = (p - K[a]["E"]).astype(np.float32), (p + K[a]["E"]).astype(np.float32)
            rej |= lo != hi
            f[:, a] = lo
    return rej, f
