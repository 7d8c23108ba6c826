"""Workloads and CPU replays shared by the mixed-count tests (tests/test_gpu_mixed_batch.py): per-count batches of
synth.make_bspline_batch padded together by synth.pad_batches, and the replay of vigo_rebound_rounds_mixed — oracle_rounds of
tests/test_gpu_rebound.py restated with the count per trajectory."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from gpu_util import emulation
from trajectory_planner_amd import synth

S_STATUS, S_SOLVE, S_FAIL, S_GSTAT, S_GDYN, S_ROUNDS, S_LBFGS, S_NSEG, S_SEG = 0, 1, 2, 3, 4, 5, 6, 7, 8
STATE_INTS, MAX_SEGS = 8 + 2 * 48, 48
RB_ACTIVE, RB_DONE, RB_NEEDS_HOST = 0, 1, 2
LBFGSERR_INVALID_N = -1021

# (count, trajectories) per source batch, in the order pad_batches deals them out.  Both shape classes of
# vigo_solver_plan.hpp's shape_for; 3 - 5 trajectories per count; an ODD number of source batches, so that the round-robin
# shifts by one every cycle and wavefront partners come in both orders — (7, 32) and (32, 7), (16, 31), (31, 8), ... — and an
# odd B, so that the last wavefront of the <= 32 class holds one trajectory.
PARTS = {32: ((7, 3), (32, 2), (16, 3), (31, 3), (8, 3), (9, 3), (32, 2)),       # B = 19
         64: ((33, 3), (64, 2), (40, 3), (63, 3), (64, 2))}                      # B = 13


def rich_guides(world, b, seed, unknown_share=0.3):
    """the batch with NEW guide lists: 0, 2 or 5 pairs per free control point (the kernels keep two pairs per point in
    registers and read the rest from memory), a pair 0.2 - 0.8 m away in a random horizontal direction, a share of them
    flagged unknown"""
    rng = np.random.default_rng(seed)
    B, N = b.B, b.N
    counts = np.zeros((B, N), dtype=np.int64)
    counts[:, 3:N - 3] = rng.choice([0, 2, 5], p=[0.4, 0.35, 0.25], size=(B, N - 6))
    if counts.max() < 5:
        counts[0, 3] = 5
    goff = np.zeros(B * N + 1, dtype=np.int32)
    goff[1:] = np.cumsum(counts.reshape(-1))
    G = int(goff[-1])
    owner = np.repeat(b.ctrl.reshape(-1, 3), counts.reshape(-1), axis=0)
    ang = rng.uniform(0.0, 2 * np.pi, size=G)
    u = np.stack([np.cos(ang), np.sin(ang), np.zeros(G)], axis=1)
    gpv = np.ascontiguousarray(np.concatenate([owner + rng.uniform(0.2, 0.8, size=(G, 1)) * u, u], axis=1))
    gunk = (rng.random(G) < unknown_share).astype(np.uint8)
    return synth.Batch(b.ctrl, goff, gpv, gunk, b.obs_off, b.obs, b.weights, dict(b.meta))


def calm(b, r):
    """trajectory r of the batch moved into free space for good: a quarter of its horizontal extent, started above the
    map's centre at z = 5 (the boxes of conftest's small_world end below 3.5), level, without guides — its gates pass"""
    c = b.ctrl[r].copy()
    c[:, :2] = 0.25 * (c[:, :2] - c[0, :2])
    c[:, 2] = 5.0
    counts = np.diff(b.guide_off.astype(np.int64))
    keep = np.repeat(np.arange(b.B * b.N) // b.N != r, counts)
    counts[r * b.N:(r + 1) * b.N] = 0
    ctrl = b.ctrl.copy()
    ctrl[r] = c
    goff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return synth.Batch(ctrl, goff, np.ascontiguousarray(b.guide_pv[keep]), b.guide_unk[keep], b.obs_off, b.obs, b.weights, dict(b.meta))


def make_parts(world, cls, seed, n_obs=0, z_jitter=0.0, z_share=0.5, guides="rich", weights=None, start_range=3.5, counts=None,
               calm_first=False):
    """the source batches of one shape class (cls = 32 | 64).  n_obs: obstacles of every trajectory of every SECOND source
    batch (the others have none, so a padded batch mixes both); weights: None, or a function (rng, B) -> [B, 4];
    calm_first: the first trajectory of each batch without obstacles is collision free (calm())"""
    parts = []
    for k, (N, B) in enumerate(counts or PARTS[cls]):
        b = synth.make_bspline_batch(world, B, N, seed + 31 * k + N, start_range=start_range, n_obs=n_obs if k % 2 == 0 else 0,
                                     guide2_prob=0.5, z_jitter=z_jitter, z_share=z_share)
        if calm_first and k % 2 == 1:
            b = calm(b, 0)
        if guides == "rich":
            b = rich_guides(world, b, seed + 7 * k)
        if weights is not None:
            b.weights = weights(np.random.default_rng(seed + k), B)
        parts.append(b)
    return parts


def random_weights(P):
    base = np.array([P.w_distance, P.w_smoothness, P.w_feasibility, P.w_dynamic])
    return lambda rng, B: np.ascontiguousarray(base[None, :] * rng.choice([0.5, 1.0, 2.0, 4.0], size=(B, 4)))


def unread_guide_entries(pb, rebound=False):
    """mask over guide_off [B*Ns+1]: the entries no kernel may read.  The solve and the cost read the lists of the free
    control points 3 .. n - 4: entries 3 .. n - 3 of a row.  The rebound rounds also ask isControlPointRequireNewGuide about
    any control point a collision segment names (rebound=True): entries 0 .. n."""
    B, Ns = pb.ctrl.shape[:2]
    mask = np.ones(B * Ns + 1, dtype=bool)
    for b in range(B):
        n = int(pb.n_pts[b])
        mask[(b * Ns, b * Ns + 3)[not rebound]:b * Ns + (n + 1 if rebound else n - 2)] = False
    return mask


def poisoned(pb, rebound=False):
    """the padded batch with everything beyond a trajectory's own rows spoiled: NaN control points, guide offsets far
    outside the pair list"""
    ctrl = pb.ctrl.copy()
    for b in range(pb.B):
        ctrl[b, pb.n_pts[b]:] = np.nan
    goff = pb.guide_off.copy()
    unread = unread_guide_entries(pb, rebound)
    goff[unread] = np.where(np.arange(goff.size) % 2 == 0, 2 ** 31 - 1, -(2 ** 30))[unread]
    return synth.PaddedBatch(ctrl, goff, pb.guide_pv, pb.guide_unk, pb.obs_off, pb.obs, pb.weights, dict(pb.meta), pb.n_pts)


def uniform_groups(pb):
    """the padded batch split by count: [(rows, synth.Batch of those rows with N = the count)], lists re-based"""
    Ns = pb.ctrl.shape[1]
    out = []
    for n in sorted(set(int(x) for x in pb.n_pts)):
        rows = np.where(pb.n_pts == n)[0]
        counts, pv, unk, obs, ocnt = [], [], [], [], []
        for i in rows:
            off = pb.guide_off[i * Ns:i * Ns + n + 1].astype(np.int64)
            counts.append(np.diff(off))
            pv.append(pb.guide_pv[off[0]:off[-1]])
            unk.append(pb.guide_unk[off[0]:off[-1]])
            if pb.obs is not None:
                obs.append(pb.obs[pb.obs_off[i]:pb.obs_off[i + 1]])
                ocnt.append(len(obs[-1]))
        goff = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int32)
        out.append((rows, synth.Batch(np.ascontiguousarray(pb.ctrl[rows, :n]), goff, np.ascontiguousarray(np.concatenate(pv).reshape(-1, 6)),
                                      np.concatenate(unk).astype(np.uint8),
                                      np.concatenate([[0], np.cumsum(ocnt)]).astype(np.int32) if pb.obs is not None else None,
                                      np.ascontiguousarray(np.concatenate(obs).reshape(-1, 9)) if pb.obs is not None else None,
                                      None if pb.weights is None else np.ascontiguousarray(pb.weights[rows]))))
    return out


def count_ok(n, Ns):
    return 7 <= n <= Ns <= 64 and (n <= 32) == (Ns <= 32)


def initial_state(world, pb, rng, fail_max=3, ncr=0.0, preset=True):
    """vigo_rebound_state_t rows as makePlan's step 1 leaves them (collisionSeg_ = findCollisionSeg of the initial control
    points, an optimize() owed), failCount seeds 0 .. fail_max, and (preset) a few entries already DONE / NEEDS_HOST"""
    B = pb.B
    state = np.zeros((B, STATE_INTS), dtype=np.int32)
    state[:, S_SOLVE] = 1
    state[:, S_FAIL] = rng.integers(0, fail_max + 1, size=B)
    if preset:
        state[1, S_STATUS] = RB_DONE
        state[B // 2, S_STATUS] = RB_NEEDS_HOST
    g, keep = ol.make_grid(world)
    for i in range(B):
        n = int(pb.n_pts[i])
        if not count_ok(n, pb.ctrl.shape[1]):
            continue
        seg = np.zeros(2 * MAX_SEGS, dtype=np.int32)
        state[i, S_NSEG] = ol.oracle().vgo_find_collision_seg(C.byref(g), n, ol._d(np.ascontiguousarray(pb.ctrl[i, :n])), ncr, ol._i(seg), MAX_SEGS)
        state[i, S_SEG:] = seg
    return state


def oracle_rounds_mixed(P, world, pb, weights, state, gate_dt, max_rounds, ncr=0.0):
    """CPU replay of vigo_rebound_rounds_mixed (include/vigo.h): ctrl [B,Ns,3], weights, state after the call.  Every
    trajectory with its own count: the gates and the decision (vgo_rebound_decide), and the solve in the oracle's
    emulation of the lane layout of that count."""
    O = ol.oracle()
    g, keep = ol.make_grid(world)
    B, Ns = pb.ctrl.shape[:2]
    ctrl = np.array(pb.ctrl, dtype=np.float64, copy=True)
    w = np.array(weights, dtype=np.float64, copy=True)
    st = np.array(state, dtype=np.int32, copy=True)
    # a count outside the contract: the device cannot represent this planner — handed to the host, no batch-wide wait
    bad = np.array([not count_ok(int(n), Ns) for n in pb.n_pts])
    hand = bad & (st[:, S_STATUS] == RB_ACTIVE)
    st[hand, S_STATUS] = RB_NEEDS_HOST
    st[hand, S_LBFGS] = LBFGSERR_INVALID_N
    good = synth.PaddedBatch(np.where(bad[:, None, None], 0.0, pb.ctrl), pb.guide_off, pb.guide_pv, pb.guide_unk, pb.obs_off, pb.obs,
                             None, {}, np.where(bad, 7, pb.n_pts).astype(np.int32))
    groups = uniform_groups(good)

    def solve(idx):
        if len(idx) == 0:
            return
        want = np.zeros(B, dtype=bool)
        want[idx] = True
        for rows, ub in groups:        # (the oracle solves whole batches: solve every group with a wanted row, keep those rows)
            sel = want[rows]
            if not sel.any():
                continue
            n = ub.N
            tmp = synth.Batch(np.ascontiguousarray(ctrl[rows, :n]), ub.guide_off, ub.guide_pv, ub.guide_unk, ub.obs_off, ub.obs)
            with emulation(n):
                r = ol.optimize_batch(P, tmp, weights=np.ascontiguousarray(w[rows]))
            ctrl[rows[sel], :n] = r["ctrl"][sel]
            st[rows[sel], S_LBFGS] = r["status"][sel]

    first = np.where((st[:, S_STATUS] == RB_ACTIVE) & (st[:, S_SOLVE] != 0))[0]
    solve(first)
    st[first, S_SOLVE] = 0
    waiting = False
    for _ in range(max_rounds):
        if waiting:
            break
        raised = False
        for i in np.where(st[:, S_STATUS] == RB_ACTIVE)[0]:
            n = int(pb.n_pts[i])
            c = np.ascontiguousarray(ctrl[i, :n])
            goff = np.ascontiguousarray(pb.guide_off[i * Ns:i * Ns + n + 1])
            o = np.ascontiguousarray(pb.obs[pb.obs_off[i]:pb.obs_off[i + 1]]) if pb.obs is not None else np.zeros((0, 9))
            wi, si = np.ascontiguousarray(w[i]), np.ascontiguousarray(st[i])
            status = O.vgo_rebound_decide(C.byref(P), C.byref(g), n, ol._d(c), ol._i(goff), ol._d(pb.guide_pv) if len(pb.guide_pv) else None,
                                          len(o), ol._d(o) if len(o) else None, gate_dt, ncr, ol._d(wi), ol._i(si))
            w[i], st[i] = wi, si
            raised = raised or status == RB_NEEDS_HOST
        active = np.where(st[:, S_STATUS] == RB_ACTIVE)[0]
        if raised:                       # a trajectory waits for A*: the optimize() the active ones owe is deferred, for ALL
            st[active, S_SOLVE] = 1
            waiting = True
        else:
            solve(active)
    return ctrl, w, st


def pulling_guides_everywhere(pb, seed=5):
    """the construction of tests/test_gpu_rebound.py for a padded batch: EVERY control point of a trajectory gets one guide
    pair whose point lies 3 m ahead in a random horizontal direction, so isControlPointRequireNewGuide is false for every
    point, always, and the previous collision segment covers the whole trajectory: nobody asks for A* before failCount
    reaches 4.  Returns (padded batch with those guides, state)."""
    rng = np.random.default_rng(seed)
    B, Ns = pb.ctrl.shape[:2]
    counts = np.zeros((B, Ns), dtype=np.int64)
    for b in range(B):
        counts[b, :pb.n_pts[b]] = 1
    goff = np.zeros(B * Ns + 1, dtype=np.int32)
    goff[1:] = np.cumsum(counts.reshape(-1))
    c = pb.ctrl.reshape(-1, 3)[counts.reshape(-1) == 1]
    u = rng.normal(size=c.shape)
    u[:, 2] = 0.0
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    gpv = np.ascontiguousarray(np.concatenate([c + 3.0 * u, u], axis=1))
    state = np.zeros((B, STATE_INTS), dtype=np.int32)
    state[:, S_SOLVE] = 1
    state[:, S_NSEG] = 1
    state[:, S_SEG] = 2
    state[:, S_SEG + 1] = pb.n_pts - 1
    return synth.PaddedBatch(pb.ctrl, goff, gpv, np.zeros(len(gpv), dtype=np.uint8), None, None, None, dict(pb.meta), pb.n_pts), state


# ---- makePlanBatch under setMixedBatches (needs a GPU) -------------------------------------------------------------------
def pose_lists(world, poses, seed=23):
    """one straight jittered path of poses[t] poses, 0.25 m apart, per planner, with both ends free and inside the map:
    (path_off [n+1], xyz [sum, 3])"""
    rng = np.random.default_rng(seed)
    half = -float(world.origin[0]) - 0.3
    out = []
    for K in poses:
        s = np.arange(K) * synth.CTRL_SPACING
        while True:
            M = 512
            start = np.concatenate([rng.uniform(-half, half, size=(M, 2)), np.full((M, 1), 1.0)], axis=1)
            heading = rng.uniform(0.0, 2 * np.pi, size=M)
            dirv = np.stack([np.cos(heading), np.sin(heading), np.zeros(M)], axis=1)
            lat = np.stack([-np.sin(heading), np.cos(heading), np.zeros(M)], axis=1)
            pts = start[:, None, :] + s[None, :, None] * dirv[:, None, :] + rng.normal(0.0, 0.05, size=(M, K, 1)) * lat[:, None, :]
            ok = (np.abs(pts[:, -1, :2]).max(1) < half) & (synth.lookup(world, pts[:, 0], 0) == 0) & (synth.lookup(world, pts[:, -1], 0) == 0)
            if ok.any():
                out.append(pts[np.argmax(ok)])
                break
    off = np.concatenate([[0], np.cumsum([len(p) for p in out])]).astype(np.int32)
    return off, np.ascontiguousarray(np.concatenate(out))


def plan_batch_mixed(world, path_off, xyz, reps=1, cfg=synth.PIPELINE_CFG):
    """makePlanBatch with setMixedBatches off (slot 0) and on (slot 1), `reps` rounds over off, then on -> dict of per-slot
    arrays; counts[slot] = (device batches the solves and rounds opened, planners in them)"""
    import plan_batch as pb
    r = pb.plan_batch(world, path_off, xyz, [(0, 16384, pb.BY_CALL), (pb.MIXED_BATCHES, 16384, pb.BY_CALL)], [0, 1] * reps, cfg=cfg)
    return dict(total_ms=r["slot_seconds"][:, :, 2] * 1e3, counts=pb.stat(r, "solveBatches", "solvePlanners"), switches=r["switches"],
                **{k: r[k] for k in ("ok", "solver", "ncp", "ctrl", "n_seg", "segs", "n_guides", "guides")})
