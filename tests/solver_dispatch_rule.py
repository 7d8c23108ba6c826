"""The launch rule of vigo_optimize, restated independently of csrc/vigo_solver_plan.hpp (written from its comments, not
generated from it), and the dispatch matrix CELLS of test_gpu_solver_dispatch.py.  test_solver_plan.py holds the C++ plan
to this restatement and to CELLS without a GPU; test_gpu_solver_dispatch.py runs every cell against the oracle."""
from collections import namedtuple

PREC = {"f64": 0, "f32": 1, "fast": 2}   # VIGO_PREC_F64, _F32, _F64_FAST (include/vigo.h)
WAVE, LDS = 64, 160 * 1024           # kWave, kLdsPerWorkgroup
OBS_TAB_OBS = 16                     # kObsTabObs
LEVEL_RH = {32: 4, 64: 5}            # kLevelRH, kLevelRH64
MI355X_SIMDS = 4 * 256

# one k_optimize launch: the instantiation's (WPS, OBS, D, RH), the grid, the dynamic LDS bytes and the
# level_waves_elsewhere it is given
Launch = namedtuple("Launch", "wps obs D rh grid lds level_waves_elsewhere")


def obs_tab_entries(group):          # kObsTabEntries<GROUP>
    return 88 if group == 32 else 33


def shape_for(N):                    # (GROUP, PPL)
    return (32, 1) if N <= 32 else ((64, 1) if N <= 64 else ((64, 2) if N <= 128 else (64, 4)))


def lds_bytes(mode, N, m, D=3, obs=True, rh=1):
    """optimize_lds_bytes: the history slots that are not in registers (a record per free control point and column —
    a trajectory of the wave, or with D = 1 an axis — plus the zero column, then {ys, 1/ys} per trajectory), the
    alphas, the obstacle table"""
    group, ppl = shape_for(N)
    cols = WAVE // group
    tpb = 1 if D == 1 else cols
    hpair = -(-2 * D * (4 if mode == "f32" else 8) // 16) * 16          # alignas(16) HPair<T, D>
    ys = 8 if mode == "fast" else 16                                     # YSv<FAST>
    ms = (m - (rh + 1) if m > rh + 1 else 0) if ppl == 1 else m
    h = ms * ((cols * (N - 6) + 1) * hpair + ((tpb * ys + 15) & ~15)) + m * tpb * 8
    if obs:
        h += tpb * (3 * obs_tab_entries(group) + OBS_TAB_OBS) * 8
    return h


def plan(mode, N, B, m, has_obs, plan_in_z, strict_z, simds, allow_axis=True):
    """the k_optimize launches of one vigo_optimize call, in order; None: the shape does not fit the LDS.
    simds == 0: the SIMD count is unknown — never two waves per SIMD, never the axis kernel, never the redirect."""
    group, ppl = shape_for(N)
    grid = -(-B // (WAVE // group))
    more_waves = simds > 0 and grid > simds
    obs_inst = has_obs or (mode == "fast" and 32 < N <= 64 and simds > 0 and B > simds and bool(plan_in_z or strict_z))
    lds = lds_bytes(mode, N, m, obs=has_obs)     # by the list that is there, not by the instantiation
    if lds > LDS:
        return None
    out, elsewhere = [], 0
    if ppl == 1 and not obs_inst and not plan_in_z and not strict_z:     # the level launch comes first
        elsewhere = 1
        lds2 = lds_bytes(mode, N, m, D=2, obs=False)
        lds3 = lds_bytes(mode, N, m, D=2, obs=False, rh=LEVEL_RH[group])
        if mode == "f64" and group == 32 and 0 < B <= simds and allow_axis:
            out.append(Launch(1, False, 1, 1, B, lds_bytes(mode, N, m, D=1, obs=False), 1))    # a wave per trajectory
            elsewhere = 2
        elif mode != "f32" and more_waves and lds2 > LDS // 8 and LDS // lds3 > LDS // lds2:
            out.append(Launch(2, False, 2, LEVEL_RH[group], grid, lds3, 1))
        else:
            out.append(Launch(2 if more_waves and lds2 <= LDS // 8 else 1, False, 2, 1, grid, lds2, 1))
    out.append(Launch(2 if ppl == 1 and more_waves and lds <= LDS // 8 else 1, obs_inst, 3, 1 if ppl == 1 else 0, grid, lds, elsewhere))
    return out


def launches(mode, N, B, m, has_obs, plan_in_z, strict_z, simds):
    """the launches of plan() as (WPS, OBS, D, RH)"""
    return [tuple(l[:4]) for l in plan(mode, N, B, m, has_obs, plan_in_z, strict_z, simds)]


def kernel_name(mode, N, wps, obs, D, rh):
    group, ppl = shape_for(N)
    t = "float" if mode == "f32" else "double"
    b = lambda x: "true" if x else "false"
    return f"k_optimize<{t}, {group}, {ppl}, {b(mode == 'fast')}, {wps}, {b(obs)}, {D}, {rh}>"


def obs_table_fit(N, pred_num):
    """obstacles per trajectory k_optimize stages in LDS"""
    return min(OBS_TAB_OBS, obs_tab_entries(shape_for(N)[0]) // (pred_num // 2 + 1))


# ---- the dispatch matrix ------------------------------------------------------------------------------------------
# (cell, modes, N, batch: "small" = 40, "wps2" = the smallest batch with more waves than SIMDs, "simds+2" = two
#  trajectories more than SIMDs, mem_size, obstacles per trajectory, plan_in_z / strict_z, the launches expected on a
#  device of at least 40 SIMDs as (WPS, OBS, D, RH))
O, L = True, False
CELLS = [
    ("32x1-obs-wps1", "f64 fast f32", 20, "small", 16, 2, "", [(1, O, 3, 1)]),
    ("32x1-obs-wps2", "f64 fast f32", 16, "wps2", 16, 2, "", [(2, O, 3, 1)]),
    ("64x1-obs-wps1", "f64 fast f32", 50, "small", 16, 2, "", [(1, O, 3, 1)]),
    ("64x1-obs-wps2", "f64 fast f32", 40, "wps2", 5, 2, "", [(2, O, 3, 1)]),
    ("64x2-obs-wps1", "f64 fast f32", 100, "small", 16, 2, "", [(1, O, 3, 0)]),
    ("64x4-obs-wps1", "f64 fast f32", 200, "small", 16, 2, "", [(1, O, 3, 0)]),
    # at most one trajectory per SIMD: fp64 reference order takes the axis-per-lane kernel for the level ones
    ("32x1-level-wps1", "f64", 24, "small", 16, 0, "", [(1, L, 1, 1), (1, L, 3, 1)]),
    ("32x1-level-wps1", "fast f32", 24, "small", 16, 0, "", [(1, L, 2, 1), (1, L, 3, 1)]),
    # two trajectories per wave, a wave per SIMD or fewer: the fp64 D = 2 kernel of 512 registers
    ("32x1-level-pairs-wps1", "f64", 8, "simds+2", 16, 0, "", [(1, L, 2, 1), (1, L, 3, 1)]),
    ("32x1-level-wps2", "f64 fast f32", 16, "wps2", 16, 0, "", [(2, L, 2, 1), (2, L, 3, 1)]),
    ("32x1-level-rh-wps2", "f64 fast", 32, "wps2", 16, 0, "", [(2, L, 2, 4), (1, L, 3, 1)]),
    ("32x1-level-wps2-general-wps1", "f32", 32, "wps2", 16, 0, "", [(2, L, 2, 1), (1, L, 3, 1)]),
    ("64x1-level-wps1", "f64 fast f32", 50, "small", 16, 0, "", [(1, L, 2, 1), (1, L, 3, 1)]),
    ("64x1-level-wps2", "f64 fast f32", 40, "wps2", 5, 0, "", [(2, L, 2, 1), (2, L, 3, 1)]),
    ("64x1-level-rh-wps2", "f64 fast", 64, "wps2", 16, 0, "", [(2, L, 2, 5), (1, L, 3, 1)]),
    ("64x1-level-wps2-general-wps1", "f32", 64, "wps2", 16, 0, "", [(2, L, 2, 1), (1, L, 3, 1)]),
    ("64x2-noobs-wps1", "f64 fast f32", 100, "small", 16, 0, "", [(1, L, 3, 0)]),
    ("64x4-noobs-wps1", "f64 fast f32", 180, "small", 16, 0, "", [(1, L, 3, 0)]),
    ("32x1-planz-noobs-wps2", "f64 fast f32", 16, "wps2", 16, 0, "plan_in_z", [(2, L, 3, 1)]),
    ("64x1-strictz-noobs-wps1", "f64 fast f32", 50, "small", 16, 0, "strict_z", [(1, L, 3, 1)]),
    ("64x1-planz-noobs-wps2", "f64 f32", 40, "wps2", 5, 0, "plan_in_z", [(2, L, 3, 1)]),
    # f64_fast, 32 < N <= 64, more waves than SIMDs, plan_in_z or strict_z: the obstacle instantiation without a list
    ("64x1-redirect-wps1", "fast", 50, "wps2", 16, 0, "strict_z", [(1, O, 3, 1)]),
    ("64x1-redirect-wps2", "fast", 40, "wps2", 5, 0, "plan_in_z", [(2, O, 3, 1)]),
]


def cell_batch_size(cell, simds):
    N, bk = cell[2], cell[3]
    return {"small": 40, "wps2": WAVE // shape_for(N)[0] * simds + 1, "simds+2": simds + 2}[bk]
