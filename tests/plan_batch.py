"""The one binding of vigo_host_plan_batch (host/src/cabiPlanBatch.h): n planners plan by bsplineTraj::makePlanBatch under
the options of a SLOT, one run on fresh planners per entry of a SCHEDULE of slots.  Job mirrors the C struct and is its
only declaration on this side; plan_batch() checks its size against the library's before every call."""
import ctypes as C
import os

import numpy as np

from trajectory_planner_amd import synth

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "trajectory_planner_amd", "lib", "libtrajectory_planner_vigo.so")

# a slot's mask: vigo_host_switches' bits
ASTAR, GUIDES1, GUIDES2, PROLOGUE, REGUIDE1, REGUIDE2, MIXED_BATCHES, EPILOGUE, MIXED_PROLOGUE = (1 << k for k in range(9))
# a slot's route: the options passed to the call / set through the setters and put back / the untouched default (mask 0)
BY_CALL, BY_SETTERS, UNTOUCHED = 0, 1, 2
# BatchStats' count fields in the order of their declaration
STAT_NAMES = ("astarDecided", "astarHost", "guidesDecided", "guidesHost", "prologueDecided", "prologueHost", "reguideDecided", "reguideHost",
              "epilogueDecided", "epilogueHost", "seedDecided", "seedHost", "epilogueGroups", "solveBatches", "solvePlanners", "prologueGroups",
              "reguideGroups", "validateDecided", "validateHost", "validateGroups")

_INPUTS = ("vox", "vox2", "dims", "origin", "cfg", "path_off", "path_xyz", "planner_device", "planner_timestep", "slot_mask", "slot_budget",
           "slot_route", "run_slot")
# the per-slot outputs a caller may ask for -> the arrays of each: (name, dtype, shape after [n_slots]) for n planners
_OUTPUTS = {"ok": lambda j: [("ok", np.int32, (j.n,))],
            "solver": lambda j: [("solver", np.int32, (j.n,))],
            "ncp": lambda j: [("ncp", np.int32, (j.n,))],
            "ctrl": lambda j: [("ctrl", np.float64, (j.n, j.ncp_cap, 3))],
            "factor": lambda j: [("factor", np.float64, (j.n,))],
            "segs": lambda j: [("n_seg", np.int32, (j.n,)), ("segs", np.int32, (j.cap, 2))],
            "paths": lambda j: [("n_path_pts", np.int32, (j.n,)), ("paths", np.float64, (j.cap, 3))],
            "guides": lambda j: [("n_guides", np.int32, (j.n,)), ("guides", np.float64, (j.cap, 6))],
            "poses": lambda j: [("n_poses", np.int32, (j.n,)), ("pos", np.float64, (j.n, j.pose_cap, 3)), ("quat", np.float64, (j.n, j.pose_cap, 4))]}


class Job(C.Structure):
    _fields_ = [("size", C.c_int), ("n_maps", C.c_int), ("vox", C.c_void_p), ("vox2", C.c_void_p), ("dims", C.c_void_p), ("origin", C.c_void_p),
                ("res", C.c_double), ("cfg", C.c_void_p),
                ("n", C.c_int), ("with_paths", C.c_int), ("yaw", C.c_int), ("path_off", C.c_void_p), ("path_xyz", C.c_void_p),
                ("planner_device", C.c_void_p), ("planner_timestep", C.c_void_p),
                ("n_slots", C.c_int), ("slot_mask", C.c_void_p), ("slot_budget", C.c_void_p), ("slot_route", C.c_void_p),
                ("n_runs", C.c_int), ("run_slot", C.c_void_p), ("concurrent", C.c_int), ("replay_slot", C.c_int), ("caps", C.c_int * 4),
                ("ncp_cap", C.c_int), ("pose_cap", C.c_int), ("cap", C.c_longlong),
                ("ok", C.c_void_p), ("solver", C.c_void_p), ("ncp", C.c_void_p), ("ctrl", C.c_void_p), ("factor", C.c_void_p),
                ("n_seg", C.c_void_p), ("segs", C.c_void_p), ("n_path_pts", C.c_void_p), ("paths", C.c_void_p), ("n_guides", C.c_void_p),
                ("guides", C.c_void_p), ("n_poses", C.c_void_p), ("pos", C.c_void_p), ("quat", C.c_void_p),
                ("stats", C.c_void_p), ("totals", C.c_void_p), ("twin", C.c_void_p), ("seconds", C.c_void_p)]


def host_lib(path=None):
    lib = C.CDLL(path or LIB)
    lib.vigo_host_plan_batch.restype = lib.vigo_host_plan_batch_job_size.restype = lib.vigo_host_switches.restype = C.c_int
    lib.vigo_host_plan_batch.argtypes = [C.POINTER(Job)]
    return lib


def uniform_paths(pts):
    """pts[P][n_pts][3] as (path_off, xyz)"""
    return np.arange(pts.shape[0] + 1, dtype=np.int32) * pts.shape[1], pts.reshape(-1, 3)


def build_job(world, path_off, xyz, slots, schedule, outputs=("ok", "solver", "ncp", "ctrl", "segs", "guides"), cfg=None, vox2=None, n_maps=1,
              with_paths=False, yaw=True, planner_device=None, planner_timestep=None, concurrent=False, replay_slot=-1, caps=(0, 0, 0, 0), ncp_cap=96,
              room=None, pose_cap=0):
    """-> (job, the arrays its pointers name).  world: .voxels, .origin, .res; slots: (mask, budget, route) each; schedule:
    the slot of each run; outputs: keys of _OUTPUTS; room: the rows per slot of segs / paths / guides.  Nothing is checked
    here: that is the entry's part."""
    arr = dict(vox=np.ascontiguousarray(world.voxels, dtype=np.uint8), vox2=None if vox2 is None else np.ascontiguousarray(vox2, dtype=np.uint8),
               origin=np.ascontiguousarray(world.origin, dtype=np.float64),
               cfg=np.ascontiguousarray(synth.PIPELINE_CFG if cfg is None else cfg, dtype=np.float64),
               path_off=np.ascontiguousarray(path_off, dtype=np.int32), path_xyz=np.ascontiguousarray(xyz, dtype=np.float64),
               planner_device=None if planner_device is None else np.ascontiguousarray(planner_device, dtype=np.int32),
               planner_timestep=None if planner_timestep is None else np.ascontiguousarray(planner_timestep, dtype=np.float64),
               run_slot=np.ascontiguousarray(schedule, dtype=np.int32))
    arr["dims"] = np.array(arr["vox"].shape, dtype=np.int32)
    arr["slot_mask"], arr["slot_budget"], arr["slot_route"] = (np.array([s[k] for s in slots], dtype=np.int32) for k in range(3))
    job = Job(size=C.sizeof(Job), n_maps=n_maps, res=float(world.res), n=len(arr["path_off"]) - 1, with_paths=int(bool(with_paths)), yaw=int(bool(yaw)),
              n_slots=len(slots), n_runs=len(arr["run_slot"]), concurrent=int(bool(concurrent)), replay_slot=replay_slot, caps=(C.c_int * 4)(*caps),
              ncp_cap=ncp_cap, pose_cap=pose_cap)
    job.cap = 256 * job.n if room is None else room
    for key in outputs:
        for name, dtype, shape in _OUTPUTS[key](job):
            arr[name] = np.zeros((job.n_slots,) + shape, dtype=dtype)
    arr["stats"], arr["totals"] = np.zeros((job.n_slots, len(STAT_NAMES)), dtype=np.int64), np.zeros(len(STAT_NAMES), dtype=np.int64)
    arr["twin"], arr["seconds"] = np.zeros(2, dtype=np.int64), np.zeros((job.n_runs, 3))
    for name, a in arr.items():
        setattr(job, name, None if a is None else a.ctypes.data)
    return job, arr


def plan_batch(world, path_off, xyz, slots, schedule, lib=None, **options):
    """vigo_host_plan_batch -> dict: the outputs asked for, [n_slots, ...] of each slot's last run; stats [n_slots, K] and
    totals [K] (columns: STAT_NAMES); twin [2]; seconds [n_runs, 3] (prologue, chains, the whole call) and the same by slot,
    slot_seconds [n_slots, most runs of a slot, 3] (a slot's k-th run in row k, zeros after its last); switches.  lib: the path
    of another build of the library"""
    lib = host_lib(lib)
    job, arr = build_job(world, path_off, xyz, slots, schedule, **options)
    assert C.sizeof(Job) == lib.vigo_host_plan_batch_job_size()
    rc = lib.vigo_host_plan_batch(C.byref(job))
    assert rc == 0, rc
    r = {k: a for k, a in arr.items() if k not in _INPUTS}
    runs = [int(s) for s in arr["run_slot"]]
    r["slot_seconds"] = np.zeros((len(slots), max(runs.count(s) for s in set(runs)), 3))
    for i, s in enumerate(runs):
        r["slot_seconds"][s, runs[:i].count(s)] = r["seconds"][i]
    r["switches"] = int(lib.vigo_host_switches())
    return r


def stat(r, *names):
    """the columns `names` of a result's stats: [n_slots] for one name, [n_slots, len(names)] for more"""
    cols = r["stats"][:, [STAT_NAMES.index(k) for k in names]]
    return cols[:, 0] if len(names) == 1 else cols
