"""vigo_host_plan_batch's job struct (host/src/cabiPlanBatch.h) against its one Python mirror (plan_batch.Job), and the
entry's argument checks: a bad job is refused before a map or a planner is made, so none of this needs a GPU."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import plan_batch as pb

WORLD = SimpleNamespace(voxels=np.zeros((4, 4, 4), dtype=np.uint8), origin=np.zeros(3), res=0.1)
OFF, XYZ = np.array([0, 2, 5]), np.zeros((5, 3))                       # two planners, paths of 2 and 3 poses
CALL, SETTERS, UNTOUCHED = ((0, 16384, route) for route in (pb.BY_CALL, pb.BY_SETTERS, pb.UNTOUCHED))
MIXED = (pb.MIXED_BATCHES, 16384, pb.BY_CALL)


def refused(slots=(CALL,), schedule=(0,), off=OFF, **options):
    job, arrays = pb.build_job(WORLD, off, XYZ, list(slots), list(schedule), **options)
    return pb.host_lib().vigo_host_plan_batch(C.byref(job)) == -1


def test_the_struct_has_the_librarys_size():
    assert C.sizeof(pb.Job) == pb.host_lib().vigo_host_plan_batch_job_size()


def test_a_wrong_size_field_is_refused():
    job, arrays = pb.build_job(WORLD, OFF, XYZ, [CALL], [0])
    job.size += 4
    assert pb.host_lib().vigo_host_plan_batch(C.byref(job)) == -1


@pytest.mark.parametrize("bad", [dict(off=[0]),                                                  # n = 0
                                 dict(off=[0, 2, 3]),                                            # a path of one pose
                                 dict(schedule=[1]),                                             # run_slot == n_slots
                                 dict(slots=[(pb.ASTAR, 16384, pb.UNTOUCHED)]),                  # route 2 with a mask
                                 dict(slots=[CALL, (pb.MIXED_BATCHES, 16384, pb.BY_SETTERS)], schedule=[0, 1], concurrent=True),
                                 dict(slots=[CALL, MIXED], schedule=[0, 1, 0], concurrent=True),
                                 dict(slots=[CALL, MIXED], schedule=[0, 0], concurrent=True),    # one slot twice
                                 dict(replay_slot=1),                                            # replay_slot == n_slots
                                 dict(slots=[SETTERS], replay_slot=0),                           # a step log needs the options route
                                 dict(n_maps=0), dict(schedule=[]), dict(slots=[(512, 16384, pb.BY_CALL)]), dict(slots=[(0, 16384, 3)]),
                                 dict(planner_timestep=[np.nan, 0.0])], ids=lambda bad: " ".join(bad))
def test_a_bad_job_is_refused(bad):
    assert refused(**bad)
