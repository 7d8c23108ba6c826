"""-m gpu: bsplineTraj::makePlanBatch under setDeviceReguide through vigo_host_plan_batch, 256 planners of the
pipeline world.  Setting 1 (vigo_rebound_reguide per device group, what it defers by the workers' twin) against setting 2
(every re-guide step by the workers' twin): ok flags, solver statuses, control points, collisionSeg_, astarPaths_ and
guides of every planner bit for bit; the step counts; the device-decided steps equal to what the kernels' host twin
decides under the shipped capacities on the steps setting 2 logged.  Setting 0 against setDeviceReguide never called."""
import numpy as np
import pytest

import reguide_cases as rc

pytestmark = pytest.mark.gpu
P = 256


@pytest.fixture(scope="module")
def plans():
    return rc.plan_batch_reguide(P)


def _same(r, a, b, label):
    for k in ("ok", "solver", "ncp", "n_guides", "n_seg", "n_path_pts"):
        assert np.array_equal(r[k][a], r[k][b]), f"{label}: {k} differs"
    for k in ("ctrl", "guides", "paths"):
        assert np.array_equal(rc.bits(r[k][a]), rc.bits(r[k][b])), f"{label}: {k} differs"
    assert np.array_equal(r["segs"][a], r["segs"][b]), f"{label}: collision segments differ"


def test_device_reguide_is_the_twins_plan(plans):
    r = plans
    dev, host = (int(x) for x in r["counts"][rc.SLOT_DEVICE])
    steps2 = int(r["counts"][rc.SLOT_TWIN].sum())
    logged, twin_decided = (int(x) for x in r["twin"])
    print(f"\n{P} planners: {int(r['ok'][rc.SLOT_TWIN].sum())} planned; re-guide steps under setting 2: {steps2} (logged {logged}), of which the "
          f"twin under the shipped capacities decides {twin_decided}; setting 1: {dev} by vigo_rebound_reguide, {host} by the workers")
    _same(r, rc.SLOT_DEVICE, rc.SLOT_TWIN, "setDeviceReguide(1) against (2)")
    assert r["counts"][rc.SLOT_TWIN][0] == 0 and logged == steps2
    assert dev > 0 and dev + host == steps2
    assert dev == twin_decided                                    # the device defers what its twin defers, nothing more
    assert r["ok"][rc.SLOT_TWIN].sum() >= P // 2


def test_setting_0_is_the_untouched_default(plans):
    r = plans
    _same(r, rc.SLOT_HOST, rc.SLOT_UNTOUCHED, "setDeviceReguide(0) against the setter never called")
    assert r["counts"][rc.SLOT_HOST].tolist() == [0, 0] and r["counts"][rc.SLOT_UNTOUCHED].tolist() == [0, 0]


def test_every_switch_is_off_on_return(plans):
    assert plans["switches"] == 0
