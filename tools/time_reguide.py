#!/usr/bin/env python3
"""Wall time of bsplineTraj::makePlanBatch on the 1024-planner pipeline workload with the rebound loop's re-guide step on
the host (setDeviceReguide(0)), on the device (1) and on the workers' twin (2): `reps` alternating rounds through
vigo_host_plan_batch, the first one a warm-up, the median of the rest.  Prints the device / worker step totals.
Needs a GPU.  (profiles/README.md, "Device re-guide", holds a run of this.)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import reguide_cases as rc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planners", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--lib", help="another build of libtrajectory_planner_vigo.so (A/B of two builds)")
    a = ap.parse_args()
    if a.lib:
        rc.LIB = os.path.abspath(a.lib)
    r = rc.plan_batch_reguide(a.planners, reps=a.reps)
    for name, slot in (("0 (host step)", rc.SLOT_HOST), ("1 (vigo_rebound_reguide)", rc.SLOT_DEVICE), ("2 (workers' twin)", rc.SLOT_TWIN)):
        t = r["total_ms"][slot]
        print(f"setDeviceReguide {name}: makePlanBatch of {a.planners} median {np.median(t[1:]):.2f} ms over {a.reps - 1} runs after a warm-up "
              f"(min {t[1:].min():.2f}, max {t[1:].max():.2f}; warm-up {t[0]:.2f}); {int(r['ok'][slot].sum())} planned; "
              f"re-guide steps: {int(r['counts'][slot][0])} device, {int(r['counts'][slot][1])} workers")
    print(f"untouched default, one cold run: {r['total_ms'][rc.SLOT_UNTOUCHED][0]:.2f} ms")
    print(f"steps logged under setting 2: {int(r['twin'][0])}, decided by the kernels' twin under the shipped capacities: {int(r['twin'][1])}")


if __name__ == "__main__":
    main()
