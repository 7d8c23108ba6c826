"""Writes tests/golden/poly_ref.npz from the compiled reference's polynomial side (oracle/_ref/libref_poly.so).  Runs only
where the reference is mounted and `make -C oracle` has built that library:

    python tests/golden/make_poly_golden.py

Every case of tests/poly_ref_cases.py is run through its runner; the arrays it returns, next to the case's inputs
('in_*'), go into one member per case, '<kind>/<case>' (kind s: polyTrajSolver, p: polyTrajOccMap, w: pwlTraj;
poly_ref_cases.pack / Fixture give the layout), beside the worlds ('world/<name>'), the certified answer to every QP the
reference asked for ('qp': the minimiser per digest, or an empty array for an infeasible QP) and 'meta', a JSON text with
the case names, the dropped cases and their reasons, the drop counts, the share of samples in the pow mask and the index
of every member.  Data only."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as ol  # noqa: E402
import poly_ref_cases as pc  # noqa: E402

OUT = os.path.join(HERE, "poly_ref.npz")


def solver_inputs(c):
    K = len(c["wp"]) - 1
    nan = np.full(0, np.nan)
    return {"in_wp": c["wp"], "in_params": np.array([c["diff"], c["cont"], c["vel"], c["cres"]], np.float64),
            "in_conds": nan if c["conds"] is None else np.asarray(c["conds"], np.float64),
            "in_corridor": nan if c["corridor"] is None else np.asarray(c["corridor"], np.float64),
            "in_second": nan if c["second"] is None else np.asarray(c["second"], np.float64),
            "in_soft": nan if c["soft"] is None else np.array([c["soft"][0]] + list(c["soft"][1]), np.float64),
            "in_force": np.array(c["force"], np.int32), "in_delT": np.array(c["delT"], np.float64), "in_K": np.int32(K)}


def plan_inputs(c):
    return {"in_wp": c["wp"], "in_cfg": pc.plan_cfg(c), "in_mode": np.int32(c["mode"]),
            "in_conds": np.full(0, np.nan) if c["conds"] is None else np.asarray(c["conds"], np.float64)}


def generate(L, hook, log=print):
    """-> (arrays, meta)"""
    arrays, meta = {}, {"solver": [], "plan": [], "pwl": [], "dropped": {}}
    t0 = time.time()
    for kind, cases, run, inputs in (("s", pc.solver_cases(), pc.run_solver_case, solver_inputs),
                                     ("p", pc.plan_cases(), pc.run_plan_case, plan_inputs)):
        for c in cases:
            try:
                out = run(L, hook, c)
            except pc.Dropped as e:
                meta["dropped"][c["name"]] = str(e)
                log(f"dropped {c['name']}: {e}")
                continue
            out.update(inputs(c))
            if kind == "p":
                meta.setdefault("world_of", {})[c["name"]] = c["world"]
            for k, v in out.items():
                arrays[f"{kind}/{c['name']}/{k}"] = np.asarray(v)
            meta["solver" if kind == "s" else "plan"].append(c["name"])
            log(f"{time.time() - t0:7.1f}s {c['name']}")
    for c in pc.pwl_cases():
        out = pc.run_pwl_case(L, c)
        out.update({"in_wp": c["wp"], "in_args": np.array([c["overload"], c["use_yaw"], c["vel"]], np.float64)})
        for k, v in out.items():
            arrays[f"w/{c['name']}/{k}"] = np.asarray(v)
        meta["pwl"].append(c["name"])
    for name, make in pc.WORLDS.items():
        arrays[f"world/{name}"] = make()
    for key, x in hook.cache.items():
        arrays[f"qp/{key}"] = np.zeros(0) if x is None else x
    # the named cases are what their names say
    g = lambda name, field: arrays[f"{name}/{field}"]
    assert g("p/plan_valid_at_once", "verdict") == 1 and g("p/plan_valid_at_once", "solves") == 1
    assert g("p/plan_valid_after_shrinking", "verdict") == 1 and g("p/plan_valid_after_shrinking", "solves") > 1
    assert g("p/plan_inflated_but_known_is_no_collision", "verdict") == 1 and g("p/plan_inflated_but_known_is_no_collision", "solves") == 1
    for name, it in (("p/plan_out_of_iterations", 2), ("p/plan_out_of_iterations_pwl", 2), ("p/plan_infeasible_while_shrinking", 9)):
        assert g(name, "verdict") == 0 and g(name, "solves") == it + 1, name
    assert g("p/plan_infeasible_while_shrinking", "qp_status")[0].max() == 0 and g("p/plan_infeasible_while_shrinking", "qp_status").max() > 0
    assert g("p/plan_out_of_iterations_pwl", "duration") > g("p/plan_out_of_iterations_pwl", "knots")[-1]
    assert g("p/plan_valid_with_pwl_configured", "verdict") == 1
    assert g("p/plan_no_corridor_mode", "verdict") == 1 and g("p/plan_no_corridor_mode", "check_flag") == 1
    assert g("s/cor_res5_generous", "x").shape and not (g("s/cor_second_round_shrunk", "tag_2") != 1).any()
    assert (g("s/cor_second_round_forced_infeasible", "status_2") != 0).all()
    assert np.array_equal(g("s/cor_second_round_forced_infeasible", "sol_2"), g("s/cor_second_round_forced_infeasible", "sol"))
    st = g("s/cor_second_round_y_forced_infeasible", "status_2")
    assert st[1] != 0 and st[0] == 0 and st[2] == 0
    kn, tr = g("s/samp_knots_on_the_clock", "knots"), g("s/samp_knots_on_the_clock", "traj_0.1")
    hits = sum(pc.clock(0.1, j) in set(kn[1:-1]) for j in range(len(tr) - 1))
    meta["inner_knot_hits"] = int(hits)
    assert hits >= 1, "no sample falls on an inner knot"
    kn, tr = g("s/samp_clock_ends_on_last_knot", "knots"), g("s/samp_clock_ends_on_last_knot", "traj_0.1")
    assert pc.clock(0.1, len(tr) - 1) == kn[-1]
    kn, tr = g("s/samp_clock_passes_last_knot_by_ulps", "knots"), g("s/samp_clock_passes_last_knot_by_ulps", "traj_0.1")
    assert 0 < pc.clock(0.1, len(tr) - 1) - kn[-1] < 1e-15
    assert len(g("s/samp_last_knot_an_ulp_above_the_clock", "traj_0.1")) == len(tr) + 1
    # the drop rule: every named case survives, at most one seeded random case in ten is dropped
    named = [n for n in meta["dropped"] if not n.startswith("rand_")]
    assert not named, f"named cases dropped: {named}"
    n_rand = sum(c["name"].startswith("rand_") for c in pc.solver_cases() + pc.plan_cases())
    n_drop = len(meta["dropped"])
    meta["random_cases"], meta["random_dropped"] = n_rand, n_drop
    assert n_drop <= pc.DROP_CAP * n_rand, (n_drop, n_rand)
    masks = [v for k, v in arrays.items() if "/powmask" in k]
    meta["pow_samples"] = int(sum(len(m) for m in masks))
    meta["pow_masked"] = int(sum(int(m.sum()) for m in masks))
    assert meta["pow_masked"] <= 0.01 * meta["pow_samples"], (meta["pow_masked"], meta["pow_samples"])
    meta["duplicate_inserts"] = int(sum(int(v) for k, v in arrays.items() if k.endswith("/dup")))
    return arrays, meta


def main():
    L = ol.ref_poly()
    if L is None:
        sys.exit("oracle/_ref/libref_poly.so is not built: mount the reference and run make -C oracle")
    arrays, meta = generate(L, pc.QpHook())
    np.savez_compressed(OUT, **pc.pack(arrays, meta))
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1024:.0f} KiB, {len(meta['solver'])} solver, {len(meta['plan'])} planner, "
          f"{len(meta['pwl'])} PWL cases; dropped {meta['dropped']}; pow mask {meta['pow_masked']} / {meta['pow_samples']}")


if __name__ == "__main__":
    main()
