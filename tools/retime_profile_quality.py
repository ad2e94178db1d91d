#!/usr/bin/env python3
"""The three retiming forms side by side on the queries of tools/retime_quality.py (bench.py's
C3 scene and per-step seeds at both batch sizes, one C4 step, and C4's first eight queries under
the full-size fixture's seeds): per query the plan is finished three times and retimed once
each way -- uniform (tcmp_plan_retime), per run (tcmp_plan_retime_runs) and by velocity profile
(tcmp_plan_retime_profile) -- and the record holds the execution time as planned and after each,
the statuses and the device ms of each stage.  A query that validates is retimed too (every form
leaves it as it is), for the stages' times on it.  bench.py is imported read-only.
usage: python tools/retime_profile_quality.py [--steps N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from torque_constrained_motion_planning_amd import _lib  # noqa: E402

EXEC = 5.0


def one(eng, query, n_samples, batch, seed, mode, mass):
    obs, pack, goal = query
    eng.set_scene(obs, pack)
    assert eng.plan_begin(bench.START, goal, mode, mass, EXEC, max_nodes=n_samples + 1,
                          max_batch=batch, seed=seed) == _lib.PLAN_OK
    eng.plan_run(n_samples, batch)
    r0 = eng.plan_finish()
    rec = dict(seed=seed, status=r0.status, n_traj=r0.n_traj, first_fail=r0.first_fail,
               ms_finish=r0.ms_finish, exec_planned=EXEC)
    if r0.status not in (_lib.PLAN_OK, _lib.PLAN_VALIDATION_FAILED):
        return rec
    u = eng.plan_retime()
    eng.plan_finish()
    _, rr = eng.plan_retime_runs()
    eng.plan_finish()
    p = eng.plan_retime_profile()
    rec.update(uniform_status=u.status, uniform_exec=u.exec_time_after, uniform_ms=u.ms,
               uniform_x=u.x,
               runs_status=rr.status, runs_exec=rr.exec_time_after, runs_ms=rr.ms,
               runs_n=rr.n_runs,
               profile_status=p.status, profile_exec=p.exec_time_after, profile_ms=p.ms,
               profile_anchored=p.anchored, profile_x_min=p.x_min,
               profile_n_at_floor=p.n_at_floor, profile_n_at_cap=p.n_at_cap)
    return rec


def summary(rows):
    g = [r for r in rows if "profile_status" in r]
    failed = [r for r in g if r["status"] == _lib.PLAN_VALIDATION_FAILED]
    both = [r for r in failed if r["uniform_status"] == 0 and r["profile_status"] == 0]

    def mean(key, rs):
        return statistics.fmean(r[key] for r in rs) if rs else None
    return dict(queries=len(rows), with_trajectory=len(g), status3_before=len(failed),
                fixed_uniform=sum(r["uniform_status"] == 0 for r in failed),
                fixed_runs=sum(r["runs_status"] == 0 for r in failed),
                fixed_profile=sum(r["profile_status"] == 0 for r in failed),
                exec_ratio_uniform=[r["uniform_exec"] / EXEC for r in both],
                exec_ratio_runs=[r["runs_exec"] / EXEC for r in both if r["runs_status"] == 0],
                exec_ratio_profile=[r["profile_exec"] / EXEC for r in both],
                uniform_ms_mean=mean("uniform_ms", g), runs_ms_mean=mean("runs_ms", g),
                profile_ms_mean=mean("profile_ms", g), ms_finish_mean=mean("ms_finish", g),
                n_traj_mean=mean("n_traj", g))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=os.path.join("profiles", "retime_profile_quality.json"))
    args = ap.parse_args()
    eng = _lib.Engine(0)
    out = dict(steps=args.steps, sets={})
    c3, c4 = bench.WORKLOADS["c3"], bench.WORKLOADS["c4"]
    q3 = bench.make_query(1234, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"], engine=eng)
    for batch in (c3["batch"], c3["alt_batch"]):
        rows = [one(eng, q3, c3["samples"], batch, 1234 + s, c3["mode"], c3["mass"])
                for s in range(args.steps)]
        out["sets"]["c3_B%d" % batch] = dict(summary=summary(rows), queries=rows)
    rows = []
    for j in range(c4["queries"]):
        q = bench.make_query(1234 + j, n_obs=c4["boxes"], mode=c4["mode"], mass=c4["mass"],
                             engine=eng)
        rows.append(one(eng, q, c4["samples"], c4["batch"], 1234 + 7919 * j, c4["mode"],
                        c4["mass"]))
    out["sets"]["c4_step0"] = dict(summary=summary(rows), queries=rows)
    rows = []
    for j in range(8):
        q = bench.make_query(1234 + j, n_obs=c4["boxes"], mode=c4["mode"], mass=c4["mass"],
                             engine=eng)
        rows.append(one(eng, q, c4["samples"], c4["batch"], 5000 + j, c4["mode"], c4["mass"]))
    out["sets"]["c4_fixture_seeds"] = dict(summary=summary(rows), queries=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for k, v in out["sets"].items():
        print(k, json.dumps(v["summary"]))


if __name__ == "__main__":
    main()
