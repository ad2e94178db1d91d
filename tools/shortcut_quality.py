#!/usr/bin/env python3
"""What force-aware shortcutting (tcmp_plan_shortcut) does to the bench's queries: per query,
the plan finished without the stage and then again with it -- status, waypoints, path cost
before / after, the straight-line dist(start, goal) as the lower bound, the stage's device time
next to ms_finish.  Queries: bench.py's own C3 scene and per-step seeds at B = 262,144 and
B = 65,536, and one C4 step (64 queries, 1e5 samples each, B = 65,536); bench.py is imported
read-only.  usage: python tools/shortcut_quality.py [--steps N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from torque_constrained_motion_planning_amd import _lib  # noqa: E402


def dist(a, b):
    d = np.asarray(b, dtype=np.float64) - np.asarray(a, dtype=np.float64)
    return float(np.sqrt((10.0 * d * d).sum()))


def one(eng, query, n_samples, batch, seed, mode, mass, passes):
    obs, pack, goal = query
    eng.set_scene(obs, pack)
    assert eng.plan_begin(bench.START, goal, mode, mass, 5.0, max_nodes=n_samples + 1,
                          max_batch=batch, seed=seed) == _lib.PLAN_OK
    t0 = time.perf_counter()
    eng.plan_run(n_samples, batch)
    eng.synchronize()
    t1 = time.perf_counter()
    r0 = eng.plan_finish()
    rec = dict(seed=seed, status=r0.status, n_waypoints=r0.n_waypoints, goal_cost=r0.goal_cost,
               straight=dist(bench.START, goal), ms_finish=r0.ms_finish,
               ms_rounds=r0.ms_nearest + r0.ms_edges + r0.ms_insert + r0.ms_rewire + r0.ms_edge_prep,
               wall_run_ms=(t1 - t0) * 1e3)
    if not r0.goal_found:
        return rec
    t2 = time.perf_counter()
    sc = eng.plan_shortcut(passes=passes)
    t3 = time.perf_counter()
    r1 = eng.plan_finish()
    rec.update(sc_status=r1.status, sc_n_waypoints=r1.n_waypoints, cost_before=sc.cost_before,
               cost_after=sc.cost_after, sc_ms=sc.ms, sc_wall_ms=(t3 - t2) * 1e3,
               sc_ms_finish=r1.ms_finish - r0.ms_finish, chords_tested=sc.chords_tested,
               chords_valid=sc.chords_valid, chords_used=sc.chords_used,
               chord_steps=sc.chord_steps, passes_run=sc.passes_run)
    return rec


def summary(rows):
    g = [r for r in rows if "cost_after" in r]
    ratio = [r["cost_after"] / r["cost_before"] for r in g]
    gap = [(r["cost_after"] - r["straight"]) / (r["cost_before"] - r["straight"]) for r in g
           if r["cost_before"] > r["straight"]]
    step = [r["sc_ms"] / (r["ms_rounds"] + r["ms_finish"]) for r in g if r["ms_rounds"] > 0]
    return dict(queries=len(rows), goal=len(g),
                cost_ratio_median=statistics.median(ratio) if ratio else None,
                cost_ratio_mean=statistics.fmean(ratio) if ratio else None,
                excess_over_straight_ratio_median=statistics.median(gap) if gap else None,
                status3_to_0=sum(1 for r in g if r["status"] == 3 and r["sc_status"] == 0),
                status0_to_3=sum(1 for r in g if r["status"] == 0 and r["sc_status"] == 3),
                status3_before=sum(1 for r in g if r["status"] == 3),
                status3_after=sum(1 for r in g if r["sc_status"] == 3),
                waypoints_mean=(statistics.fmean(r["n_waypoints"] for r in g),
                                statistics.fmean(r["sc_n_waypoints"] for r in g)) if g else None,
                sc_ms_mean=statistics.fmean(r["sc_ms"] for r in g) if g else None,
                sc_wall_ms_mean=statistics.fmean(r["sc_wall_ms"] for r in g) if g else None,
                ms_finish_mean=statistics.fmean(r["ms_finish"] for r in g) if g else None,
                sc_share_of_step_mean=statistics.fmean(step) if step else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--out", default=os.path.join("profiles", "shortcut_quality.json"))
    args = ap.parse_args()
    eng = _lib.Engine(0)
    out = dict(passes=args.passes, sets={})
    c3, c4 = bench.WORKLOADS["c3"], bench.WORKLOADS["c4"]
    q3 = bench.make_query(1234, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"], engine=eng)
    for batch in (c3["batch"], c3["alt_batch"]):
        rows = [one(eng, q3, c3["samples"], batch, 1234 + s, c3["mode"], c3["mass"], args.passes)
                for s in range(args.steps)]
        out["sets"]["c3_B%d" % batch] = dict(summary=summary(rows), queries=rows)
    rows = []
    for j in range(c4["queries"]):
        q = bench.make_query(1234 + j, n_obs=c4["boxes"], mode=c4["mode"], mass=c4["mass"],
                             engine=eng)
        rows.append(one(eng, q, c4["samples"], c4["batch"], 1234 + 7919 * j, c4["mode"],
                        c4["mass"], args.passes))
    out["sets"]["c4_step0"] = dict(summary=summary(rows), queries=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for k, v in out["sets"].items():
        print(k, json.dumps(v["summary"]))


if __name__ == "__main__":
    main()
