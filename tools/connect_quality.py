#!/usr/bin/env python3
"""What the best-parent goal connection (tcmp_plan_connect) does to the bench's queries: per
query, the plan finished without the stage (the rounds are untouched by it, so this is the plan
as it was before the stage existed) and then again with it -- goal found, goal cost before /
after, the candidates tested and valid, the stage's device time next to the plan's summed ms_*.
Queries: bench.py's own C3 scene with per-step seeds and a seeded set of further 16-box queries
at the C3 shape (1e6 samples), each at B = 262,144 and B = 65,536; one C5-size tree (256 meshes,
a third of 1e7 samples) for the stage's time on a large tree.  bench.py is imported read-only.
One record per (candidates, passes) pair.
usage: python tools/connect_quality.py [--steps N] [--queries N] [--candidates K[,K...]]
       [--passes P[,P...]] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from torque_constrained_motion_planning_amd import _lib  # noqa: E402


def dist(a, b):
    d = np.asarray(b, dtype=np.float64) - np.asarray(a, dtype=np.float64)
    return float(np.sqrt((10.0 * d * d).sum()))


def one(eng, query, n_samples, batch, seed, mode, mass, K, passes):
    obs, pack, goal = query
    eng.set_scene(obs, pack)
    assert eng.plan_begin(bench.START, goal, mode, mass, 5.0, max_nodes=n_samples + 2,
                          max_batch=batch, seed=seed) == _lib.PLAN_OK
    eng.plan_run(n_samples, batch)
    r0 = eng.plan_finish()
    cn = eng.plan_connect(K, passes)
    r1 = eng.plan_finish()
    return dict(seed=seed, straight=dist(bench.START, goal), n_nodes=r0.n_nodes,
                status_before=r0.status, status_after=r1.status,
                goal_before=bool(r0.goal_found), goal_after=bool(r1.goal_found),
                cost_before=r0.goal_cost if r0.goal_found else None,
                cost_after=r1.goal_cost if r1.goal_found else None,
                connect=cn.as_dict(),
                ms_plan=r0.ms_nearest + r0.ms_edges + r0.ms_insert + r0.ms_rewire
                + r0.ms_edge_prep + r0.ms_finish)


def summary(rows):
    n = len(rows)
    both = [r for r in rows if r["goal_before"] and r["goal_after"]]
    tested = sum(r["connect"]["n_tested"] for r in rows)
    ratio = [r["cost_after"] / r["cost_before"] for r in both]
    share = [r["connect"]["ms"] / r["ms_plan"] for r in rows if r["ms_plan"] > 0]
    return dict(queries=n,
                goal_rate_before=sum(r["goal_before"] for r in rows) / n,
                goal_rate_after=sum(r["goal_after"] for r in rows) / n,
                rescued=sum(1 for r in rows if r["goal_after"] and not r["goal_before"]),
                solved_by_both=len(both),
                cost_mean_before=statistics.fmean(r["cost_before"] for r in both) if both else None,
                cost_mean_after=statistics.fmean(r["cost_after"] for r in both) if both else None,
                cost_ratio_median=statistics.median(ratio) if ratio else None,
                improved_share=sum(1 for r in rows if r["connect"]["status"] == _lib.CONNECT_OK
                                   and r["goal_before"]) / n,
                valid_over_tested=sum(r["connect"]["n_valid"] for r in rows) / tested
                if tested else None,
                eligible_mean=statistics.fmean(r["connect"]["n_eligible"] for r in rows),
                status3_before=sum(1 for r in rows if r["status_before"] == 3),
                status3_after=sum(1 for r in rows if r["status_after"] == 3),
                connect_ms_mean=statistics.fmean(r["connect"]["ms"] for r in rows),
                plan_ms_mean=statistics.fmean(r["ms_plan"] for r in rows),
                connect_share_of_plan_mean=statistics.fmean(share) if share else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--candidates", default="1024,65536")
    ap.add_argument("--passes", default="1,8")
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "connect_quality.json"))
    args = ap.parse_args()
    eng = _lib.Engine(0)
    out = {}

    def flush():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    c3, c5 = bench.WORKLOADS["c3"], bench.WORKLOADS["c5"]
    q3 = bench.make_query(1234, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"], engine=eng)
    qs = [bench.make_query(4321 + j, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"],
                           engine=eng) for j in range(args.queries)]
    q5 = None if args.no_c5 else bench.make_query(1234, n_obs=0, mode=c5["mode"], mass=c5["mass"],
                                                  engine=eng, n_mesh=c5["meshes"])
    for K in [int(x) for x in args.candidates.split(",")]:
        for passes in [int(x) for x in args.passes.split(",")]:
            rec = out["K%d_passes%d" % (K, passes)] = dict(candidates=K, passes=passes, sets={})
            record(eng, args, K, passes, rec["sets"], c3, c5, q3, qs, q5, flush)


def record(eng, args, K, passes, sets, c3, c5, q3, qs, q5, flush):
    for batch in (c3["batch"], c3["alt_batch"]):
        rows = [one(eng, q3, c3["samples"], batch, 1234 + s, c3["mode"], c3["mass"],
                    K, passes) for s in range(args.steps)]
        sets["c3_steps_B%d" % batch] = dict(summary=summary(rows), queries=rows)
        print("K", K, "passes", passes, "c3_steps_B%d" % batch, json.dumps(summary(rows)), flush=True)
        flush()
        rows = [one(eng, q, c3["samples"], batch, 977 + 31 * j, c3["mode"], c3["mass"],
                    K, passes) for j, q in enumerate(qs)]
        sets["c3_queries_B%d" % batch] = dict(summary=summary(rows), queries=rows)
        print("K", K, "passes", passes, "c3_queries_B%d" % batch, json.dumps(summary(rows)), flush=True)
        flush()
    if q5 is not None:
        n5 = c5["samples"] // c5["fleet"]
        rows = [one(eng, q5, n5, c5["batch"], 1234, c5["mode"], c5["mass"], K, passes)]
        sets["c5_tree"] = dict(summary=summary(rows), queries=rows)
        print("K", K, "passes", passes, "c5_tree", json.dumps(summary(rows)), flush=True)
        flush()


if __name__ == "__main__":
    main()
