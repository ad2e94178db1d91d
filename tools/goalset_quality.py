#!/usr/bin/env python3
"""What the goal-set connection (tcmp_connect_goal_set) buys over the single-goal stage
(tcmp_connect_nodes) on the bench's queries.  Each query is planned once; its tree is fetched and
both stages run on that same tree in their stand-alone form with the bound the plan form uses
(the goal node's cost, or none), so neither changes the tree and every setting sees the same
input.  The goal set is the query goal first, then the nearest feasible IK images of its pose
from Engine.goal_search, 8 and 64 goals in all (and, for the stage's time at a full 64 goals
whatever the pose offers, the goal with 63 uniform configurations: "setrand64").  Per setting:
goal rate, rescued queries, cost before / after, winners by goal index, valid / tested, and the
stage's device ms beside the single-goal stage's on the same tree (that one is the baseline).
Queries: tools/connect_quality.py's (bench.py's C3 scene under per-step seeds and a seeded set of
further 16-box queries, each at B = 262,144 and B = 65,536) and one C5-size tree.
usage: python tools/goalset_quality.py [--steps N] [--queries N] [--no-c5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from torque_constrained_motion_planning_amd import _lib  # noqa: E402
from torque_constrained_motion_planning_amd.ik import (JOINT_LOWER, JOINT_UPPER,  # noqa: E402
                                                       free_grid)

SETTINGS = ((1024, 1), (65536, 1), (65536, 8))
SET_SIZES = (8, 64)


def goal_sets(eng, goal, mode, mass):
    """{n: the query goal, then the nearest feasible images of its pose, n rows at most}"""
    goal = np.asarray(goal, dtype=np.float64)
    q, _, _, _, st = eng.goal_search(eng.fk([goal]), free_grid(goal[6], 256), bench.START, mode,
                                     mass, max_out=max(SET_SIZES))
    rest = [r for r in q[0, :st[0].n_out] if np.abs(r - goal).max() > 1e-6]
    return {n: np.array([goal] + rest[:n - 1]) for n in SET_SIZES}, st[0].n_feasible


KEEP = ("status", "passes_run", "n_eligible", "n_tested", "n_valid", "rank", "parent", "cost_after",
        "goal_index", "ms")


def slim(r):
    """the fields of a result record that the summary and the table need"""
    return {k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items() if k in KEEP}


RUN_FIELDS = ["status", "goal_index", "rank", "n_tested", "n_valid", "cost_after", "ms"]


def compact(q):
    """a query's row for the file: each run as the list of its RUN_FIELDS"""
    runs = {key: {w: [r.get(k) if not isinstance(r.get(k), float) else round(r[k], 4)
                      for k in RUN_FIELDS] for w, r in rec.items()}
            for key, rec in q["runs"].items()}
    return dict(q, runs=runs)


def write(out, path):
    """one line per summary and per query (the record stays small enough to read)"""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (name, rec) in enumerate(out.items()):
            f.write(' %s: {\n  "summary": {\n' % json.dumps(name))
            keys = list(rec["summary"].items())
            for j, (key, s) in enumerate(keys):
                f.write("   %s: {\n" % json.dumps(key))
                f.write(",\n".join("    %s: %s" % (json.dumps(w), json.dumps(v))
                                   for w, v in s.items()))
                f.write("\n   }%s\n" % ("," if j + 1 < len(keys) else ""))
            f.write('  },\n  "run_fields": %s,\n  "queries": [\n' % json.dumps(RUN_FIELDS))
            f.write(",\n".join("   " + json.dumps(compact(q)) for q in rec["queries"]))
            f.write("\n  ]\n }%s\n" % ("," if i + 1 < len(out) else ""))
        f.write("}\n")


def one(eng, query, n_samples, batch, seed, mode, mass):
    obs, pack, goal = query
    eng.set_scene(obs, pack)
    assert eng.plan_begin(bench.START, goal, mode, mass, 5.0, max_nodes=n_samples + 2,
                          max_batch=batch, seed=seed) == _lib.PLAN_OK
    eng.plan_run(n_samples, batch)
    r0 = eng.plan_finish()
    cfg, cost, _, n = eng.plan_tree(int(r0.n_nodes))
    bound = float(cost[r0.goal_node]) if r0.goal_found else np.inf
    sets, n_feasible = goal_sets(eng, goal, mode, mass)
    # the stage's time at a full 64 goals wherever the pose has fewer images (C5's has none but
    # the goal): the goal, then 63 uniform configurations inside the limits -- timing only
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(JOINT_LOWER, dtype=np.float64), np.asarray(JOINT_UPPER, dtype=np.float64)
    sets["rand64"] = np.concatenate([np.asarray(goal, dtype=np.float64)[None],
                                     lo + (hi - lo) * rng.random((63, 7))])
    row = dict(seed=seed, n_nodes=int(n), goal_before=bool(r0.goal_found),
               cost_before=bound if r0.goal_found else None, n_feasible_images=int(n_feasible),
               set_sizes={str(k): len(v) for k, v in sets.items()}, runs={})
    for K, p in SETTINGS:
        s = eng.connect_nodes(cfg, cost, goal, mode, mass, bound=bound, max_candidates=K,
                              passes=p)["result"]
        rec = dict(single=slim(s.as_dict()))
        for k, G in sets.items():
            o = eng.connect_goal_set(cfg, cost, G, mode, mass, bound=bound, max_candidates=K,
                                     passes=p)
            rec["set%s" % k] = dict(slim(o["result"].as_dict()),
                                    tested_goals=int((o["per_goal"][1] > 0).sum()),
                                    valid_goals=int((o["per_goal"][2] > 0).sum()))
        row["runs"]["K%d_passes%d" % (K, p)] = rec
    return row


def summary(rows, key, which):
    n = len(rows)
    rs = [r["runs"][key][which] for r in rows]
    ok = [x["status"] == _lib.CONNECT_OK for x in rs]
    after = [r["goal_before"] or o for r, o in zip(rows, ok)]
    # (the stand-alone form knows no goal node: without a winner the cost stays the plan's)
    both = [(r["cost_before"], x["cost_after"] if o else r["cost_before"])
            for r, x, o in zip(rows, rs, ok) if r["goal_before"]]
    tested = sum(x["n_tested"] for x in rs)
    winners = {}
    for x, o in zip(rs, ok):
        if o:
            j = str(x.get("goal_index", 0))
            winners[j] = winners.get(j, 0) + 1
    return dict(queries=n, goal_rate_before=sum(r["goal_before"] for r in rows) / n,
                goal_rate_after=sum(after) / n,
                rescued=sum(1 for r, o in zip(rows, ok) if o and not r["goal_before"]),
                improved=sum(1 for r, o in zip(rows, ok) if o and r["goal_before"]),
                cost_mean_before=statistics.fmean(b for b, _ in both) if both else None,
                cost_mean_after=statistics.fmean(a for _, a in both) if both else None,
                rescued_cost_mean=(statistics.fmean(x["cost_after"] for r, x, o in zip(rows, rs, ok)
                                                    if o and not r["goal_before"])
                                   if any(o and not r["goal_before"] for r, o in zip(rows, ok))
                                   else None),
                winners_by_goal_index=winners,
                valid_over_tested=sum(x["n_valid"] for x in rs) / tested if tested else None,
                ms_mean=statistics.fmean(x["ms"] for x in rs))


def summaries(rows):
    return {key: {w: summary(rows, key, w) for w in rows[0]["runs"][key]}
            for key in rows[0]["runs"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "goalset_quality.json"))
    args = ap.parse_args()
    eng = _lib.Engine(0)
    out = {}
    c3, c5 = bench.WORKLOADS["c3"], bench.WORKLOADS["c5"]
    q3 = bench.make_query(1234, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"], engine=eng)
    qs = [bench.make_query(4321 + j, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"],
                           engine=eng) for j in range(args.queries)]

    def record(name, rows):
        out[name] = dict(summary=summaries(rows), queries=rows)
        for key, s in out[name]["summary"].items():
            for w, v in s.items():
                print(name, key, w, json.dumps(v), flush=True)
        write(out, args.out)

    for batch in (c3["batch"], c3["alt_batch"]):
        record("c3_steps_B%d" % batch,
               [one(eng, q3, c3["samples"], batch, 1234 + s, c3["mode"], c3["mass"])
                for s in range(args.steps)])
        record("c3_queries_B%d" % batch,
               [one(eng, q, c3["samples"], batch, 977 + 31 * j, c3["mode"], c3["mass"])
                for j, q in enumerate(qs)])
    if not args.no_c5:
        q5 = bench.make_query(1234, n_obs=0, mode=c5["mode"], mass=c5["mass"], engine=eng,
                              n_mesh=c5["meshes"])
        record("c5_tree", [one(eng, q5, c5["samples"] // c5["fleet"], c5["batch"], 1234,
                               c5["mode"], c5["mass"])])


if __name__ == "__main__":
    main()
