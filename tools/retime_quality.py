#!/usr/bin/env python3
"""What torque-feasible retiming (tcmp_plan_retime) does to the bench's queries: per query, the
plan finished as usual and, when its validation failed (status 3), retimed -- the status after,
the slow-down s, the binding row and joint, the statically critical rows, the stage's device
time next to the same plan's ms_finish.  Queries: bench.py's own C3 scene and per-step seeds at
B = 262,144 and B = 65,536, one C4 step (64 queries, 1e5 samples each, B = 65,536), and C4's
first eight queries under the sample seeds 5000 + q of the suite's full-size fixture
(tests/golden/fullsize_c4.npz, which holds a status-3 query); bench.py is imported read-only.
A query that validates is retimed too (x = 1, rows untouched), for the stage's time on it.
usage: python tools/retime_quality.py [--steps N] [--out FILE]"""
import argparse
import collections
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from torque_constrained_motion_planning_amd import _lib  # noqa: E402


def one(eng, query, n_samples, batch, seed, mode, mass, max_scale):
    obs, pack, goal = query
    eng.set_scene(obs, pack)
    assert eng.plan_begin(bench.START, goal, mode, mass, 5.0, max_nodes=n_samples + 1,
                          max_batch=batch, seed=seed) == _lib.PLAN_OK
    eng.plan_run(n_samples, batch)
    r0 = eng.plan_finish()
    rec = dict(seed=seed, status=r0.status, n_traj=r0.n_traj, first_fail=r0.first_fail,
               ms_finish=r0.ms_finish)
    if r0.status not in (_lib.PLAN_OK, _lib.PLAN_VALIDATION_FAILED):
        return rec
    rt = eng.plan_retime(max_scale=max_scale)
    d = rt.as_dict()
    rec.update(rt_status=d.pop("status"), **{"rt_" + k: v for k, v in d.items()})
    rec["status_after"] = _lib.PLAN_OK if rt.status == _lib.RETIME_OK else r0.status
    return rec


def summary(rows):
    g = [r for r in rows if "rt_status" in r]
    failed = [r for r in g if r["status"] == _lib.PLAN_VALIDATION_FAILED]
    fixed = [r for r in failed if r["status_after"] == _lib.PLAN_OK]
    s = sorted(r["rt_s"] for r in fixed)
    ratio = [r["rt_ms"] / r["ms_finish"] for r in g if r["ms_finish"] > 0]
    return dict(queries=len(rows), with_trajectory=len(g), status3_before=len(failed),
                status3_to_0=len(fixed),
                rt_status_counts=dict(collections.Counter(str(r["rt_status"]) for r in failed)),
                s_min=s[0] if s else None, s_median=statistics.median(s) if s else None,
                s_max=s[-1] if s else None,
                n_static_counts=dict(collections.Counter(str(r["rt_n_static"]) for r in failed)),
                bind_joint_counts=dict(collections.Counter(str(r["rt_bind_joint"]) for r in failed)),
                rt_ms_mean=statistics.fmean(r["rt_ms"] for r in g) if g else None,
                rt_ms_mean_status3=statistics.fmean(r["rt_ms"] for r in failed) if failed else None,
                ms_finish_mean=statistics.fmean(r["ms_finish"] for r in g) if g else None,
                rt_over_finish_mean=statistics.fmean(ratio) if ratio else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--max-scale", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join("profiles", "retime_quality.json"))
    args = ap.parse_args()
    eng = _lib.Engine(0)
    out = dict(max_scale=args.max_scale, sets={})
    c3, c4 = bench.WORKLOADS["c3"], bench.WORKLOADS["c4"]
    q3 = bench.make_query(1234, n_obs=c3["boxes"], mode=c3["mode"], mass=c3["mass"], engine=eng)
    for batch in (c3["batch"], c3["alt_batch"]):
        rows = [one(eng, q3, c3["samples"], batch, 1234 + s, c3["mode"], c3["mass"],
                    args.max_scale) for s in range(args.steps)]
        out["sets"]["c3_B%d" % batch] = dict(summary=summary(rows), queries=rows)
    rows = []
    for j in range(c4["queries"]):
        q = bench.make_query(1234 + j, n_obs=c4["boxes"], mode=c4["mode"], mass=c4["mass"],
                             engine=eng)
        rows.append(one(eng, q, c4["samples"], c4["batch"], 1234 + 7919 * j, c4["mode"],
                        c4["mass"], args.max_scale))
    out["sets"]["c4_step0"] = dict(summary=summary(rows), queries=rows)
    rows = []
    for j in range(8):
        q = bench.make_query(1234 + j, n_obs=c4["boxes"], mode=c4["mode"], mass=c4["mass"],
                             engine=eng)
        rows.append(one(eng, q, c4["samples"], c4["batch"], 5000 + j, c4["mode"], c4["mass"],
                        args.max_scale))
    out["sets"]["c4_fixture_seeds"] = dict(summary=summary(rows), queries=rows)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for k, v in out["sets"].items():
        print(k, json.dumps(v["summary"]))


if __name__ == "__main__":
    main()
