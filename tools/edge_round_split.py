#!/usr/bin/env python3
"""k_fl_edges' launches of a rocprofv3 kernel trace, split by the round they belong to: a fused
query of R rounds launches the kernel R times, so with one fleet at a time (bench.py
--pipeline 1) launch i of the trace is round i % R.  Round 1 walks the rays from the root (most
of a query's edge steps); the later rounds' edges are short.

usage: python tools/edge_round_split.py RUN_kernel_trace.csv [ROUNDS=4] [KERNEL=k_fl_edges]
"""
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pmc_summary import short  # noqa: E402


def main():
    path = sys.argv[1]
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    kern = sys.argv[3] if len(sys.argv) > 3 else "k_fl_edges"
    ks = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
                for r in csv.DictReader(open(path)) if short(r["Kernel_Name"]) == kern)
    ms = [(b - a) * 1e-6 for a, b in ks]
    total = sum(ms)
    out = {"kernel": kern, "launches": len(ms), "rounds": rounds, "total_ms": total, "per_round": []}
    for r in range(rounds):
        x = ms[r::rounds]
        out["per_round"].append({"round": r + 1, "n": len(x), "avg_ms": sum(x) / len(x) if x else None,
                                 "min_ms": min(x) if x else None, "max_ms": max(x) if x else None,
                                 "share": sum(x) / total if total else None})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
