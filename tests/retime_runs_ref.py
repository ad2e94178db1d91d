"""Restatement of the per-run torque-feasible retiming (include/tcmp.h tcmp_minjerk_runs,
tcmp_retime_runs_traj), the oracle of tests/test_retime_runs_host.py and
tests/test_gpu_retime_runs.py.  The rest rule is repair_ref.waypoint_velocity's, the per-run
decision is retime_ref.retime on the run's rows, and the warp is the definition in numpy fp64."""
import numpy as np

import repair_ref as RP
import retime_ref as RT

OK, INFEASIBLE, OVER_CAP, UNVERIFIED, NOT_APPLICABLE = range(5)


def runs(P, ni, gates=None):
    """Row offsets (n_runs + 1) of the runs between rest waypoints: interior waypoints whose
    gate is closed or whose seven velocities are all 0.0."""
    P = RP._rows(P)
    W = len(P)
    assert W >= 2 and ni >= 1
    off = [0]
    for w in range(1, W - 1):
        closed = gates is not None and gates[w] == 0
        if closed or not RP.waypoint_velocity(P, w).any():
            off.append(w * ni)
    off.append((W - 1) * ni)
    return np.array(off, dtype=np.int64)


def warp(psg, off, s):
    """The continuous piecewise-linear time warp -> (psg', O): knots at the rows off[k] - 1; a
    run with s_k == 1 whose origin did not move keeps its bits."""
    psg = np.asarray(psg, dtype=np.float64)
    out = psg.copy()
    o = [psg[0 if off[k] == 0 else off[k] - 1] for k in range(len(off) - 1)]
    big = []
    for k in range(len(off) - 1):
        big.append(o[0] if k == 0 else big[k - 1] + (o[k] - o[k - 1]) * s[k - 1])
        if not (s[k] == 1.0 and big[k] == o[k]):
            a, b = off[k], off[k + 1]
            out[a:b] = big[k] + (psg[a:b] - o[k]) * s[k]
    return out, np.array(big)


def retime_runs(q, v, a, off, mode, mass, psg=None, min_scale=1.0, max_scale=0.0, exec_time=0.0):
    """The definition -> (list of per-run dicts, result dict).  A per-run dict is
    retime_ref.retime's on the run's rows with absolute bind_row / first_fail and the run's
    status (OK, INFEASIBLE or OVER_CAP); the result holds tcmp_retime_runs_result's fields and,
    when OK, the scaled rows "qd", "qdd", "psg"."""
    q, v, a = RT._rows(q), RT._rows(v), RT._rows(a)
    n = len(q)
    off = np.asarray(off, dtype=np.int64)
    nr = len(off) - 1
    assert (n == 0 and nr <= 0) or (off[0] == 0 and off[-1] == n and (np.diff(off) > 0).all())
    x_max = 1.0 / (min_scale * min_scale)
    res = dict(status=OK, n_scaled=0, n_rows=n, n_runs=max(nr, 0), fail_run=-1,
               first_fail_before=-1, first_fail_after=-1, x_min=0.0, time_ratio=0.0,
               exec_time_after=0.0)
    if n == 0:
        res.update(x_min=x_max, time_ratio=1.0)
        return [], res
    per = []
    for k in range(nr):
        b, e = int(off[k]), int(off[k + 1])
        r = RT.retime(q[b:e], v[b:e], a[b:e], mode, mass, min_scale=min_scale,
                      max_scale=max_scale)
        r["row_begin"], r["row_end"] = b, e
        r["first_fail"] = r["first_fail_before"] + b if r["first_fail_before"] >= 0 else -1
        if r["bind_row"] >= 0:
            r["bind_row"] += b
        if r["status"] == UNVERIFIED:
            r["status"] = OK   # (the overall validation below decides)
        r["t_begin"] = 0.0
        per.append(r)
    ffs = [r["first_fail"] for r in per if r["first_fail"] >= 0]
    res["first_fail_before"] = res["first_fail_after"] = min(ffs) if ffs else -1
    for st in (INFEASIBLE, OVER_CAP):
        bad = [k for k, r in enumerate(per) if r["status"] == st]
        if bad:
            res.update(status=st, fail_run=bad[0])
            return per, res
    s = [r["s"] for r in per]
    qd, qdd = v.copy(), a.copy()
    total = 0.0
    for k, r in enumerate(per):
        b, e = r["row_begin"], r["row_end"]
        qd[b:e] = v[b:e] * r["r"]
        qdd[b:e] = a[b:e] * r["x"]
        total += r["s"] * float(e - b)
    res.update(x_min=min(r["x"] for r in per), n_scaled=sum(r["x"] != 1.0 for r in per),
               time_ratio=total / float(n), qd=qd, qdd=qdd, psg=None)
    res["exec_time_after"] = exec_time * res["time_ratio"]
    if psg is not None:
        res["psg"], big = warp(psg, off, s)
        for k, r in enumerate(per):
            r["t_begin"] = float(big[k])
    res["first_fail_after"] = RT.first_fail(q, qd, qdd, mode, mass)
    if res["first_fail_after"] >= 0:
        res["status"] = UNVERIFIED
    return per, res
