"""Restatement of the torque-limited velocity-profile retiming (include/tcmp.h
tcmp_retime_profile_traj), the oracle of tests/test_retime_profile_host.py and
tests/test_gpu_retime_profile.py.  Torques are the CPU oracle's, as in tests/retime_ref.py;
everything else is the definition, in numpy fp64, one IEEE operation per arithmetic sign (numpy
never contracts a multiply and an add).  sweep() takes the coefficients as given, so the device's
own (coef_out) can be fed to it."""
import numpy as np

import oracle as O
import retime_ref as RT

OK, INFEASIBLE, OVER_CAP, UNVERIFIED, NOT_APPLICABLE = range(5)
LIMITS = RT.LIMITS
EPS = RT.EPS
LG = LIMITS - EPS
INF = np.inf


def coefficients(q, v, a, mode, mass):
    """(n, 18): g = T(q, 0, 0), m = T(q, 0, v) - g, d = T(q, v, a) - g of the six tested joints
    as the mode's test sees them."""
    q, v, a = RT._rows(q), RT._rows(v), RT._rows(a)
    z = np.zeros_like(q)
    g, tm = RT.torques(q, z, v, mode, mass)
    _, td = RT.torques(q, v, a, mode, mass)
    return np.hstack([g, tm - g, td - g])


def joint_bounds(g, d):
    """The uniform retiming's ub / lb of every (row, joint) from g and d = tau - g (tcmp.h;
    csrc/tcmp_stage.h rt_interval)."""
    g, d = np.asarray(g, dtype=np.float64), np.asarray(d, dtype=np.float64)
    L = np.broadcast_to(LIMITS, g.shape)
    inside = np.abs(g) < L
    ub = np.where(inside, INF, -INF)
    lb = np.where(inside, 0.0, INF)
    nz = d != 0
    sg = np.where(d > 0, g, -g)
    with np.errstate(divide="ignore", invalid="ignore"):
        ub = np.where(nz, ((L - EPS) - sg) / np.abs(d), ub)
        lb = np.where(nz, (-(L - EPS) - sg) / np.abs(d), lb)
    bad = np.isnan(ub) | np.isnan(lb)
    return np.where(bad, -INF, ub), np.where(bad, INF, lb)


def uniform(g, d, min_scale=1.0, max_scale=0.0):
    """tcmp_retime_traj's decision on the rows' (g, d) -> (status, x or 0.0)."""
    x_max = 1.0 / (min_scale * min_scale)
    if len(g):
        ub, lb = joint_bounds(g, d)
        x_hi, x_lo = float(ub.min()), max(0.0, float(lb.max()))
    else:
        x_hi, x_lo = INF, 0.0
    x = min(x_max, x_hi)
    if x >= 1.0 and min_scale == 1.0:
        x = 1.0
    if not x > 0.0 or x < x_lo:
        return INFEASIBLE, 0.0
    if max_scale > 0 and x < 1.0 / (max_scale * max_scale):
        return OVER_CAP, 0.0
    return OK, x


def row_lines(c):
    """A row's 18 coefficients -> (P, S, p, s, ub, lb): the joint lines p - s x <= u <= P - S x
    (joints with m != 0) and the direct bounds on x of the others (+inf / 0 without any)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g, m, d = c[0:6], c[6:12], c[12:18]
        nan = np.isnan(g) | np.isnan(m) | np.isnan(d)
        line = (m != 0) & ~nan
        A = np.abs(m[line])
        sg = np.where(m[line] > 0, g[line], -g[line])
        sd = np.where(m[line] > 0, d[line], -d[line])
        P, p, S = (LG[line] - sg) / A, (-LG[line] - sg) / A, sd / A
        ub, lb = joint_bounds(g, d)
        ub = np.where(nan, -INF, ub)[~line]
        lb = np.where(nan, INF, lb)[~line]
    return P, S, p, S.copy(), (ub.min() if len(ub) else INF), (lb.max() if len(lb) else 0.0)


def row_set(c, link, x_max, x_floor):
    """One step of the backward pass: the x of row i from which some u reaches the next row's
    set.  link: None (last row) or (hi_next, lo_next, 2 delta).  -> (hi, lo) before anchoring."""
    P, S, p, s, ub, lb = row_lines(c)
    if link is not None:
        hn, ln, dd = link
        P, S = np.append(P, hn / dd), np.append(S, 1.0 / dd)
        p, s = np.append(p, ln / dd), np.append(s, 1.0 / dd)
    hi, lo = min(x_max, ub), max(x_floor, lb)
    if len(P) and len(p):
        with np.errstate(divide="ignore", invalid="ignore"):
            cc = S[:, None] - s[None, :]
            ee = P[:, None] - p[None, :]
            b = ee / cc
        if (cc > 0).any():      # (fmin / fmax: a NaN quotient binds nothing, as on the device)
            hi = float(np.fmin(hi, np.fmin.reduce(b[cc > 0])))
        if (cc < 0).any():
            lo = float(np.fmax(lo, np.fmax.reduce(b[cc < 0])))
        if ((cc == 0) & (ee < 0)).any():
            hi = -INF
    return float(hi), float(lo)


def sweep(coef, psg=None, min_scale=1.0, max_scale=0.0):
    """The definition on given coefficients (n, 18) -> dict of tcmp_retime_profile_result's
    fields (first_fail_* aside), plus hi, lo (the reachable sets) and, unless INFEASIBLE, x, u
    and psg (the warped times; from 0 in unit steps without psg)."""
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64)).reshape(-1, 18)
    n = len(coef)
    min_scale = 1.0 if min_scale == 0 else float(min_scale)
    x_max = 1.0 / (min_scale * min_scale)
    t = np.arange(n, dtype=np.float64) if psg is None else np.asarray(psg, dtype=np.float64)
    dl = t[1:] - t[:-1]
    assert (dl > 0).all()
    ust, x_u = uniform(coef[:, 0:6], coef[:, 12:18], min_scale, max_scale)
    anchored = ust == OK
    x_floor = x_u if anchored else (1.0 / (max_scale * max_scale) if max_scale > 0 else 1e-6)
    r = dict(status=OK, anchored=int(anchored), uniform_status=ust, n_rows=n, fail_row=-1,
             x_uniform=x_u, x_floor=x_floor, x_min=0.0, n_at_floor=0, n_at_cap=0,
             time_before=float(t[-1] - t[0]) if n else 0.0, time_after=0.0, time_uniform=0.0)
    if n == 0:
        r["x_min"] = x_max
        return r
    hi, lo = np.zeros(n), np.zeros(n)
    for i in range(n - 1, -1, -1):
        link = None if i == n - 1 else (hi[i + 1], lo[i + 1], 2.0 * dl[i])
        h, l = row_set(coef[i], link, x_max, x_floor)
        if anchored:
            h, l = max(h, x_floor), x_floor
        elif not l <= h:
            r.update(status=INFEASIBLE, fail_row=i)
            return r
        hi[i], lo[i] = h, l
    x, u = np.zeros(n), np.zeros(n)
    x[0] = hi[0]
    for i in range(n):
        P, S, p, s, _, _ = row_lines(coef[i])
        U = float((P - S * x[i]).min()) if len(P) else INF
        W = float((p - s * x[i]).max()) if len(p) else -INF
        if i < n - 1:
            dd = 2.0 * dl[i]
            tt = min(U, (hi[i + 1] - x[i]) / dd)
            x[i + 1] = min(hi[i + 1], max(lo[i + 1], x[i] + dd * tt))
            u[i] = (x[i + 1] - x[i]) / dd
        else:
            u[i] = min(U, max(0.0, W))
    rr = np.sqrt(x)
    tp, tu = np.zeros(n), t[0]
    tp[0] = t[0]
    ru = np.sqrt(np.float64(x_u)) if anchored else 0.0
    for i in range(n - 1):
        dd = 2.0 * dl[i]
        tp[i + 1] = tp[i] + dd / (rr[i] + rr[i + 1])
        if anchored:
            tu = tu + dd / (ru + ru)
    r.update(hi=hi, lo=lo, x=x, u=u, psg=tp, x_min=float(x.min()),
             n_at_floor=int((x == x_floor).sum()), n_at_cap=int((x == x_max).sum()),
             time_after=float(tp[-1] - tp[0]), time_uniform=float(tu - t[0]) if anchored else 0.0)
    return r


def apply_rows(v, a, x, u):
    """qd', qdd' of the definition: a row with x = 1 and u = 0 is copied; else qd' = qd sqrt(x),
    qdd' = qdd x + qd u with both products rounded before the add."""
    v, a = RT._rows(v), RT._rows(a)
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    keep = ((x == 1.0) & (u == 0.0))[:, None]
    return (np.where(keep, v, v * np.sqrt(x)[:, None]),
            np.where(keep, a, a * x[:, None] + v * u[:, None]))


def retime_profile(q, v, a, mode, mass, psg=None, min_scale=1.0, max_scale=0.0):
    """The whole stage with the oracle's torques: sweep()'s dict plus first_fail_before /
    first_fail_after, "coef", and (OK only) the new rows "qd", "qdd"."""
    q, v, a = RT._rows(q), RT._rows(v), RT._rows(a)
    coef = coefficients(q, v, a, mode, mass)
    r = sweep(coef, psg, min_scale, max_scale)
    r["coef"] = coef
    r["first_fail_before"] = r["first_fail_after"] = RT.first_fail(q, v, a, mode, mass)
    if r["status"] != OK or len(q) == 0:
        if r["status"] == OK:
            r["first_fail_after"] = -1
        return r
    qd, qdd = apply_rows(v, a, r["x"], r["u"])
    r["first_fail_after"] = RT.first_fail(q, qd, qdd, mode, mass)
    if r["first_fail_after"] >= 0:
        r["status"] = UNVERIFIED
    else:
        r["qd"], r["qdd"] = qd, qdd
    return r


def half_planes(c, link, x_max, x_floor):
    """Row i's constraints as rows (a_u, a_x, b) of a_u u + a_x x <= b, for an LP solver: the
    joint lines, the link lines, the direct bounds and [x_floor, x_max]."""
    P, S, p, s, ub, lb = row_lines(c)
    if link is not None:
        hn, ln, dd = link
        P, S = np.append(P, hn / dd), np.append(S, 1.0 / dd)
        p, s = np.append(p, ln / dd), np.append(s, 1.0 / dd)
    rows = [(1.0, Sk, Pk) for Pk, Sk in zip(P, S)] + [(-1.0, -sj, -pj) for pj, sj in zip(p, s)]
    rows += [(0.0, 1.0, min(x_max, ub)), (0.0, -1.0, -max(x_floor, lb))]
    return np.array(rows)
