"""Restatement of the torque-feasible retiming stage (include/tcmp.h tcmp_retime_traj), the
oracle of tests/test_retime_host.py and tests/test_gpu_retime.py.  Torques are the CPU oracle's
(oracle.rne, oracle.dyn_tau); everything else is the definition, in numpy fp64."""
import numpy as np

import oracle as O

OK, INFEASIBLE, OVER_CAP, UNVERIFIED, NOT_APPLICABLE = range(5)
LIMITS = np.array([87.0, 87.0, 87.0, 87.0, 12.0, 12.0])   # joint 7 is never tested
EPS = 1e-9   # N m, the guard on the limit: the tolerance the RNE is pinned at
BASE, NOV, RNE, DYN = range(4)


def _rows(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).reshape(-1, 7)


def torques(q, v, a, mode, mass):
    """(g, tau), (n, 6) each: the static and the full torques of the six tested joints as the
    mode's test sees them."""
    q, v, a = _rows(q), _rows(v), _rows(a)
    n = len(q)
    z = np.zeros_like(q)
    if mode == BASE or n == 0:
        return np.zeros((n, 6)), np.zeros((n, 6))
    if mode in (NOV, RNE):
        m = mass if mass > 0.01 else 0.0
        g = O.rne(q, z, z, m)
        tau = g.copy() if mode == NOV else O.rne(q, v, a, m)
    else:
        g = np.array([O.dyn_tau(q[i], None, None, mass) for i in range(n)])
        tau = np.array([O.dyn_tau(q[i], v[i], a[i], mass) for i in range(n)])
    return g[:, :6].copy(), tau[:, :6].copy()


def bounds(g, tau):
    """ub, lb (n, 6) of the definition."""
    d = tau - g
    L = np.broadcast_to(LIMITS, g.shape)
    ub = np.where(np.abs(g) < L, np.inf, -np.inf)
    lb = np.where(np.abs(g) < L, 0.0, np.inf)
    nz = d != 0
    sg = np.where(d > 0, g, -g)
    with np.errstate(divide="ignore", invalid="ignore"):
        ub = np.where(nz, ((L - EPS) - sg) / np.abs(d), ub)
        lb = np.where(nz, (-(L - EPS) - sg) / np.abs(d), lb)
    return ub, lb


def first_fail(q, v, a, mode, mass):
    """The final validation (rrt_star.py:208-210) with the oracle's torque test: the first
    failing row or -1."""
    q, v, a = _rows(q), _rows(v), _rows(a)
    for i in range(len(q)):
        if not O.torque_ok(q[i], mode, mass, v[i], a[i]):
            return i
    return -1


def retime(q, v, a, mode, mass, psg=None, min_scale=1.0, max_scale=0.0, exec_time=0.0):
    """The definition -> dict of tcmp_retime_result's fields, plus (OK only) the scaled rows
    "qd", "qdd", "psg" and the second-lowest ub, "ub2" (the margin of the binding row)."""
    q, v, a = _rows(q), _rows(v), _rows(a)
    n = len(q)
    min_scale = 1.0 if min_scale == 0 else float(min_scale)
    assert 0 < min_scale <= 1 and (max_scale == 0 or max_scale >= 1)
    g, tau = torques(q, v, a, mode, mass)
    r = dict(n_rows=n, bind_row=-1, bind_joint=-1, n_static=0, x=0.0, r=0.0, s=0.0,
             exec_time_after=0.0)
    if mode == BASE or n == 0:
        x_hi, x_lo, ub2 = np.inf, 0.0, np.inf
    else:
        ub, lb = bounds(g, tau)
        x_hi = float(ub.min())
        x_lo = max(0.0, float(lb.max()))
        flat = np.sort(ub.reshape(-1))
        ub2 = float(flat[1])
        if x_hi < np.inf:
            k = int(np.argmax(ub.reshape(-1) == x_hi))   # lowest row, then lowest joint
            r["bind_row"], r["bind_joint"] = k // 6, k % 6
        r["n_static"] = int((np.abs(g) >= LIMITS - EPS).any(axis=1).sum())
    r.update(x_hi=x_hi, x_lo=x_lo, ub2=ub2)
    r["first_fail_before"] = r["first_fail_after"] = first_fail(q, v, a, mode, mass)
    x_max = 1.0 / (min_scale * min_scale)
    x = min(x_max, x_hi)
    if x >= 1.0 and min_scale == 1.0:
        x = 1.0
    if x <= 0 or x < x_lo:
        r["status"] = INFEASIBLE
        return r
    if max_scale > 0 and x < 1.0 / (max_scale * max_scale):
        r["status"] = OVER_CAP
        return r
    rr = float(np.sqrt(np.float64(x)))
    s = 1.0 / rr
    r.update(status=OK, x=x, r=rr, s=s, exec_time_after=s * exec_time)
    r["qd"], r["qdd"] = v * rr, a * x
    r["psg"] = None if psg is None else np.asarray(psg, dtype=np.float64) * s
    r["first_fail_after"] = first_fail(q, r["qd"], r["qdd"], mode, mass)
    if r["first_fail_after"] >= 0:
        r["status"] = UNVERIFIED
    return r


def all_pass(q, v, a, mode, mass):
    """oracle.torque_ok on every row."""
    return first_fail(q, v, a, mode, mass) < 0


def binding_torque(q, v, a, mode, mass, row, joint):
    """The oracle's torque of (row, joint) on the given rows."""
    _, tau = torques(_rows(q)[row:row + 1], _rows(v)[row:row + 1], _rows(a)[row:row + 1], mode,
                     mass)
    return float(tau[0, joint])
