"""Writes tests/golden/torque_limits.npz: configurations whose deciding torque sits a chosen
margin from its limit in the high-precision restatement tests/torque_ref.py (layout: its Fixture).

    python tests/golden/gen_torque_limits.py [--out PATH]

CPU only, deterministic (one fixed seed per group, arrays reproduce one for one).  A *base* is a
row (q, qd, qdd0, mode, mass, joint j, sign of tau_j) with a bracket on one scalar x -- joint j's
own angle for a static row, a factor on qdd0 for a dynamic one, the far end's angle j for an edge
-- found by random search; its *variants* are the values of x that bisection (to adjacent fp64
values) puts at |tau_j| - L_j = +delta (fails) and -delta (passes) for each level delta.  A base
is kept only if every variant obeys the construction rules: q inside the joint limits by 1e-3,
the deciding torque of the wanted sign, every other tested joint at least 0.5 Nm inside.

Levels: 1e-6, 1e-9 and delta_min, the smallest power of ten >= 4 B; the band B is 64 times the
largest |oracle fp64 - restatement| over every row of the fixture (rows, goal rows, edge steps; mode
torques and tcmp_rne_batch's), found by iterating to a fixed point from 1e-11.  The oracle enters
nowhere else.  A subset of rows is recomputed at 50 digits; the largest difference from
longdouble is stored as ref_uncertainty.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torque_ref as TR  # noqa: E402

LD = np.longdouble
LIM = np.array(TR.EFFORT[:6])
INSIDE = 1e-3
QLO, QHI = TR.LO + 1.5 * INSIDE, TR.HI - 1.5 * INSIDE
PER_GROUP = 8
SPARE = 3                      # bases tried per kept one
SLACK = 0.1                    # Nm of clearance beyond CLEAR asked of a candidate
SIDES = (1, -1)
SEED = 20260911


def rng_of(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def rand_q(rng, n):
    return QLO + (QHI - QLO) * rng.random((n, 7))


def taus(q, qd, qdd, mode, mass):
    return TR.mode_torques(q, qd, qdd, mode, mass)


def others_inside(tau, joint, clear):
    """Every tested joint but `joint` (n,) at least `clear` inside -> (n,) bool."""
    m = np.asarray(TR.margins(tau), dtype=np.float64)
    m[np.arange(len(m)), joint] = -np.inf
    return (m <= -clear).all(axis=1)


def signed_g(tau, joint, sign):
    r = np.arange(len(tau))
    return sign * tau[r, joint] - LIM[joint]


# ---- bisection on rows ---------------------------------------------------------------------------
def bisect(g, lo, hi, target, pick_hi):
    """Rows of scalars with g(lo) < target <= g(hi) (rows violating it come back NaN), halved
    until lo and hi are adjacent fp64 values.  pick_hi (n,) bool: the end returned."""
    lo, hi = lo.copy(), hi.copy()
    target = target.astype(LD)
    bad = ~((g(lo) < target) & (g(hi) >= target))
    for _ in range(200):
        mid = lo + (hi - lo) / 2
        done = (mid == lo) | (mid == hi)
        if done.all():
            break
        up = g(mid) >= target
        hi = np.where(up & ~done, mid, hi)
        lo = np.where(~up & ~done, mid, lo)
    else:
        raise RuntimeError("bisection did not end")
    x = np.where(pick_hi, hi, lo)
    x[bad] = np.nan
    return x


def variants(levels):
    """(side, delta) of a base's variants, the order of the fixture's x columns."""
    return [(s, d) for d in levels for s in SIDES]


# ---- static bases ----------------------------------------------------------------------------------
def static_candidates(mode, mass, key, n):
    rng = rng_of(1, *key)
    q = rand_q(rng, n)
    tau = taus(q, None, None, mode, mass)
    return q, tau


def static_bases(q, tau, mode, mass, joint, sign, want, var=None):
    """Up to `want` brackets (q, x_below, x_above) on the angle of joint `var` (default: joint)."""
    var = joint if var is None else var
    jj = np.full(len(q), joint)
    g = np.asarray(signed_g(tau, jj, sign), dtype=np.float64)
    near = (np.abs(g) < 3.0) & (np.abs(g) > 1e-3) & others_inside(tau, jj, TR.CLEAR + SLACK)
    idx = np.nonzero(near)[0][:4 * want]
    out = []
    if not len(idx):
        return out
    steps = np.array([0.02, -0.02, 0.06, -0.06, 0.15, -0.15, 0.4, -0.4])
    alt = np.repeat(q[idx], len(steps), axis=0)
    alt[:, var] += np.tile(steps, len(idx))
    ok = (alt[:, var] >= QLO[var]) & (alt[:, var] <= QHI[var])
    alt[:, var] = np.clip(alt[:, var], QLO[var], QHI[var])
    ga = np.asarray(signed_g(taus(alt, None, None, mode, mass), np.full(len(alt), joint), sign),
                    dtype=np.float64).reshape(len(idx), len(steps))
    ok = ok.reshape(len(idx), len(steps))
    for r, i in enumerate(idx):
        for c in range(len(steps)):
            if ok[r, c] and ga[r, c] * g[i] < 0 and abs(ga[r, c]) > 1e-3:
                x0, x1 = q[i, var], alt[r * len(steps) + c, var]
                below, above = (x0, x1) if g[i] < 0 else (x1, x0)
                out.append((q[i].copy(), below, above))
                break
        if len(out) == want:
            break
    return out


def solve_static(bases, mode, mass, joint, sign, levels, var=None, clear=TR.CLEAR):
    """-> [(q, x (V,), margin (V,))] of the bases whose every variant obeys the rules."""
    var = joint if var is None else var
    V = variants(levels)
    nb, nv = len(bases), len(V)
    if not nb:
        return []
    Q = np.repeat(np.array([b[0] for b in bases]), nv, axis=0)
    lo = np.repeat(np.array([b[1] for b in bases]), nv)
    hi = np.repeat(np.array([b[2] for b in bases]), nv)
    side = np.tile(np.array([v[0] for v in V]), nb)
    delta = np.tile(np.array([v[1] for v in V]), nb)
    jj = np.full(len(Q), joint)

    def g(x):
        q = Q.copy()
        q[:, var] = x
        return signed_g(taus(q, None, None, mode, mass), jj, sign)

    x = bisect(g, lo, hi, side * delta, side > 0)
    good = ~np.isnan(x)
    q = Q.copy()
    q[:, var] = np.where(good, x, lo)
    tau = taus(q, None, None, mode, mass)
    marg = np.asarray(signed_g(tau, jj, sign), dtype=np.float64)
    good &= others_inside(tau, jj, clear)
    good &= (q >= TR.LO + INSIDE).all(axis=1) & (q <= TR.HI - INSIDE).all(axis=1)
    good &= (side * marg >= delta) & (side * marg <= delta + 1e-12)
    good = good.reshape(nb, nv).all(axis=1)
    x, marg = x.reshape(nb, nv), marg.reshape(nb, nv)
    return [(bases[i][0], x[i], marg[i]) for i in range(nb) if good[i]]


# ---- dynamic bases ---------------------------------------------------------------------------------
QDD_CAP = 120.0


def dynamic_bases(mode, mass, joint, sign, want, key, target=0.0, n=1500, effect=None):
    """Brackets (q, qd, qdd0, x_below, x_above) on the factor x of qdd0, from tau's linearity in
    qdd: x* solves sign tau_j = L_j + target."""
    rng = rng_of(2, *key)
    out = []
    for _ in range(40):
        q = rand_q(rng, n)
        qd = rng.uniform(-2, 2, (n, 7))
        w = rng.uniform(0, 0.5, (n, 7))
        w[:, joint] = 1.0
        qdd0 = rng.uniform(-6, 6, (n, 7)) * w
        t0 = np.asarray(taus(q, qd, 0 * qdd0, mode, mass), dtype=np.float64)
        t1 = np.asarray(taus(q, qd, qdd0, mode, mass), dtype=np.float64)
        slope = sign * (t1 - t0)[:, joint]
        with np.errstate(divide="ignore", invalid="ignore"):
            xs = (LIM[joint] + target - sign * t0[:, joint]) / slope
        ok = np.isfinite(xs) & (xs > 0.5) & (np.abs(qdd0).max(axis=1) * xs <= QDD_CAP)
        ok &= (np.abs(slope) * xs > 1.0)
        xs = np.where(ok, xs, 1.0)
        at = t0 + xs[:, None] * (t1 - t0)
        m = np.abs(at[:, :6]) - LIM
        m[:, joint] = -np.inf
        ok &= (m <= -(TR.CLEAR + SLACK)).all(axis=1)
        if effect is not None:      # (mass, Nm): what that mass must add to sign * tau_j at x*
            f0 = np.asarray(taus(q, qd, 0 * qdd0, mode, effect[0]), dtype=np.float64)
            f1 = np.asarray(taus(q, qd, qdd0, mode, effect[0]), dtype=np.float64)
            ok &= sign * ((f0 - t0) + xs[:, None] * ((f1 - f0) - (t1 - t0)))[:, joint] >= effect[1]
        for i in np.nonzero(ok)[0]:
            out.append((q[i], qd[i], qdd0[i], xs[i] * (1 - 1e-4), xs[i] * (1 + 1e-4)))
            if len(out) == want:
                return out
    return out


def solve_dynamic(bases, mode, mass, joint, sign, targets, pick_hi):
    """Variants at signed targets (V,) -> [(q, qd, qdd0, x (V,), margin (V,))] of the valid."""
    nb, nv = len(bases), len(targets)
    if not nb:
        return []
    rep = lambda k: np.repeat(np.array([b[k] for b in bases]), nv, axis=0)  # noqa: E731
    Q, QD, QDD, lo, hi = rep(0), rep(1), rep(2), rep(3), rep(4)
    tgt = np.tile(np.asarray(targets, dtype=np.float64), nb)
    pick = np.tile(np.asarray(pick_hi, dtype=bool), nb)
    jj = np.full(len(Q), joint)

    def g(x):
        return signed_g(taus(Q, QD, QDD * x[:, None], mode, mass), jj, sign)

    x = bisect(g, lo, hi, tgt, pick)
    good = ~np.isnan(x)
    xx = np.where(good, x, lo)
    tau = taus(Q, QD, QDD * xx[:, None], mode, mass)
    marg = np.asarray(signed_g(tau, jj, sign), dtype=np.float64)
    good &= others_inside(tau, jj, TR.CLEAR)
    good &= np.where(pick, (marg >= tgt) & (marg <= tgt + 1e-12),
                     (marg < tgt) & (marg >= tgt - 1e-12))
    good = good.reshape(nb, nv).all(axis=1)
    x, marg = x.reshape(nb, nv), marg.reshape(nb, nv)
    return [(bases[i][0], bases[i][1], bases[i][2], x[i], marg[i]) for i in range(nb) if good[i]]


# ---- the row families ------------------------------------------------------------------------------
class Rows:
    def __init__(self):
        self.d = {k: [] for k in TR.BASE_KEYS}

    def add(self, family, q, qd, qdd, mode, mass, joint, sign, var, x, margin, nv):
        pad = lambda a: np.concatenate([np.asarray(a, dtype=np.float64),  # noqa: E731
                                        np.full(nv - len(a), np.nan)])
        for k, v in zip(TR.BASE_KEYS, (TR.FAMILIES.index(family), q, qd, qdd, mode, mass, joint,
                                       sign, var, pad(x), pad(margin))):
            self.d[k].append(v)

    def arrays(self):
        dt = dict(b_family=np.int8, b_mode=np.int8, b_joint=np.int8, b_sign=np.int8,
                  b_var=np.int8)
        return {k: np.array(v, dtype=dt.get(k, np.float64)) for k, v in self.d.items()}


def static_group(levels, family, mode, mass, joint, batches=6, need=True):
    """Candidate batches until both signs hold PER_GROUP valid bases: the first uniform over
    the joint limits, each later one the 300 largest sign * tau_j so far, each moved 40 times
    by N(0, 0.1 rad) per joint."""
    Z = np.zeros(7)
    got = {1: [], -1: []}
    key = (mode, joint, int(round(mass * 10)))
    q0, tau0 = static_candidates(mode, mass, key, 30000)
    jj = np.full(len(q0), joint)
    for sign in (1, -1):
        q, tau = q0, tau0
        for bt in range(batches):
            b = static_bases(q, tau, mode, mass, joint, sign, SPARE * PER_GROUP)
            got[sign] += solve_static(b, mode, mass, joint, sign, levels)
            if len(got[sign]) >= PER_GROUP:
                break
            s = np.asarray(sign * tau[:, joint], dtype=np.float64)
            top = q[np.argsort(-s, kind="stable")[:300]]
            rng = rng_of(3, *key, sign + 1, bt)
            q = np.clip(np.repeat(top, 40, axis=0) + rng.normal(0, 0.1, (12000, 7)), QLO, QHI)
            tau = taus(q, None, None, mode, mass)
    if min(len(v) for v in got.values()) < PER_GROUP:
        if need:
            raise RuntimeError("group %s: %s bases" % ((family, mode, mass, joint),
                                                       [len(v) for v in got.values()]))
        return None
    return [(family, qq, Z, Z, mode, mass, joint, sign, joint, x, m)
            for sign in (1, -1) for qq, x, m in got[sign][:PER_GROUP]]


def static_groups(levels, log):
    """Family 1 (nov; run as rne too) and dyn's static rows: (mode, mass, joint) groups."""
    out = []
    payload = {}

    def group(*a, **kw):
        return static_group(levels, *a, **kw)

    for mass, joint in ((5.0, 1), (3.7, 1), (9.0, 4), (9.0, 5)):
        out += group("static", TR.MODE_NOV, mass, joint)
    for joint in (2, 3):            # the smallest whole-kg payload whose search brackets them
        for kg in range(9, 40):
            g = group("static", TR.MODE_NOV, float(kg), joint, batches=3, need=False)
            if g is not None:
                payload[joint] = kg
                out += g
                break
        else:
            raise RuntimeError("joint %d never bracketed" % (joint + 1))
        log("joint %d bracketed at %d kg" % (joint + 1, payload[joint]))
    for joint in (1, 4, 5):
        out += group("dyn_static", TR.MODE_DYN, 5.0, joint)
    return out, payload


def dynamic_groups(levels, log):
    V = variants(levels)
    tg = [s * d for s, d in V]
    pick = [s > 0 for s, d in V]
    out = []
    for family, mode, masses in (("dynamic", TR.MODE_RNE, (0.0, 2.0, 5.0)),
                                 ("dyn_dynamic", TR.MODE_DYN, (0.0, 5.0))):
        for mass in masses:
            for joint in range(6):
                for sign in (1, -1):
                    key = (mode, int(mass * 10), joint, sign + 1)
                    b = dynamic_bases(mode, mass, joint, sign, SPARE * PER_GROUP, key)
                    s = solve_dynamic(b, mode, mass, joint, sign, tg, pick)[:PER_GROUP]
                    if len(s) < PER_GROUP:
                        raise RuntimeError("dynamic group %s: %d" % (key, len(s)))
                    out += [(family, q, qd, qdd, mode, mass, joint, sign, -1, x, m)
                            for q, qd, qdd, x, m in s]
    return out


M_ABOVE = float(np.nextafter(0.01, 1))


def threshold_groups(log):
    """Family 4.  rne: the deciding joint passes by 0.03 Nm without the payload body and fails
    with it at the first mass above 0.01 kg; dyn: passes by 0.02 Nm at 0 kg, fails at 0.005 kg.
    One variant per base: x at the passing margin; the masses are the test's."""
    out = []
    for family, mode, pass_by, m_fail in (("threshold_rne", TR.MODE_RNE, 0.03, M_ABOVE),
                                          ("threshold_dyn", TR.MODE_DYN, 0.02, 0.005)):
        got = []
        for joint, sign in ((1, 1), (1, -1), (3, 1), (3, -1)):
            b = dynamic_bases(mode, 0.0, joint, sign, 6, (9, mode, joint, sign + 1),
                              target=-pass_by, effect=(m_fail, pass_by + 5e-3))
            s = solve_dynamic(b, mode, 0.0, joint, sign, [-pass_by], [False])
            keep = []
            for q, qd, qdd, x, m in s:
                tau = taus(q, qd, qdd * x[0], mode, m_fail)
                jj = np.array([joint])
                gf = float(signed_g(tau, jj, sign)[0])
                if gf >= 2e-3 and others_inside(tau, jj, TR.CLEAR)[0] and -0.04 <= m[0] <= -0.02:
                    keep.append((family, q, qd, qdd, mode, m_fail, joint, sign, -1, x,
                                 np.array([gf])))
            got.append(keep)
        rows = [g[i] for i in range(6) for g in got if i < len(g)][:PER_GROUP]   # round robin
        if len(rows) < PER_GROUP:
            raise RuntimeError("%s: %d rows" % (family, len(rows)))
        out += rows
    return out


def joint7_rows(log):
    """Family 5: |tau_7| beyond 12 Nm by at least 1 Nm through qdd_7, every tested joint at least
    0.5 Nm inside under nov, rne and dyn alike.  One base per row, no variant."""
    rng = rng_of(5)
    out = []
    while len(out) < PER_GROUP:
        n = 2000
        q = rand_q(rng, n)
        qd = rng.uniform(-1, 1, (n, 7))
        qdd = rng.uniform(-2, 2, (n, 7))
        qdd[:, 6] = rng.choice([-1.0, 1.0], n) * rng.uniform(130, 220, n)
        mass = 5.0 if len(out) % 2 == 0 else 0.0
        ok = np.ones(n, dtype=bool)
        t7 = None
        for mode in (TR.MODE_NOV, TR.MODE_RNE, TR.MODE_DYN):
            tau = taus(q, qd, qdd, mode, mass)
            ok &= (np.asarray(TR.margins(tau), dtype=np.float64) <= -TR.CLEAR).all(axis=1)
            if mode != TR.MODE_NOV:
                ok &= np.abs(np.asarray(tau[:, 6], dtype=np.float64)) >= 13.0
                t7 = tau[:, 6]
        for i in np.nonzero(ok)[0][:1]:
            out.append(("joint7", q[i], qd[i], qdd[i], TR.MODE_RNE, mass, 6,
                        int(np.sign(float(t7[i]))), -2, np.array([1.0]),
                        np.array([abs(float(t7[i])) - 12.0])))
    return out


def joint1_rows(log):
    """Family 1's joint 1: its axis is vertical, so it carries no static torque; rows that pass
    by 0.5 Nm on joints 2..6 at 5 kg, recorded with |tau_1| as the margin's distance from 87."""
    rng = rng_of(11)
    q = rand_q(rng, 400)
    tau = taus(q, None, None, TR.MODE_NOV, 5.0)
    ok = (np.asarray(TR.margins(tau), dtype=np.float64) <= -TR.CLEAR).all(axis=1)
    Z = np.zeros(7)
    return [("static_j1", q[i], Z, Z, TR.MODE_NOV, 5.0, 0, 0, -2, np.array([1.0]),
             np.array([abs(float(tau[i, 0])) - 87.0])) for i in np.nonzero(ok)[0][:PER_GROUP]]


# ---- edges (family 6) -------------------------------------------------------------------------------
EDGE_PER = 4
EDGE_GROUPS = ((TR.MODE_NOV, 1), (TR.MODE_RNE, 1), (TR.MODE_DYN, 1), (TR.MODE_DYN, 4))
EDGE_MASS = 5.0


def edge_steps(a, b):
    import metric_cases as MC
    return np.array(MC.extend_ref(a, b, 0.1 * np.ones(7)), dtype=np.float64)


def edge_bases(mode, joint, kpos, clear, want, log):
    """Edges (a, b, k) in an empty scene through a configuration P within 0.1 Nm of joint's limit
    at step k.  Last position: a random direction.  First and middle: a direction along which
    tau_j is stationary at P (the random one minus its part along the finite-difference gradient),
    so that the step can be the profile's peak.  Kept when, relative to step k, the deciding
    joint is `clear` lower at every other point (the start included) and every other joint is
    CLEAR inside everywhere."""
    rng = rng_of(6, mode, joint, kpos)
    out = []
    for _ in range(30):
        n = 40000
        q = rand_q(rng, n)
        tau = taus(q, None, None, mode, EDGE_MASS)
        m = np.asarray(TR.margins(tau), dtype=np.float64)
        near = np.abs(m[:, joint]) < 0.1
        oth = m.copy()
        oth[:, joint] = -np.inf
        near &= (oth <= -(TR.CLEAR + 2 * SLACK)).all(axis=1)
        P = q[near]
        if not len(P):
            continue
        tries = 48
        d = rng.normal(size=(len(P) * tries, 7))
        if kpos < 2:
            grad = np.zeros_like(P)
            for c in range(7):
                e = np.zeros(7)
                e[c] = 1e-4
                grad[:, c] = np.asarray(taus(P + e, None, None, mode, EDGE_MASS)[:, joint] -
                                        taus(P - e, None, None, mode, EDGE_MASS)[:, joint],
                                        dtype=np.float64) / 2e-4
            gh = np.repeat(grad / np.linalg.norm(grad, axis=1)[:, None], tries, axis=0)
            d -= (d * gh).sum(axis=1)[:, None] * gh
        P = np.repeat(P, tries, axis=0)
        d /= np.linalg.norm(d, axis=1)[:, None]
        ns = rng.integers(4, 8, len(P))
        k = np.where(kpos == 0, 0, np.where(kpos == 1, ns // 2, ns - 1))
        L = 0.1 * (ns - 1 + rng.uniform(0.1, 0.9, len(P)))
        a = P - ((k + 1) / ns * L)[:, None] * d
        b = a + L[:, None] * d
        inside = ((a >= QLO) & (a <= QHI) & (b >= QLO) & (b <= QHI)).all(axis=1)
        # every point a + (i / n)(b - a), i = 0..n: one evaluation of 8 rows per edge
        fr = np.arange(8)[None, :] / ns[:, None]
        pts = a[:, None, :] + np.minimum(fr, 1.0)[:, :, None] * (b - a)[:, None, :]
        sel = np.nonzero(inside)[0]
        if not len(sel):
            continue
        tp = taus(pts[sel].reshape(-1, 7), None, None, mode, EDGE_MASS)
        mp = np.asarray(TR.margins(tp), dtype=np.float64).reshape(len(sel), 8, 6)
        dj = mp[:, :, joint].copy()
        mp[:, :, joint] = -np.inf
        for r, i in enumerate(sel):
            kk = k[i] + 1                           # the point index of step k
            rel = dj[r, :ns[i] + 1] - dj[r, kk]
            rel[kk] = -np.inf
            if rel.max() <= -(clear + 0.3 * clear) and mp[r, :ns[i] + 1].max() <= -(TR.CLEAR + 0.15):
                sign = 1 if float(tp[r * 8 + kk, joint]) > 0 else -1
                out.append((a[i].copy(), b[i].copy(), int(k[i]), int(ns[i]), sign))
                if len(out) == want:
                    return out
    return out


def solve_edges(bases, mode, joint, levels, clear_after):
    """Variants on a shift x of both ends' angle `joint` -> [(a, b, k, sign, xa (V,), xb (V,),
    margin (V,), clear before, clear after)] of the bases whose every variant obeys the rules."""
    V = variants(levels)
    nv = len(V)
    rowsA, rowsB, K, N, S = [], [], [], [], []
    for a, b, k, ns, sign in bases:
        rowsA += [a] * nv; rowsB += [b] * nv; K += [k] * nv; N += [ns] * nv; S += [sign] * nv
    A, B0 = np.array(rowsA), np.array(rowsB)
    K, N, S = np.array(K), np.array(N), np.array(S)
    side = np.tile(np.array([v[0] for v in V]), len(bases))
    delta = np.tile(np.array([v[1] for v in V]), len(bases))
    jj = np.full(len(A), joint)

    def ends(i, x):
        a, b = A[i].copy(), B0[i].copy()
        a[joint] += x
        b[joint] += x
        return a, b

    def step_k(x):
        out = np.empty_like(A)
        for i in range(len(A)):
            st = edge_steps(*ends(i, x[i]))
            out[i] = st[K[i]] if len(st) == N[i] else np.nan
        return out

    def g(x):
        return S * taus(step_k(x), None, None, mode, EDGE_MASS)[np.arange(len(A)), jj] - LIM[joint]

    x0 = np.zeros(len(A))
    g0 = np.asarray(g(x0), dtype=np.float64)
    lo = np.full(len(A), np.nan)
    hi = np.full(len(A), np.nan)
    for dx in (0.004, -0.004, 0.012, -0.012, 0.04, -0.04):
        x1 = x0 + dx
        g1 = np.asarray(g(x1), dtype=np.float64)
        take = np.isnan(lo) & np.isfinite(g1) & (g1 * g0 < 0) & (np.abs(g1) > 1e-4) & \
            (np.abs(g0) > 1e-4)
        lo = np.where(take, np.where(g0 < 0, x0, x1), lo)
        hi = np.where(take, np.where(g0 < 0, x1, x0), hi)
    have = ~np.isnan(lo)
    lo, hi = np.where(have, lo, x0), np.where(have, hi, x0)
    x = bisect(g, lo, hi, side * delta, side > 0)
    good = have & ~np.isnan(x)
    out = []
    nb = len(bases)
    info = []
    for i in range(len(A)):
        if not good[i]:
            info.append(None)
            continue
        a, b = ends(i, x[i])
        st = edge_steps(a, b)
        if len(st) != N[i]:
            good[i] = False
            info.append(None)
            continue
        pts = np.concatenate([a[None], st])
        tau = taus(pts, None, None, mode, EDGE_MASS)
        m = np.asarray(TR.margins(tau), dtype=np.float64)
        kk = K[i] + 1
        marg = float(S[i] * tau[kk, joint] - LIM[joint])
        o = m[kk].copy()
        o[joint] = -np.inf
        before = -m[:kk].max()
        after = -m[kk + 1:].max() if kk + 1 < len(pts) else np.inf
        lim_ok = (pts >= TR.LO + INSIDE).all() and (pts <= TR.HI - INSIDE).all()
        if not (lim_ok and o.max() <= -TR.CLEAR and min(before, after) >= clear_after
                and delta[i] <= side[i] * marg <= delta[i] + 1e-12):
            good[i] = False
        info.append((marg, before, after, a[joint], b[joint]))
    good = good.reshape(nb, nv).all(axis=1)
    for r in range(nb):
        if good[r]:
            sl = slice(r * nv, (r + 1) * nv)
            a, b, k, ns, sign = bases[r]
            ii = range(sl.start, sl.stop)
            out.append((a, b, k, sign, np.array([info[i][3] for i in ii]),
                        np.array([info[i][4] for i in ii]), np.array([info[i][0] for i in ii]),
                        min(info[i][1] for i in range(sl.start, sl.stop)),
                        min(info[i][2] for i in range(sl.start, sl.stop))))
    return out


def edge_groups(levels, log):
    out = []
    for mode, joint in EDGE_GROUPS:
        for kpos in (0, 1, 2):
            ca = TR.EDGE_CLEAR_PEAK if kpos < 2 else TR.CLEAR
            b = edge_bases(mode, joint, kpos, ca, 3 * EDGE_PER, log)
            s = solve_edges(b, mode, joint, levels, ca)[:EDGE_PER] if b else []
            if len(s) < EDGE_PER:
                raise RuntimeError("edges (%d, %d, %d): %d" % (mode, joint, kpos, len(s)))
            out += [(mode, joint, kpos) + e for e in s]
    return out


# ---- the goal search's coarse level and the rewire case -----------------------------------------
GOAL_LEVEL = 1e-3


def goal_rows(arrs):
    """A further level for tcmp_goal_search: every static base (families 1 and 3) at +-1e-3 Nm,
    bracketed from its own 1e-6 variants.  -> g_base, g_x (., 2: fails, passes), g_margin."""
    fam = [TR.FAMILIES.index(f) for f in ("static", "dyn_static")]
    idx = np.nonzero(np.isin(arrs["b_family"], fam))[0]
    gx, gm = np.zeros((len(idx), 2)), np.zeros((len(idx), 2))
    for key in sorted({(int(arrs["b_mode"][b]), float(arrs["b_mass"][b]), int(arrs["b_joint"][b]),
                        int(arrs["b_sign"][b])) for b in idx}):
        mode, mass, joint, sign = key
        sel = [r for r, b in enumerate(idx)
               if (int(arrs["b_mode"][b]), float(arrs["b_mass"][b]), int(arrs["b_joint"][b]),
                   int(arrs["b_sign"][b])) == key]
        bases = []
        for r in sel:
            b = idx[r]
            xf, xp = arrs["b_x"][b, 0], arrs["b_x"][b, 1]          # +1e-6, -1e-6
            bases.append((arrs["b_q"][b], xp - 4000 * (xf - xp), xf + 4000 * (xf - xp)))
        s = solve_static(bases, mode, mass, joint, sign, [GOAL_LEVEL])
        if len(s) != len(bases):
            raise RuntimeError("goal level: group %s" % (key,))
        for r, (_, x, m) in zip(sel, s):
            gx[r], gm[r] = x, m
    return dict(g_base=idx.astype(np.int64), g_x=gx, g_margin=gm)


REWIRE_RADIUS = 4.0
REWIRE_CLEAR = 0.03            # Nm inside asked of every step the case walks beside the probe


def _from_u(u):
    return (1 - u) * TR.LO + u * TR.HI          # the planner's uniform sample, as it computes it


def rewire_case(E, log):
    """Three rounds by host-supplied samples whose last new node's rewire edge is a family-6 probe
    at 1e-9 Nm.  Start a (an rne edge's start at 5 kg, probe at a middle step).  Round 1 draws
    the goal, placed up the deciding torque's gradient so that the edge from a fails at its first
    step and adds nothing.  Round 2 samples C (uniform draw u_C) beside b: the node C' = the end of
    a -> C.  Round 3 samples S (draw u_S) at b: nearest C', the node nw = the end of C' -> S, and
    the neighbour a offers the cheaper path, so the edge a -> nw is walked: the probe.  Bisection
    on u_S[joint] puts its step k at +-1e-9 Nm.  -> arrays r_*; expected parents (C' = 1 when the
    probe fails, a = 0 when it passes)."""
    mode, joint, mass = TR.MODE_RNE, 1, EDGE_MASS
    rng = rng_of(7)
    span = TR.HI - TR.LO
    for ent in [e for e in E if e[0] == mode and e[1] == joint and e[2] == 1]:
        a, b, k, sign = ent[3].copy(), ent[4].copy(), ent[5], ent[6]
        a[joint], b[joint] = ent[7][0], ent[8][0]
        n = len(edge_steps(a, b))
        grad = np.zeros(7)
        for c in range(7):
            e = np.zeros(7)
            e[c] = 1e-4
            grad[c] = float(taus(a + e, None, None, mode, mass)[0, joint] -
                            taus(a - e, None, None, mode, mass)[0, joint]) / 2e-4
        goal = a + 0.8 * sign * grad / np.linalg.norm(grad)
        if not ((goal >= QLO) & (goal <= QHI)).all():
            continue
        m0 = TR.margins(taus(edge_steps(a, goal)[:1], None, None, mode, mass))
        if float(m0[0, joint]) < TR.CLEAR:
            continue

        def clear(pts):
            return -float(np.asarray(TR.margins(taus(pts, None, None, mode, mass)),
                                     dtype=np.float64).max())

        uS0 = (b - TR.LO) / span
        for _ in range(400):
            uC = (np.clip(b + rng.normal(0, 0.12, 7), QLO, QHI) - TR.LO) / span
            C = _from_u(uC)
            st = edge_steps(a, C)
            Cn = st[-1]
            if np.linalg.norm(Cn - b) >= np.linalg.norm(a - b) or clear(st) < 0.2:
                continue
            if clear(edge_steps(Cn, _from_u(uS0))) < REWIRE_CLEAR + 0.01:
                continue
            break
        else:
            continue

        def node(uj):
            u = uS0.copy()
            u[joint] = uj
            return edge_steps(Cn, _from_u(u))[-1]

        def g(x):
            out = np.zeros(len(x), dtype=LD)
            for i in range(len(x)):
                st = edge_steps(a, node(x[i]))
                out[i] = sign * taus(st[k:k + 1], None, None, mode, mass)[0, joint] - LIM[joint] \
                    if len(st) == n else np.nan
            return out

        du = 0.03 / span[joint]
        x0 = np.array([uS0[joint] - du, uS0[joint] + du])
        g0 = np.asarray(g(x0), dtype=np.float64)
        if not (np.isfinite(g0).all() and g0[0] * g0[1] < 0):
            continue
        lo, hi = (x0[0], x0[1]) if g0[0] < 0 else (x0[1], x0[0])
        side = np.array([1, -1])
        x = bisect(g, np.full(2, lo), np.full(2, hi), side * 1e-9, side > 0)
        if np.isnan(x).any():
            continue
        uS = np.repeat(uS0[None], 2, axis=0)
        uS[:, joint] = x
        marg, good = np.zeros(2), True
        for v in range(2):
            S = _from_u(uS[v])
            walk = edge_steps(Cn, S)
            nw = walk[-1]
            st = edge_steps(a, nw)
            m = np.asarray(TR.margins(taus(st, None, None, mode, mass)), dtype=np.float64)
            marg[v] = float(sign * taus(st[k:k + 1], None, None, mode, mass)[0, joint] - LIM[joint])
            m[k, joint] = -np.inf
            good &= len(st) == n and m[:, joint].max() <= -REWIRE_CLEAR
            m[:, joint] = -np.inf
            good &= m.max() <= -TR.CLEAR and clear(walk) >= REWIRE_CLEAR
            good &= np.linalg.norm(Cn - S) < np.linalg.norm(a - S)
            good &= 1e-9 <= side[v] * marg[v] <= 1e-9 + 1e-12
            good &= bool(((walk >= TR.LO + INSIDE) & (walk <= TR.HI - INSIDE)).all())
        if good:
            return dict(r_a=a, r_goal=goal, r_uC=uC, r_uS=uS, r_margin=marg,
                        r_mode=np.int8(mode), r_mass=np.float64(mass), r_joint=np.int8(joint),
                        r_k=np.int8(k), r_radius=np.float64(REWIRE_RADIUS),
                        r_parent=np.array([1, 0], dtype=np.int32))
    raise RuntimeError("no rewire case")


# ---- assembling --------------------------------------------------------------------------------------
def build_once(levels, log):
    R = Rows()
    nv = 2 * len(levels)
    st, payload = static_groups(levels, log)
    rows = st + joint1_rows(log) + dynamic_groups(levels, log) + threshold_groups(log) + \
        joint7_rows(log)
    order = {f: i for i, f in enumerate(TR.FAMILIES)}
    rows.sort(key=lambda r: order[r[0]])          # stable: family order, then search order
    for r in rows:
        R.add(*r, nv=nv)
    out = R.arrays()
    E = edge_groups(levels, log)
    out.update(
        e_mode=np.array([e[0] for e in E], dtype=np.int8),
        e_joint=np.array([e[1] for e in E], dtype=np.int8),
        e_kpos=np.array([e[2] for e in E], dtype=np.int8),
        e_a=np.array([e[3] for e in E]), e_b=np.array([e[4] for e in E]),
        e_k=np.array([e[5] for e in E], dtype=np.int8),
        e_sign=np.array([e[6] for e in E], dtype=np.int8),
        e_xa=np.array([e[7] for e in E]), e_xb=np.array([e[8] for e in E]),
        e_margin=np.array([e[9] for e in E]),
        e_clear_before=np.array([e[10] for e in E]), e_clear_after=np.array([e[11] for e in E]),
        e_mass=np.full(len(E), EDGE_MASS),
        levels=np.array(levels), j3_payload=np.int64(payload[2]), j4_payload=np.int64(payload[3]))
    out.update(goal_rows(out))
    out.update(rewire_case(E, log))
    return out


def oracle_deviation(arrs):
    """The largest |oracle fp64 - restatement| (Nm) over every row and edge step of the fixture:
    the mode's torques and rne with the payload body at the row's mass."""
    import oracle as O
    fx = TR.Fixture(arrays=arrs)
    worst = 0.0
    ref_mode = TR.mode_torques(fx.q, fx.qd, fx.qdd, fx.mode, fx.mass)
    ref_rne = TR.rne_hp(fx.q, fx.qd, fx.qdd, fx.mass)
    for i in range(fx.n):
        rates = fx.mode[i] != TR.MODE_NOV
        qd, qdd = (fx.qd[i], fx.qdd[i]) if rates else (np.zeros(7), np.zeros(7))
        if fx.mode[i] == TR.MODE_DYN:
            t = O.dyn_tau(fx.q[i], qd, qdd, fx.mass[i])
        else:
            t = O.rne(fx.q[i], qd, qdd, fx.mass[i] if fx.mass[i] > TR.PAYLOAD_MIN else 0.0)[0]
        worst = max(worst, float(np.abs(t.astype(LD) - ref_mode[i]).max()))
        t = O.rne(fx.q[i], fx.qd[i], fx.qdd[i], fx.mass[i])[0]
        worst = max(worst, float(np.abs(t.astype(LD) - ref_rne[i]).max()))
    ref = TR.mode_torques(fx.gq, None, None, fx.gmode, fx.gmass)
    for i in range(len(fx.gq)):
        t = O.dyn_tau(fx.gq[i], None, None, fx.gmass[i]) if fx.gmode[i] == TR.MODE_DYN \
            else O.rne(fx.gq[i], 0 * fx.gq[i], 0 * fx.gq[i], fx.gmass[i])[0]
        worst = max(worst, float(np.abs(t.astype(LD) - ref[i]).max()))
    for e in range(fx.m):
        st = fx.steps[e]
        ref = TR.mode_torques(st, None, None, fx.emode[e], fx.emass[e])
        for i in range(len(st)):
            t = O.dyn_tau(st[i], None, None, fx.emass[e]) if fx.emode[e] == TR.MODE_DYN \
                else O.rne(st[i], 0 * st[i], 0 * st[i], fx.emass[e])[0]
            worst = max(worst, float(np.abs(t.astype(LD) - ref[i]).max()))
    return worst


def ref_uncertainty(arrs, every=16):
    """Longdouble against 50 digits on every `every`-th row (mode torques and rne)."""
    fx = TR.Fixture(arrays=arrs)
    idx = np.arange(0, fx.n, every)
    mc = TR.mpc(50)
    args = (fx.q[idx], fx.qd[idx], fx.qdd[idx])
    u = TR.ld_minus_mp(TR.mode_torques(*args, fx.mode[idx], fx.mass[idx]),
                       TR.mode_torques(*args, fx.mode[idx], fx.mass[idx], mc))
    return max(u, TR.ld_minus_mp(TR.rne_hp(*args, fx.mass[idx]),
                                 TR.rne_hp(*args, fx.mass[idx], mc)))


def delta_min_of(band):
    k = 0
    while float("1e-%d" % (k + 1)) >= 4 * band:
        k += 1
    return float("1e-%d" % k)


def build(log=lambda s: None):
    fine = 1e-11
    for _ in range(4):
        levels = [1e-6, 1e-9, fine] if fine < 1e-9 else [1e-6, fine]
        arrs = build_once(levels, log)
        dev = oracle_deviation(arrs)
        band = 64 * dev
        dmin = delta_min_of(band)
        log("levels %s: oracle deviation %.3g, band %.3g, delta_min %g" % (levels, dev, band, dmin))
        if dmin == fine:
            break
        fine = dmin
    else:
        raise RuntimeError("delta_min did not settle")
    arrs.update(oracle_dev=np.float64(dev), band=np.float64(band), delta_min=np.float64(dmin),
                ref_uncertainty=np.float64(ref_uncertainty(arrs)))
    assert 1000 * float(arrs["ref_uncertainty"]) <= dmin
    return arrs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=TR.fixture_path())
    a = ap.parse_args()
    arrs = build(print)
    np.savez_compressed(a.out, **arrs)
    print("%s: %d bases, %d edges, %d bytes" % (a.out, len(arrs["b_q"]), len(arrs["e_a"]),
                                               os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
