"""CPU: the torque test pinned at its limits (tests/torque_ref.py, tests/golden/torque_limits.npz).

The high-precision restatement is held against the reference's own vectors; the fixture against
its construction rules, its generator and its recorded band; and the oracle against every probe,
which shows that it stays a valid comparison at these margins."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

import metric_cases as MC
import oracle as O
import torque_ref as TR

sys.path.insert(0, GOLDEN)
import gen_torque_limits as G  # noqa: E402

LD = np.longdouble
LIM = np.array(TR.EFFORT[:6])


@pytest.fixture(scope="module")
def fx():
    return TR.Fixture()


@pytest.fixture(scope="module")
def ref(fx):
    """The restatement's torques of every row, once: what each mode's test compares."""
    return TR.mode_torques(fx.q, fx.qd, fx.qdd, fx.mode, fx.mass)


def test_restatement_matches_reference():
    """torque_ref.rne_hp against rne_golden.npz (the reference's own output), within the tolerance
    test_oracle_golden.py holds the oracle to against the same file."""
    z = np.load(os.path.join(GOLDEN, "rne_golden.npz"))
    for m in (0, 2, 5):
        t = "m%d" % m
        q, qd, qdd = z["q_" + t], z["qd_" + t], z["qdd_" + t]
        assert np.abs(TR.f64(TR.rne_hp(q, 0 * q, 0 * q, m)) - z["tau_static_" + t]).max() < 1e-9
        assert np.abs(TR.f64(TR.rne_hp(q, qd, qdd, m)) - z["tau_dyn_" + t]).max() < 1e-9


def test_dyn_force_term_is_its_own_fk_gradient():
    """dyn's J^T [0, 0, m g, 0, 0, 0] has no reference vector: the reference calls
    panda_dynamics_model, which it does not ship.  The term is m g times the gradient of the grasp
    target's height; checked against a central difference of torque_ref.target_z in longdouble
    (h = 1e-6: truncation about 1e-12, rounding about 1e-13).  Unpinned against pdm."""
    rng = np.random.default_rng(2)
    q = TR.LO + (TR.HI - TR.LO) * rng.random((20, 7))
    m = 3.5
    ext = TR.dyn_force_term(q, m)
    h = LD(1e-6)
    for c in range(7):
        e = np.zeros(7, dtype=LD)
        e[c] = h
        up = TR.target_z(q.astype(LD) + e)
        dn = TR.target_z(q.astype(LD) - e)
        fd = LD(m) * LD(TR.GRAV) * (up - dn) / (2 * h)
        assert float(np.abs(ext[:, c] - fd).max()) < 1e-9
    base = TR.mode_torques(q, None, None, TR.MODE_DYN, 0.0)
    assert float(np.abs(base - TR.rne_hp(q, 0 * q, 0 * q, 0.0)).max()) == 0.0
    assert float(np.abs(TR.mode_torques(q, None, None, TR.MODE_DYN, m) - base - ext).max()) < 1e-15


def test_reference_uncertainty(fx):
    """Longdouble against 50 digits on every 16th row: the stored figure, and at least 1000 times
    below the smallest margin."""
    u = G.ref_uncertainty(fx.__dict__)
    assert u == float(fx.ref_uncertainty)
    assert 1000 * u <= fx.delta_min


def test_band_and_levels(fx):
    """B = 64 times the oracle's largest deviation from the restatement over every row and edge
    step, remeasured; delta_min the smallest power of ten >= 4 B; the levels."""
    dev = G.oracle_deviation(fx.__dict__)
    assert dev == float(fx.oracle_dev)
    assert fx.band == 64 * dev
    assert fx.delta_min >= 4 * fx.band > fx.delta_min / 10
    want = [1e-6, 1e-9, fx.delta_min] if fx.delta_min < 1e-9 else [1e-6, fx.delta_min]
    assert [float(x) for x in fx.levels] == want


def _same(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def test_fixture_regenerates(fx):
    """Groups of every kind searched and bisected again from their seeds: bit for bit the stored
    bases.  A sample, because the whole generator takes three minutes: gen_torque_limits.py writes
    the file group by group from per-group seeds in the same way, and a full run of it reproduces
    the committed file (checked when the fixture was written); the groups not resampled here are
    the static ones at 3.7, 9, 10 and 13 kg, dyn's static ones and eleven of the twelve edge
    groups.  The goal level and the rewire case, which derive from stored bases, are rebuilt
    whole."""
    levels = [float(x) for x in fx.levels]
    V = G.variants(levels)
    nv = len(V)

    def stored(family, mode, mass, joint, sign=None):
        f = TR.FAMILIES.index(family)
        m = (fx.b_family == f) & (fx.b_mode == mode) & (fx.b_mass == mass) & (fx.b_joint == joint)
        if sign is not None:
            m &= fx.b_sign == sign
        return np.nonzero(m)[0]

    g = G.static_group(levels, "static", TR.MODE_NOV, 5.0, 1)
    idx = stored("static", TR.MODE_NOV, 5.0, 1)
    assert len(g) == len(idx) == 2 * G.PER_GROUP
    for r, b in zip(g, idx):
        assert _same(r[1], fx.b_q[b]) and _same(r[9], fx.b_x[b]) and r[7] == fx.b_sign[b]
    tg, pick = [s * d for s, d in V], [s > 0 for s, d in V]
    b0 = G.dynamic_bases(TR.MODE_RNE, 5.0, 0, 1, G.SPARE * G.PER_GROUP, (TR.MODE_RNE, 50, 0, 2))
    s = G.solve_dynamic(b0, TR.MODE_RNE, 5.0, 0, 1, tg, pick)[:G.PER_GROUP]
    idx = stored("dynamic", TR.MODE_RNE, 5.0, 0, 1)
    assert len(s) == len(idx) == G.PER_GROUP
    for r, b in zip(s, idx):
        assert _same(r[0], fx.b_q[b]) and _same(r[2], fx.b_qdd[b]) and _same(r[3], fx.b_x[b])
    for rows, fam in ((G.threshold_groups(None), ("threshold_rne", "threshold_dyn")),
                      (G.joint7_rows(None), ("joint7",)), (G.joint1_rows(None), ("static_j1",))):
        idx = np.nonzero(np.isin(fx.b_family, [TR.FAMILIES.index(f) for f in fam]))[0]
        assert len(rows) == len(idx)
        for r, b in zip(rows, idx):
            assert _same(r[1], fx.b_q[b]) and _same(r[3], fx.b_qdd[b])
            assert _same(r[9], fx.b_x[b, :len(r[9])]) and r[5] == fx.b_mass[b]
    mode, joint, kpos = TR.MODE_DYN, 4, 1
    e = G.solve_edges(G.edge_bases(mode, joint, kpos, TR.EDGE_CLEAR_PEAK, 3 * G.EDGE_PER, None),
                      mode, joint, levels, TR.EDGE_CLEAR_PEAK)[:G.EDGE_PER]
    idx = np.nonzero((fx.e_mode == mode) & (fx.e_joint == joint) & (fx.e_kpos == kpos))[0]
    assert len(e) == len(idx) == G.EDGE_PER
    for r, b in zip(e, idx):
        assert _same(r[0], fx.e_a[b]) and _same(r[1], fx.e_b[b])
        assert _same(r[4], fx.e_xa[b]) and _same(r[5], fx.e_xb[b]) and nv == len(r[4])
    g = G.goal_rows(fx.__dict__)
    assert np.array_equal(g["g_base"], fx.g_base) and _same(g["g_x"], fx.g_x)
    E = [(fx.e_mode[i], fx.e_joint[i], fx.e_kpos[i], fx.e_a[i], fx.e_b[i], int(fx.e_k[i]),
          int(fx.e_sign[i]), fx.e_xa[i], fx.e_xb[i]) for i in range(len(fx.e_a))]
    r = G.rewire_case(E, None)
    for k in TR.REWIRE_KEYS:
        assert _same(r[k], getattr(fx, k)), k


def test_rows_obey_their_construction_rules(fx, ref):
    """One comparison decides each probe: the deciding joint sits its level from the limit on its
    side, with its sign; every other tested joint is at least 0.5 Nm inside; q is inside the joint
    limits by 1e-3; each group holds 8 probes per (joint, sign, side, level)."""
    m = np.asarray(TR.margins(ref), dtype=np.float64)
    tau = TR.f64(ref)
    assert ((fx.q >= TR.LO + 1e-3) & (fx.q <= TR.HI - 1e-3)).all()
    assert (np.abs(fx.qd) <= 2.0).all()
    assert (TR.decide(ref) == fx.ok).all()
    pr = fx.rows(*TR.PROBES)
    r = np.arange(fx.n)
    dec = m[r, fx.joint.clip(0, 5)]
    assert (np.sign(tau[pr, fx.joint[pr]]) == fx.sign[pr]).all()
    assert (fx.side[pr] * dec[pr] >= fx.delta[pr]).all()
    assert (fx.side[pr] * dec[pr] <= fx.delta[pr] + 1e-12).all()
    assert (np.abs(dec[pr]) > fx.band).all() and fx.delta[pr].min() == fx.delta_min
    assert _same(dec[pr], fx.margin[pr])
    oth = m.copy()
    oth[pr, fx.joint[pr]] = -np.inf
    th = fx.rows("threshold_rne", "threshold_dyn")
    oth[th, fx.joint[th]] = -np.inf
    assert (oth <= -TR.CLEAR).all()
    # 8 per (family, mode, mass, joint, sign, side, level), both sides and both signs
    keys = {}
    for i in pr:
        k = (fx.names[i], fx.mode[i], fx.mass[i], fx.joint[i], fx.sign[i], fx.side[i], fx.delta[i])
        keys[k] = keys.get(k, 0) + 1
    assert set(keys.values()) == {G.PER_GROUP}
    groups = {k[:4] for k in keys}
    j3, j4 = float(fx.j3_payload), float(fx.j4_payload)
    want = {("static", 1, 5.0, 1), ("static", 1, 3.7, 1), ("static", 1, 9.0, 4),
            ("static", 1, 9.0, 5), ("static", 1, j3, 2), ("static", 1, j4, 3)}
    want |= {("dyn_static", 3, 5.0, j) for j in (1, 4, 5)}
    want |= {("dynamic", 2, ms, j) for ms in (0.0, 2.0, 5.0) for j in range(6)}
    want |= {("dyn_dynamic", 3, ms, j) for ms in (0.0, 5.0) for j in range(6)}
    assert groups == want
    assert len(keys) == len(want) * 2 * 2 * len(fx.levels)
    st = fx.rows("static", "dyn_static", "static_j1")
    assert not fx.qd[st].any() and not fx.qdd[st].any()
    # joint 1 cannot bind statically: its torque is nothing, far below every limit
    j1 = fx.rows("static_j1")
    assert len(j1) == G.PER_GROUP and (np.abs(tau[j1, 0]) < 1e-12).all()
    # the payload threshold: the passing mass by 0.02-0.04 Nm, the failing one clearly
    for fam, m_pass, m_fail in (("threshold_rne", 0.01, float(np.nextafter(0.01, 1))),
                                ("threshold_dyn", 0.0, 0.005)):
        t = fx.rows(fam)
        assert len(t) == 2 * G.PER_GROUP
        p, f = t[0::2], t[1::2]
        assert (fx.mass[p] == m_pass).all() and (fx.mass[f] == m_fail).all()
        assert np.array_equal(fx.q[p], fx.q[f]) and np.array_equal(fx.qdd[p], fx.qdd[f])
        assert ((dec[p] <= -0.02) & (dec[p] >= -0.04)).all() and (dec[f] >= 2e-3).all()
        assert fx.ok[p].all() and not fx.ok[f].any()
    # joint 7 is not tested: beyond its 12 Nm by 1 Nm or more under rne and dyn, and the rows pass
    j7 = fx.rows("joint7")
    assert len(j7) == 3 * G.PER_GROUP and fx.ok[j7].all()
    assert (np.abs(tau[j7, 6])[fx.mode[j7] != TR.MODE_NOV] >= 13.0).all()


def test_edges_obey_their_construction_rules(fx):
    """Family 6: one step of each edge is the probe; every other step and the start are inside by
    0.5 Nm (last position) or EDGE_CLEAR_PEAK (first, middle: see torque_ref); four edges per
    (mode, joint, position, side, level), the start always feasible."""
    keys = {}
    for e in range(fx.m):
        st, k, j = fx.steps[e], int(fx.ek[e]), int(fx.ejoint[e])
        pts = np.concatenate([fx.ea[e][None], st])
        assert ((pts >= TR.LO + 1e-3) & (pts <= TR.HI - 1e-3)).all()
        m = np.asarray(TR.margins(TR.mode_torques(pts, None, None, fx.emode[e], fx.emass[e])),
                       dtype=np.float64)
        d = m[k + 1, j]
        assert fx.edelta[e] <= fx.eside[e] * d <= fx.edelta[e] + 1e-12 and d == fx.emargin[e]
        m[k + 1, j] = -np.inf
        clear = TR.CLEAR if fx.ekpos[e] == 2 else TR.EDGE_CLEAR_PEAK
        assert m[:, j].max() <= -clear
        m[:, j] = -np.inf
        assert m.max() <= -TR.CLEAR
        assert k == (0, fx.nsteps[e] // 2, fx.nsteps[e] - 1)[fx.ekpos[e]] and fx.nsteps[e] >= 4
        assert fx.nsafe[e] == (k if fx.eside[e] > 0 else fx.nsteps[e])
        kk = (fx.emode[e], j, fx.ekpos[e], fx.eside[e], fx.edelta[e])
        keys[kk] = keys.get(kk, 0) + 1
    assert set(keys.values()) == {G.EDGE_PER}
    assert len(keys) == len(G.EDGE_GROUPS) * 3 * 2 * len(fx.levels)
    want = np.where(fx.e_kpos == 2, TR.CLEAR, TR.EDGE_CLEAR_PEAK)     # the stored clearances
    assert (fx.e_clear_before >= want).all() and (fx.e_clear_after >= want).all()
    assert (fx.emass == 5.0).all()


def test_goal_rows_and_rewire_case_obey_their_rules(fx):
    """The goal search's rows sit 1e-6 and 1e-3 Nm from the limit with every other joint 0.5 Nm
    inside.  The rewire case: the goal edge fails at once; a -> C and C' -> S are clear; C' is
    nearer to S than a; the edge a -> nw has its probe at step k, 1e-9 Nm on either side, the
    other steps clear; and the oracle's replay gives the expected parents (it also shows that the
    oracle maps the uniform draws to the samples this file computes)."""
    m = np.asarray(TR.margins(TR.mode_torques(fx.gq, None, None, fx.gmode, fx.gmass)),
                   dtype=np.float64)
    r = np.arange(len(fx.gq))
    d = m[r, fx.gjoint]
    assert ((fx.gside * d >= fx.gdelta) & (fx.gside * d <= fx.gdelta + 1e-12)).all()
    m[r, fx.gjoint] = -np.inf
    assert (m <= -TR.CLEAR).all()
    assert ((fx.gq >= TR.LO + 1e-3) & (fx.gq <= TR.HI - 1e-3)).all()
    assert len(fx.gq) == 4 * len(fx.g_base) == 576 and fx.gok.sum() == 288

    mode, mass, j, k = int(fx.r_mode), float(fx.r_mass), int(fx.r_joint), int(fx.r_k)
    ext = lambda a, b: np.array(MC.extend_ref(a, b, 0.1 * np.ones(7)))  # noqa: E731
    marg = lambda pts: np.asarray(TR.margins(TR.mode_torques(pts, None, None, mode, mass)),  # noqa: E731
                                  dtype=np.float64)
    a = fx.r_a
    assert marg(ext(a, fx.r_goal)[:1])[0, j] >= TR.CLEAR and marg(a[None]).max() <= -G.REWIRE_CLEAR
    C = (1 - fx.r_uC) * TR.LO + fx.r_uC * TR.HI
    st = ext(a, C)
    Cn = st[-1]
    assert marg(st).max() <= -0.2
    for v in (0, 1):
        S = (1 - fx.r_uS[v]) * TR.LO + fx.r_uS[v] * TR.HI
        walk = ext(Cn, S)
        nw = walk[-1]
        assert marg(walk).max() <= -G.REWIRE_CLEAR
        assert np.linalg.norm(Cn - S) < np.linalg.norm(a - S)
        m = marg(ext(a, nw))
        side = (1, -1)[v]
        assert 1e-9 <= side * m[k, j] <= 1e-9 + 1e-12 and m[k, j] == fx.r_margin[v]
        m[k, j] = -np.inf
        assert m[:, j].max() <= -G.REWIRE_CLEAR
        m[:, j] = -np.inf
        assert m.max() <= -TR.CLEAR
        uni = np.stack([fx.r_uC, fx.r_uS[v]])
        o = O.rrt_run(a, fx.r_goal, 3, None, mode, mass, 1.0, replay_random=[0.9, 0.9],
                      replay_uniform=uni, radius=float(fx.r_radius), tree=True, cull=2)
        assert o["n_nodes"] == 3 and o["tree_cfg"][1].tobytes() == Cn.tobytes()
        assert o["tree_cfg"][2].tobytes() == nw.tobytes()
        assert list(o["tree_parent"]) == [-1, 0, int(fx.r_parent[v])] and o["n_rewires"] == v
    assert list(fx.r_parent) == [1, 0]


def test_oracle_decides_every_probe(fx):
    """oracle.torque_ok and oracle.check_edge on every probe: the fixture's decision, which holds
    the oracle to the band (static rows with no rates and with zero rates)."""
    for i in range(fx.n):
        got = O.torque_ok(fx.q[i], fx.mode[i], fx.mass[i], fx.qd[i], fx.qdd[i])
        assert got == fx.ok[i], (i, fx.names[i])
        if fx.names[i] in TR.STATIC + ("dyn_static",):
            assert O.torque_ok(fx.q[i], fx.mode[i], fx.mass[i]) == fx.ok[i], i
            if fx.names[i] in TR.STATIC:
                assert O.torque_ok(fx.q[i], TR.MODE_RNE, fx.mass[i]) == fx.ok[i], i
    for i in range(len(fx.gq)):
        assert O.torque_ok(fx.gq[i], fx.gmode[i], fx.gmass[i]) == fx.gok[i], i
    none = np.zeros((0, 15))
    for e in range(fx.m):
        s, n, last = O.check_edge(fx.ea[e], fx.eb[e], none, fx.emode[e], fx.emass[e], cull=2)
        assert (s, n) == (fx.nsafe[e], fx.nsteps[e]), e
        if s:
            assert last.tobytes() == fx.last[e].tobytes(), e


def test_a_nan_torque_passes():
    """`not (|tau| >= L)`: a NaN torque passes, in the reference's `if abs(t) >= L: return False`,
    in the oracle and in the kernels' comparison alike."""
    q = np.full(7, np.nan)
    for mode in (TR.MODE_NOV, TR.MODE_RNE, TR.MODE_DYN):
        assert O.torque_ok(q, mode, 5.0)
    assert TR.decide(TR.mode_torques(q[None], None, None, TR.MODE_RNE, 5.0))[0]
