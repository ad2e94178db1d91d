"""GPU: velocity-profile retiming (tcmp_retime_profile_traj, tcmp_plan_retime_profile;
csrc/tcmp_retime_profile.h) against the restatement in tests/retime_profile_ref.py.

The coefficients (coef_out) are compared with the CPU oracle's to the project's RNE pin: 1e-9 on
g, 2e-9 on m and d (differences of two pinned torques).  Everything after them is exact: the
restatement's sweep fed the device's own coefficients reproduces x, u, psg', the status and the
record bit for bit, and the new rows equal the host's recomputation from the returned x and u.
Per mode one batched call carries every stand-alone case (the sweep kernel stages the uniform
floor in chunks of 64 rows, the coefficient kernel in blocks of 256), with and without psg; the
restatement runs once per call and the tests share it.
"""
import numpy as np
import pytest

import oracle as O  # noqa: E402  (test infrastructure)
import retime_profile_ref as RP
import retime_ref as R
import test_gpu_retime as TG

pytestmark = pytest.mark.gpu

MASS = TG.MASS
SENT = -7.25   # what x_out / u_out hold where the call leaves them alone


@pytest.fixture(scope="module")
def eng():
    from torque_constrained_motion_planning_amd import _lib
    return _lib.engine(0)


# ---- the cases -------------------------------------------------------------------------------
# (n, planted row): tests/test_gpu_retime.py's planted rows around 1, 2, 3, the sweep's chunk of
# 64 rows and the coefficient kernel's block of 256
PLANTED = [(1, 0), (2, 1), (3, 1), (63, 62), (64, 0), (65, 64), (255, 254), (256, 0), (257, 256)]
# (waypoints, rows per segment, duration): min-jerk rows short enough to violate at 5 kg
MINJERK = [(2, 8, 0.5), (3, 33, 1.0), (4, 100, 1.0), (5, 8, 1.0), (3, 100, 1.5), (5, 33, 1.0),
           (2, 100, 4.0)]
_built = {}


def minjerk_case(eng, k, mode):
    """Engine min-jerk rows of waypoints that pass the mode's static test with 3 N m to spare
    (rows between them may not: such a trajectory is INFEASIBLE or not anchored, a case like any
    other); the last case is a short slow move that passes as it is."""
    W, ni, T = MINJERK[k]
    P = TG._feasible(np.random.default_rng(50 + k), W, mode if mode else R.RNE, MASS)
    if k == len(MINJERK) - 1:
        P[1] = P[0] + np.random.default_rng(7).uniform(-0.1, 0.1, 7)
    q, v, a = eng.minjerk(P, ni)
    seg = T / (W - 1)
    return q, v / seg, a / (seg * seg), np.arange(len(q)) * (seg / ni)


def infeasible_case(mode):
    """70 mild rows with a row at rest that fails the static test at 40, and another at 12."""
    q, v, a, psg = (x.copy() for x in TG.case(70, None, mode))
    bad = TG._feasible(np.random.default_rng(5), 2, R.RNE, MASS, want=False)
    for i, b in zip((12, 40), bad):
        q[i], v[i], a[i] = b, 0.0, 0.0
    return q, v, a, psg


def build(eng, mode):
    """Every stand-alone case of a mode -> (names, offsets, q, v, a, psg)."""
    if mode in _built:
        return _built[mode]
    parts = [("planted%d" % n, TG.case(n, plant, mode)) for n, plant in PLANTED]
    parts += [("minjerk%d" % k, minjerk_case(eng, k, mode)) for k in range(len(MINJERK))]
    parts.append(("passing", TG.case(257, None, mode)))
    # the batch of three: 1, 70 and 257 rows, the middle one INFEASIBLE (base: no constraint)
    parts += [("three_a", TG.case(1, 0, mode)), ("three_b", infeasible_case(mode)),
              ("three_c", TG.case(257, 64, mode))]
    # 65 short trajectories (past a block's four wavefronts and more), lengths 0 .. 4 in turn
    q, v, a, psg = TG.case(3000, 256, mode)
    at = 0
    for t in range(65):
        m = t % 5
        parts.append(("short%d" % t, (q[at:at + m], v[at:at + m], a[at:at + m], psg[at:at + m])))
        at += m + 1
    off = np.concatenate([[0], np.cumsum([len(p[1][0]) for p in parts])]).astype(np.int64)
    cat = [np.concatenate([p[1][k] for p in parts]) for k in range(4)]
    _built[mode] = ([p[0] for p in parts], off, *cat)
    return _built[mode]


def call(eng, mode, q, v, a, psg, off, **kw):
    """Engine.retime_profile with sentinels in x / u, so that what the call leaves alone shows."""
    from torque_constrained_motion_planning_amd import _lib
    import ctypes
    n, nt = len(q), len(off) - 1
    cfg = _lib.RetimeCfg(float(kw.get("min_scale", 1.0)), float(kw.get("max_scale", 0.0)))
    res = (_lib.RetimeProfileResult * max(nt, 1))()
    ms = ctypes.c_double(0.0)
    o = dict(qd=v.copy(), qdd=a.copy(), psg=None if psg is None else psg.copy(),
             x=np.full(n, SENT), u=np.full(n, SENT), coef=np.full((n, 18), SENT))
    d = _lib._d
    eng._check(eng.L.tcmp_retime_profile_traj(
        eng.h, d(q), d(v), d(a), d(psg), off.ctypes.data_as(_lib._i64p), nt, mode, MASS,
        ctypes.byref(cfg), d(o["qd"]), d(o["qdd"]), d(o["psg"]), d(o["x"]), d(o["u"]),
        d(o["coef"]), res, ctypes.byref(ms)))
    o.update(results=list(res[:nt]), ms=ms.value)
    return o


_runs = {}


def run(eng, mode, with_psg=True):
    """One batched call per (mode, psg), the restatement on the device's coefficients per
    trajectory, and the oracle's coefficients: computed once, read by every test."""
    key = (mode, with_psg)
    if key not in _runs:
        names, off, q, v, a, psg = build(eng, mode)
        p = np.ascontiguousarray(psg) if with_psg else None
        out = call(eng, mode, q, v, a, p, off)
        refs = []
        for t in range(len(names)):
            b, e = off[t], off[t + 1]
            refs.append(RP.sweep(out["coef"][b:e], None if p is None else p[b:e]))
        _runs[key] = dict(names=names, off=off, q=q, v=v, a=a, psg=p, out=out, refs=refs)
        print("mode %d psg %s: %d trajectories, %d rows, %.3f ms" % (mode, with_psg, len(names),
                                                                    len(q), out["ms"]))
    return _runs[key]


FIELDS = ("status", "anchored", "uniform_status", "n_rows", "fail_row", "x_uniform", "x_floor",
          "x_min", "n_at_floor", "n_at_cap", "time_before", "time_after", "time_uniform")


def bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


# ---- the assertions --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_coefficients_agree_with_the_oracle(eng, mode):
    """1: the RNE pin.  (base has no coefficients: all zero.)"""
    c = run(eng, mode)
    ref = RP.coefficients(c["q"], c["v"], c["a"], mode, MASS)
    err = np.abs(c["out"]["coef"] - ref)
    print("max |g| %.3g |m| %.3g |d| %.3g" % (err[:, :6].max(), err[:, 6:12].max(),
                                              err[:, 12:].max()))
    assert err[:, :6].max() <= 1e-9 and err[:, 6:].max() <= 2e-9
    # a row at rest, and every row of nov: m = d = 0 exactly
    rest = ~(c["v"].any(axis=1) | c["a"].any(axis=1))
    assert rest.sum() >= 2 and not c["out"]["coef"][rest, 6:].any()
    if mode == R.NOV:
        assert not c["out"]["coef"][:, 6:].any()


def test_base_mode_has_no_constraint(eng):
    c = run(eng, R.BASE)
    assert not c["out"]["coef"].any()
    assert all(r.status == 0 and r.anchored == 1 and r.x_min == 1.0 for r in c["out"]["results"])
    assert bits(c["out"]["qd"]) == bits(c["v"]) and bits(c["out"]["qdd"]) == bits(c["a"])


@pytest.mark.parametrize("with_psg", [True, False])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_restatement_on_device_coefficients_is_bit_exact(eng, mode, with_psg):
    """2, 3, 5, 7: the sweep, the rows, the anchored guarantees, what is left alone."""
    from torque_constrained_motion_planning_amd import _lib
    c = run(eng, mode, with_psg)
    out, off = c["out"], c["off"]
    seen = set()
    for t, (name, ref, r) in enumerate(zip(c["names"], c["refs"], out["results"])):
        b, e = off[t], off[t + 1]
        got = r.as_dict()
        assert [got[k] for k in FIELDS] == [ref[k] for k in FIELDS], (name, got, ref)
        assert got["exec_time_after"] == 0.0 and got["pad"] == 0
        seen.add((r.status, r.anchored))
        v, a = c["v"][b:e], c["a"][b:e]
        if r.status != _lib.RETIME_OK:
            # 7: nothing of this trajectory is written
            assert r.status == _lib.RETIME_INFEASIBLE and r.first_fail_after == r.first_fail_before
            assert (out["x"][b:e] == SENT).all() and (out["u"][b:e] == SENT).all()
            assert bits(out["qd"][b:e]) == bits(v) and bits(out["qdd"][b:e]) == bits(a)
            if with_psg:
                assert bits(out["psg"][b:e]) == bits(c["psg"][b:e])
            continue
        assert r.first_fail_after == -1
        if e == b:
            continue
        assert bits(out["x"][b:e]) == bits(ref["x"]) and bits(out["u"][b:e]) == bits(ref["u"]), name
        if with_psg:
            assert bits(out["psg"][b:e]) == bits(ref["psg"]), name
        # 3: the rows from the returned x and u
        qd, qdd = RP.apply_rows(v, a, out["x"][b:e], out["u"][b:e])
        assert bits(out["qd"][b:e]) == bits(qd) and bits(out["qdd"][b:e]) == bits(qdd), name
        # 5
        if r.anchored:
            assert (out["x"][b:e] >= r.x_uniform).all() and r.time_after <= r.time_uniform
    if mode >= R.RNE:
        assert (_lib.RETIME_OK, 1) in seen and (_lib.RETIME_INFEASIBLE, 0) in seen
    # the batch of three holds its INFEASIBLE trajectory between two OK ones
    i = c["names"].index("three_b")
    st = [out["results"][k].status for k in (i - 1, i, i + 1)]
    assert st == ([0, 0, 0] if mode == R.BASE else [0, _lib.RETIME_INFEASIBLE, 0])
    if mode != R.BASE:
        assert out["results"][i].fail_row == 40


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_ok_trajectories_pass_the_oracle(eng, mode):
    """4, with the first failing rows as given, and the gain over the uniform retiming."""
    c = run(eng, mode)
    out, off = c["out"], c["off"]
    faster = 0
    for t, (name, r) in enumerate(zip(c["names"], out["results"])):
        b, e = off[t], off[t + 1]
        if name.startswith("short") and t % 4:
            continue                       # (a quarter of the short ones: they are all alike)
        q, v, a = c["q"][b:e], c["v"][b:e], c["a"][b:e]
        assert r.first_fail_before == R.first_fail(q, v, a, mode, MASS), name
        if r.status == 0:
            assert R.all_pass(q, out["qd"][b:e], out["qdd"][b:e], mode, MASS), name
        if name.startswith("minjerk") and r.x_uniform < 1.0:
            print("%s: time %.4f -> profile %.4f, uniform %.4f" % (name, r.time_before,
                                                                    r.time_after, r.time_uniform))
            faster += r.time_after < 0.9 * r.time_uniform
    if mode >= R.RNE:
        assert faster >= 3


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_a_passing_trajectory_keeps_its_bytes(eng, mode):
    """6"""
    c = run(eng, mode)
    out, off = c["out"], c["off"]
    for name in ("passing", "minjerk%d" % (len(MINJERK) - 1)):
        t = c["names"].index(name)
        b, e = off[t], off[t + 1]
        r = out["results"][t]
        assert (r.status, r.anchored, r.x_uniform, r.first_fail_before) == (0, 1, 1.0, -1), name
        assert (out["x"][b:e] == 1.0).all() and bits(out["u"][b:e]) == bits(np.zeros(e - b))
        for k, src in (("qd", "v"), ("qdd", "a"), ("psg", "psg")):
            assert bits(out[k][b:e]) == bits(c[src][b:e]), (name, k)
        assert r.time_after == r.time_before == r.time_uniform
        assert r.n_at_floor == r.n_at_cap == e - b


def test_single_trajectory_calls_and_determinism(eng):
    """A batch of one equals its slice of the large batch; 8: two equal calls, equal bytes."""
    from torque_constrained_motion_planning_amd import _lib
    c = run(eng, R.DYN)
    for name in ("minjerk2", "planted257", "three_b"):
        t = c["names"].index(name)
        b, e = c["off"][t], c["off"][t + 1]
        args = (c["q"][b:e], c["v"][b:e], c["a"][b:e], c["psg"][b:e],
                np.array([0, e - b], dtype=np.int64))
        one, two = call(eng, R.DYN, *args), call(eng, R.DYN, *args)
        for k in ("qd", "qdd", "psg", "x", "u", "coef"):
            assert bits(one[k]) == bits(two[k]) == bits(c["out"][k][b:e]), (name, k)
        da, db, dc = (r.as_dict() for r in (one["results"][0], two["results"][0],
                                            c["out"]["results"][t]))
        for d in (da, db, dc):
            d.pop("ms")
        assert da == db == dc
    # the public wrapper: rows as given where the status is not OK, x = 1 and u = 0 there
    t = c["names"].index("three_b")
    b, e = c["off"][t], c["off"][t + 1]
    o = eng.retime_profile(c["q"][b:e], c["v"][b:e], c["a"][b:e], R.DYN, MASS, psg=c["psg"][b:e])
    assert o["results"][0].status == _lib.RETIME_INFEASIBLE and (o["x"] == 1.0).all()
    assert bits(o["qd"]) == bits(c["v"][b:e])


def test_not_anchored_rescue_cap_and_speed_up(eng):
    """Rows the uniform retiming calls INFEASIBLE (tests/test_gpu_retime.py's static row and a
    violent row below its x_lo), min_scale below 1, and a cap that only moves the floor."""
    from torque_constrained_motion_planning_amd import _lib
    qs, vs, as_ = TG._static_rows(True)
    q, v, a, psg = (x.copy() for x in TG.case(70, None, R.RNE))
    q[66], v[66], a[66] = qs, vs, as_
    lo = R.retime(qs, vs, as_, R.RNE, MASS, min_scale=0.25)["x_lo"]
    TG._plant(q, v, a, 5, R.RNE, MASS, np.random.default_rng(2), 0.5 * lo)
    off = np.array([0, 70], dtype=np.int64)
    _, _, _, ru = eng.retime(q, v, a, R.RNE, MASS, psg=psg, min_scale=0.25)
    assert ru.status == _lib.RETIME_INFEASIBLE
    for kw in (dict(min_scale=0.25), dict(min_scale=0.25, max_scale=50.0)):
        o = call(eng, R.RNE, q, v, a, psg, off, **kw)
        r = o["results"][0]
        ref = RP.sweep(o["coef"], psg, **kw)
        assert [r.as_dict()[k] for k in FIELDS] == [ref[k] for k in FIELDS]
        assert (r.status, r.anchored, r.uniform_status) == (0, 0, _lib.RETIME_INFEASIBLE)
        assert r.x_floor == (1.0 / 2500.0 if "max_scale" in kw else 1e-6) and r.time_uniform == 0.0
        assert bits(o["x"]) == bits(ref["x"]) and bits(o["u"]) == bits(ref["u"])
        assert o["x"][5] < lo < o["x"][66] and o["x"].max() <= 16.0
        assert R.all_pass(q, o["qd"], o["qdd"], R.RNE, MASS)
    # bounds above 1 and min_scale = 0.5: played faster, never slower than the uniform retiming
    q, v, a, psg = TG.case(257, 64, R.RNE, (2.5, 3.2))
    off = np.array([0, 257], dtype=np.int64)
    o = call(eng, R.RNE, q, v, a, psg, off, min_scale=0.5)
    r = o["results"][0]
    ref = RP.sweep(o["coef"], psg, min_scale=0.5)
    assert [r.as_dict()[k] for k in FIELDS] == [ref[k] for k in FIELDS]
    assert r.status == 0 and r.anchored == 1 and 2.4 < r.x_uniform < 2.6
    assert (o["x"] >= r.x_uniform).all() and o["x"].max() == 4.0 and r.n_at_cap > 0
    assert r.time_after <= r.time_uniform < r.time_before
    assert R.all_pass(q, o["qd"], o["qdd"], R.RNE, MASS)
    # an over-cap uniform retiming is not an anchor, and the cap is the floor of every set
    o = call(eng, R.RNE, *TG.case(257, 64, R.RNE), off, max_scale=1.2)
    r = o["results"][0]
    assert (r.status, r.anchored, r.uniform_status) == (_lib.RETIME_INFEASIBLE, 0,
                                                        _lib.RETIME_OVER_CAP)
    assert r.x_floor == 1.0 / (1.2 * 1.2) and r.fail_row == 64   # the floor is above its bound


def test_no_rows_and_argument_errors(eng):
    from torque_constrained_motion_planning_amd import _lib
    z = np.zeros((0, 7))
    o = eng.retime_profile(z, z, z, R.RNE, MASS, min_scale=0.5, traj_off=[0, 0, 0])
    assert [(r.status, r.anchored, r.x_uniform, r.x_min, r.n_rows, r.fail_row)
            for r in o["results"]] == [(0, 1, 4.0, 4.0, 0, -1)] * 2
    q, v, a, psg = TG.case(3, 1, R.RNE)
    with pytest.raises(_lib.TcmpError):
        eng.retime_profile(q, v, a, R.RNE, MASS, psg=np.array([0.0, 1.0, 1.0]))   # D_1 = 0
    with pytest.raises(_lib.TcmpError):
        eng.retime_profile(q, v, a, R.RNE, MASS, traj_off=[0, 2, 1, 3])
    with pytest.raises(_lib.TcmpError):
        eng.retime_profile(q, v, a, R.RNE, MASS, min_scale=2.0)
    with pytest.raises(_lib.TcmpError):
        eng.retime_profile(q, v, a, 7, MASS)
    # psg may restart between trajectories: only the steps inside one must ascend
    o = eng.retime_profile(np.vstack([q, q]), np.vstack([v, v]), np.vstack([a, a]), R.RNE, MASS,
                           psg=np.concatenate([psg, psg]), traj_off=[0, 3, 6])
    assert [r.status for r in o["results"]] == [0, 0]
    assert bits(o["x"][:3]) == bits(o["x"][3:])


# ---- plan form -------------------------------------------------------------------------------
def test_plan_retime_profile_on_the_failing_query(eng):
    """9: tests/test_gpu_retime.py's 5 kg dyn query, whose validation fails on one row."""
    from torque_constrained_motion_planning_amd import _lib
    e, e2 = TG.fresh(), TG.fresh()
    try:
        TG.grow(e)
        fin = e.plan_finish()
        assert fin.status == _lib.PLAN_VALIDATION_FAILED
        before = e.plan_fetch(fin)
        rt = e.plan_retime_profile()
        after = e.plan_fetch(fin)
        assert (rt.status, rt.anchored, rt.n_rows, rt.first_fail_before, rt.first_fail_after) == \
            (_lib.RETIME_OK, 1, fin.n_traj, fin.first_fail, -1)
        # the fetched rows equal the stand-alone call on the fetched pre-retime rows
        o = eng.retime_profile(before["q"], before["qd"], before["qdd"], R.DYN, MASS,
                               psg=before["psg"])
        assert o["results"][0].status == _lib.RETIME_OK
        for k in ("qd", "qdd", "psg"):
            assert bits(after[k]) == bits(o[k]), k
        TG.same_rows(before, after, ("waypoints", "q"))
        a, b = rt.as_dict(), o["results"][0].as_dict()
        for d in (a, b):
            d.pop("ms"), d.pop("exec_time_after")
        assert a == b
        assert R.all_pass(after["q"], after["qd"], after["qdd"], R.DYN, MASS)
        # tau is recomputed
        tau = eng.rne(after["q"], after["qd"], after["qdd"], 0.0)
        assert np.abs(after["tau"] - tau).max() <= 1e-9
        assert np.abs(after["tau"] - before["tau"]).max() > 1e-3
        # never slower than the uniform retiming of the same plan on a second engine
        TG.grow(e2)
        fin2 = e2.plan_finish()
        ru = e2.plan_retime()
        assert ru.status == _lib.RETIME_OK and rt.x_uniform == ru.x
        assert rt.exec_time_after == TG.Q_EXEC * rt.time_after / rt.time_before
        print("exec time %.4f: profile %.4f, uniform %.4f; ms %.4f" % (
            TG.Q_EXEC, rt.exec_time_after, ru.exec_time_after, rt.ms))
        assert rt.exec_time_after <= ru.exec_time_after
        assert rt.time_after <= rt.time_uniform
        # NOT_APPLICABLE: every retiming form and the repair after it, until the next finish
        NA = _lib.RETIME_NOT_APPLICABLE
        assert e.plan_retime_profile().status == NA and e.plan_retime().status == NA
        assert e.plan_retime_runs()[1].status == NA
        assert e.plan_repair().status == _lib.REPAIR_NOT_APPLICABLE
        TG.same_rows(e.plan_fetch(fin), after)
        # ... after either other retiming
        assert e2.plan_retime_profile().status == NA
        fin = e.plan_finish()
        TG.same_rows(e.plan_fetch(fin), before)
        assert e.plan_retime_runs()[1].status == _lib.RETIME_OK
        kept = e.plan_fetch(fin)
        assert e.plan_retime_profile().status == NA
        TG.same_rows(e.plan_fetch(fin), kept)
        # ... and after a shortcut; a new finish makes it applicable again
        e.plan_finish()
        e.plan_shortcut()
        assert e.plan_retime_profile().status == NA
        fin = e.plan_finish()
        assert e.plan_retime_profile().status in (_lib.RETIME_OK, _lib.RETIME_INFEASIBLE)
        # a retrace-only finish has no rows
        e.plan_retrace()
        assert e.plan_retime_profile().status == NA
    finally:
        e.close()
        e2.close()


def test_batched_profile_retime():
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_batched
    e = TG.fresh()
    try:
        args = (TG.Q_START, TG.Q_GOAL, [], R.DYN, MASS, TG.Q_EXEC, TG.Q_SAMPLES)
        kw = dict(batch=TG.Q_BATCH, seed=TG.Q_SEED, engine=e)
        (path, vels, accels, psg), r, raw = rrt_star_batched(*args, retime="profile", **kw)
        rt = raw["retime"]
        assert isinstance(rt, _lib.RetimeProfileResult) and rt.status == _lib.RETIME_OK
        assert path is not None and r.status == _lib.PLAN_OK and r.first_fail == -1
        assert R.all_pass(path, vels, accels, R.DYN, MASS)
        assert psg[-1] - psg[0] == rt.time_after
        with pytest.raises(ValueError):
            rrt_star_batched(*args, retime="fastest", **kw)
    finally:
        e.close()


def test_drop_in_foreign_dynam_fn_goes_through_engine_retime_profile(monkeypatch):
    """rrt_star_force_aware with a foreign dynam_fn that plays the package's min-jerk five times
    faster (tests/test_gpu_retime.py's): retime="profile" hands its rows and psg to
    Engine.retime_profile."""
    import os
    import random
    from conftest import GOLDEN
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd import panda_primitives as PP
    from torque_constrained_motion_planning_amd import utils as U
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_force_aware
    z = np.load(os.path.join(GOLDEN, "rrt_empty_rne5.npz"))
    mode, mass = int(z["mode"]), float(z["mass"])
    prob = U.Problem(U.PandaRobot(), list(z["obs"]), U.Payload(mass), mass, float(z["exec_time"]),
                     torque_test="rne", retime="profile")
    assert prob.retime == "profile"
    resolutions = 0.2 ** np.ones(7)
    radius = resolutions / 2
    joints = U.get_arm_joints(prob.robot)
    native = PP.get_dynamics_fn_v5(prob, resolutions)
    K = 5.0
    rows = {}

    def fast(path, n):
        q, psg, qd, qdd = native(path, n)
        qd = [list(np.asarray(x) * K) for x in qd]
        qdd = [list(np.asarray(x) * (K * K)) for x in qdd]
        rows.update(q=np.asarray(q), qd=np.asarray(qd), qdd=np.asarray(qdd), psg=np.asarray(psg))
        return q, psg, qd, qdd
    args = (tuple(z["start"]), tuple(z["goal"]),
            U.get_distance_fn(prob.robot, joints, weights=np.reciprocal(radius)),
            U.get_sample_fn(prob.robot, joints),
            U.get_extend_fn(prob.robot, joints, resolutions=radius),
            U.get_collision_fn(prob.robot, joints, list(z["obs"]), self_collisions=False),
            PP.select_torque_test(prob), fast)
    calls = []
    real = _lib.Engine.retime_profile

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        calls.append((k.get("psg"), out))
        return out
    monkeypatch.setattr(_lib.Engine, "retime_profile", spy)
    random.seed(int(z["seed"]))
    np.random.seed(int(z["seed"]))
    path, vels, accels, psg = rrt_star_force_aware(*args, radius=[0.01], max_time=50,
                                                   max_iterations=int(z["iters"]),
                                                   retime="profile")
    assert len(calls) == 1 and bits(calls[0][0]) == bits(rows["psg"])
    o = calls[0][1]
    r = o["results"][0]
    assert r.status == _lib.RETIME_OK and r.first_fail_before >= 0
    assert r.anchored == 1 and r.x_uniform < 1.0 and r.time_after <= r.time_uniform
    assert bits(path) == bits(rows["q"])
    assert bits(vels) == bits(o["qd"]) and bits(accels) == bits(o["qdd"]) and bits(psg) == bits(o["psg"])
    assert R.all_pass(path, vels, accels, mode, mass)
    with pytest.raises(ValueError):
        rrt_star_force_aware(*args, radius=[0.01], max_iterations=1, retime="fastest")
