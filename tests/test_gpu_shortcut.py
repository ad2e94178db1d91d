"""GPU: force-aware path shortcutting (tcmp_shortcut_path, tcmp_plan_shortcut; csrc/
tcmp_shortcut.h) against the restatement in tests/shortcut_ref.py, whose chord checks are the CPU
oracle's check_edge (resolutions 0.1, weights 10: the planner's defaults, used throughout).

Waypoints bit for bit; counts equal; costs within 1e-12 relative (the project's tolerance for
tree costs); trajectories of shortened plans within 1e-12 of oracle.minjerk.  Every fixture's
seed was chosen so that the restatement uses at least one chord and rejects at least one (a
case with one chord only comes in both flavours); the tests assert that again.
"""
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, engine_with_split

import oracle as O  # noqa: E402  (test infrastructure)
import shortcut_ref as SR

pytestmark = pytest.mark.gpu

LO = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
HI = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])
START = np.array([0, -np.pi / 4, 0.0, -6 * np.pi / 8, 0, np.pi / 2, np.pi / 4])
NO_OBS = np.zeros((0, 15))

# name: (scene, n, max_anchors, passes, seed, options)
#   scene: (kind, count, torque mode, payload mass)
#   options: step = the zig-zag's largest joint step (about step / 0.07 points per hop);
#            verts = the vertices alone (hops longer than one extend step, so a chord can hold
#            more points than it replaces); free = unconstrained vertices
CASES = {
    "n1": (("box", 0, 2, 5.0), 1, 512, 1, 1, {}),
    "n2": (("box", 0, 2, 5.0), 2, 512, 1, 1, {}),
    "n3_used": (("box", 4, 2, 5.0), 3, 512, 1, 1, dict(verts=True)),
    "n3_rejected": (("box", 4, 2, 5.0), 3, 512, 1, 23, dict(verts=True)),
    "n40_empty_rne5": (("box", 0, 2, 5.0), 40, 512, 1, 8, dict(step=0.5)),
    "n40_box4": (("box", 4, 2, 5.0), 40, 512, 1, 6, dict(step=0.5)),
    "n40_box16": (("box", 16, 2, 5.0), 40, 512, 1, 7, dict(step=0.5)),
    "n40_mesh8": (("mesh", 8, 1, 2.0), 40, 512, 1, 5, dict(step=0.5)),
    # (14 anchors, stride 3: the oracle's self-collision test takes ~15 ms per chord)
    "n40_self": (("self", 0, 0, 0.0), 40, 14, 1, 11, dict(step=0.9, free=True)),
    "n300_a64": (("box", 4, 2, 5.0), 300, 64, 1, 1, dict(step=0.5)),
    "n9_a2_used": (("box", 4, 2, 5.0), 9, 2, 1, 1, dict(step=0.1)),
    "n9_a2_rejected": (("box", 4, 2, 5.0), 9, 2, 1, 37, dict(verts=True)),
    "n40_box16_passes3": (("box", 16, 2, 5.0), 40, 512, 3, 7, dict(step=0.5)),
    # more than 256 hops survive (the splice's second prefix-sum chunk): unconstrained vertices
    # under a payload most configurations cannot hold, so most chords fail and the original hops
    # stay
    "n300_hops": (("box", 0, 2, 9.0), 300, 512, 1, 34, dict(step=0.5, free=True)),
}
ONE_CHORD = {"n3_used": 1, "n3_rejected": 0, "n9_a2_used": 1, "n9_a2_rejected": 0}


def build_case(name):
    """-> dict(obs, pack, self_coll, mode, mass, W, a_max, passes); installs the oracle's scene
    state (meshes, self-collision), which conftest's autouse fixture resets."""
    from torque_constrained_motion_planning_amd.scene import (mesh_pack, obstacle_array,
                                                              random_box_scene,
                                                              random_mesh_scene)
    (kind, count, mode, mass), n, a_max, passes, seed, opt = CASES[name]
    rng = np.random.default_rng(seed)
    obs, pack = NO_OBS, None
    if kind == "box" and count:
        obs = obstacle_array(random_box_scene(rng, count, aligned=False))
    if kind == "mesh":
        pack = mesh_pack(random_mesh_scene(rng, count))
    O.set_meshes(pack)
    O.set_self_collision(kind == "self")
    W = SR.zigzag(O, rng, n, obs, mode, mass, LO, HI, **opt)
    return dict(obs=obs, pack=pack, self_coll=kind == "self", mode=mode, mass=mass, W=W,
                a_max=a_max, passes=passes)


def reference(c, W=None, a_max=None, passes=None):
    return SR.shortcut(c["W"] if W is None else W, SR.oracle_check(O, c["obs"], c["mode"], c["mass"]),
                       c["a_max"] if a_max is None else a_max,
                       c["passes"] if passes is None else passes)


def install(eng, c):
    eng.set_scene(c["obs"], c["pack"])
    eng.set_self_collision(c["self_coll"])


def same(got, r, ref, st):
    print("n %d -> %d (ref %d); chords tested %d valid %d used %d steps %d (ref %d %d %d %d); "
          "passes %d (ref %d); cost %.17g -> %.17g (ref %.17g -> %.17g)"
          % (r.n_before, r.n_after, st["n_after"], r.chords_tested, r.chords_valid, r.chords_used,
             r.chord_steps, st["chords_tested"], st["chords_valid"], st["chords_used"],
             st["chord_steps"], r.passes_run, st["passes_run"], r.cost_before, r.cost_after,
             st["cost_before"], st["cost_after"]))
    assert r.status == 0
    assert (r.n_before, r.n_after, r.n_anchors) == (st["n_before"], st["n_after"], st["n_anchors"])
    assert (r.chords_tested, r.chords_valid, r.chords_used, r.passes_run) == \
        (st["chords_tested"], st["chords_valid"], st["chords_used"], st["passes_run"])
    assert r.chord_steps == st["chord_steps"]
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    for a, b in ((r.cost_before, st["cost_before"]), (r.cost_after, st["cost_after"])):
        assert abs(a - b) <= 1e-12 * max(abs(b), 1e-300)
    assert r.cost_after <= r.cost_before


@pytest.fixture(scope="module")
def eng():
    from torque_constrained_motion_planning_amd import _lib
    e = _lib.engine(0)
    yield e
    e.set_self_collision(False)


@pytest.mark.parametrize("name", list(CASES))
def test_shortcut_path_vs_restatement(eng, name):
    c = build_case(name)
    ref, st = reference(c)
    rejected = st["chords_tested"] - st["chords_valid"]
    if name in ("n1", "n2"):
        assert st["chords_tested"] == 0 and ref.tobytes() == c["W"].tobytes()
    elif name in ONE_CHORD:
        assert (st["chords_tested"], st["chords_valid"], st["chords_used"]) == \
            (1, ONE_CHORD[name], ONE_CHORD[name])
    else:
        assert st["chords_used"] >= 1 and rejected >= 1, (st, "the fixture proves nothing")
    if name == "n300_hops":
        assert st["max_hops"] > 256
    if name == "n40_box16_passes3":
        assert st["passes_run"] >= 2
    install(eng, c)
    got, r = eng.shortcut_path(c["W"], c["mode"], c["mass"], max_anchors=c["a_max"],
                               passes=c["passes"])
    same(got, r, ref, st)
    assert got[0].tobytes() == c["W"][0].tobytes() and got[-1].tobytes() == c["W"][-1].tobytes()


@pytest.mark.parametrize("split", [1, 2])
def test_shortcut_path_edge_kernel_variants(split):
    """The chords through k_edges<., 1> and k_edges<., 2> (the default engine takes 4 lanes per
    edge at these sizes)."""
    c = build_case("n40_box16")
    ref, st = reference(c)
    e = engine_with_split(split)
    try:
        install(e, c)
        got, r = e.shortcut_path(c["W"], c["mode"], c["mass"])
        same(got, r, ref, st)
    finally:
        e.close()


def test_shortcut_path_arguments(eng):
    from torque_constrained_motion_planning_amd import _lib
    c = build_case("n40_box4")
    install(eng, c)
    for kw in (dict(max_anchors=1), dict(max_anchors=1025), dict(passes=9), dict(passes=-1)):
        with pytest.raises(_lib.TcmpError, match="error -1"):
            eng.shortcut_path(c["W"], c["mode"], c["mass"], **kw)
    # an output too small: -4 with n_after set (tcmp_gather_paths' convention)
    import ctypes
    r = _lib.ShortcutResult()
    out = np.zeros((2, 7))
    W = np.ascontiguousarray(c["W"])
    rc = eng.L.tcmp_shortcut_path(eng.h, _lib._d(W), len(W), None, None, c["mode"], c["mass"],
                                  None, _lib._d(out), 2, ctypes.byref(r))
    assert rc == -4 and r.n_after == reference(c)[1]["n_after"]
    rc = eng.L.tcmp_shortcut_path(eng.h, _lib._d(W), 0, None, None, c["mode"], c["mass"],
                                  None, _lib._d(out), 2, ctypes.byref(r))
    assert rc == -1 and eng.L.tcmp_last_error()


# ---- tcmp_plan_shortcut on real plans --------------------------------------------------------
EXEC = 1.0
# (boxes, scene / goal seed): batched plans at B = 256 that find a goal and whose path the
# restatement shortens while rejecting some chords
PLANS = {"empty": (0, 1), "box4": (4, 7), "box16": (16, 2)}
MODE, MASS, SAMPLES, BATCH = 2, 5.0, 3072, 256


def plan_query(name):
    from torque_constrained_motion_planning_amd.scene import obstacle_array, random_box_scene
    n_obs, seed = PLANS[name]
    rng = np.random.default_rng(seed)
    while True:
        goal = LO + (HI - LO) * rng.random(7)
        obs = obstacle_array(random_box_scene(rng, n_obs)) if n_obs else NO_OBS
        if O.collision(START, obs) or O.collision(goal, obs):
            continue
        if O.torque_ok(goal, MODE, MASS) and O.torque_ok(START, MODE, MASS):
            return dict(obs=obs, pack=None, self_coll=False, mode=MODE, mass=MASS, goal=goal,
                        seed=100 + seed)


def grow(e, q, begin=True):
    from torque_constrained_motion_planning_amd import _lib
    if begin:
        install(e, q)
        assert e.plan_begin(START, q["goal"], q["mode"], q["mass"], EXEC, max_nodes=SAMPLES + 1,
                            max_batch=BATCH, seed=q["seed"]) == _lib.PLAN_OK
    e.plan_run(SAMPLES, BATCH)


def fresh(timing=False):
    from torque_constrained_motion_planning_amd import _lib
    e = _lib.Engine(0)
    e.set_timing(timing)  # off: every ms_* is 0, so whole results compare equal
    return e


def check_finish(q, fin, out, ref):
    """The finished plan against the oracle on the restated list `ref`."""
    from torque_constrained_motion_planning_amd import _lib
    W = len(ref)
    assert fin.n_waypoints == W and out["waypoints"].tobytes() == ref.tobytes()
    ni = int(EXEC * 1000 / W)
    assert ni > 0 and fin.n_traj == (W - 1) * ni
    x, v, a = O.minjerk(ref, ni)
    for got, want in ((out["q"], x), (out["qd"], v), (out["qdd"], a)):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    ff = -1
    for i in range(len(x)):
        if not O.torque_ok(x[i], q["mode"], q["mass"], v[i], a[i]):
            ff = i
            break
    assert fin.first_fail == ff
    assert fin.status == (_lib.PLAN_VALIDATION_FAILED if ff >= 0 else _lib.PLAN_OK)


NOT_THE_TREES = ("n_waypoints", "n_traj", "first_fail", "status", "ms_finish")


@pytest.mark.parametrize("name", list(PLANS))
def test_plan_shortcut_vs_restatement(name):
    q = plan_query(name)
    e, twin = fresh(), fresh()
    try:
        grow(twin, q)
        rt = twin.plan_retrace()
        assert rt.goal_found == 1
        wp0 = twin.plan_fetch(rt)["waypoints"]
        fin_t = twin.plan_finish()
        ref, st = reference(q, W=wp0, a_max=512, passes=1)
        # (no chord between the waypoints of a plan in the empty scene fails: 79 seeds tried)
        assert st["chords_used"] >= 1, st
        assert name == "empty" or st["chords_tested"] > st["chords_valid"], st
        grow(e, q)
        sc = e.plan_shortcut()
        same(ref, sc, ref, st)
        fin = e.plan_finish()
        out = e.plan_fetch(fin)
        check_finish(q, fin, out, ref)
        a, b = fin.as_dict(), fin_t.as_dict()
        for f in a:
            if f not in NOT_THE_TREES:
                assert a[f] == b[f], (f, a[f], b[f])
    finally:
        e.close()
        twin.close()


def test_plan_shortcut_flag_lifetime():
    from torque_constrained_motion_planning_amd import _lib
    q = plan_query("box4")
    e, other = fresh(), fresh()
    try:
        grow(e, q)
        sc = e.plan_shortcut()
        assert sc.status == 0 and sc.chords_used >= 1
        rt = e.plan_retrace()  # the shortened list, not a new retrace
        assert rt.n_waypoints == sc.n_after and rt.n_traj == 0 and rt.status == 0
        short = e.plan_fetch(rt)["waypoints"]
        fin = e.plan_finish()
        assert fin.n_waypoints == sc.n_after
        assert e.plan_fetch(fin)["waypoints"].tobytes() == short.tobytes()
        # a new plan_begin clears the flag: the plain finish of a fresh engine
        grow(e, q)
        grow(other, q)
        a, b = e.plan_finish(), other.plan_finish()
        assert a.n_waypoints == b.n_waypoints
        oa, ob = e.plan_fetch(a), other.plan_fetch(b)
        for k in ("waypoints", "q", "qd", "qdd"):
            assert oa[k].tobytes() == ob[k].tobytes(), k
        assert (a.status, a.n_traj, a.first_fail, a.edge_steps) == \
            (b.status, b.n_traj, b.first_fail, b.edge_steps)
        assert oa["waypoints"].tobytes() != short.tobytes()
        # no goal node: status NO_GOAL, nothing changes
        for x in (e, other):
            install(x, q)
            assert x.plan_begin(START, q["goal"], q["mode"], q["mass"], EXEC, max_nodes=SAMPLES + 1,
                                max_batch=BATCH, seed=q["seed"]) == _lib.PLAN_OK
        sc = e.plan_shortcut()
        assert sc.status == _lib.PLAN_NO_GOAL
        assert (sc.passes_run, sc.n_before, sc.n_after, sc.chords_tested) == (0, 0, 0, 0)
        a, b = e.plan_finish(), other.plan_finish()
        assert a.status == b.status == _lib.PLAN_NO_GOAL
        assert a.as_dict() == b.as_dict()
    finally:
        e.close()
        other.close()


def test_plan_shortcut_fleet():
    """Two box-scene plans grown in fused rounds, shortcut on each engine, finished together ==
    the same two queries on lone engines with the shortcut."""
    from torque_constrained_motion_planning_amd import _lib
    qs = [plan_query("box4"), plan_query("box16")]
    lone = []
    for q in qs:
        e = fresh()
        grow(e, q)
        sc = e.plan_shortcut()
        fin = e.plan_finish()
        lone.append((sc, fin, e.plan_fetch(fin)))
        e.close()
    es = [fresh(), fresh()]
    try:
        for e, q in zip(es, qs):
            install(e, q)
        st = _lib.plan_begin_many(es, [_lib.plan_cfg(START, q["goal"], q["mode"], q["mass"], EXEC,
                                                     SAMPLES + 1, BATCH, q["seed"]) for q in qs])
        assert st == [_lib.PLAN_OK] * 2
        _lib.plan_run_fused(es, SAMPLES, BATCH)
        scs = [e.plan_shortcut() for e in es]
        fins = _lib.plan_finish_many(es)
        for e, sc, fin, (sc0, fin0, out0) in zip(es, scs, fins, lone):
            assert sc0.chords_used >= 1
            a, b = sc.as_dict(), sc0.as_dict()
            a.pop("ms"), b.pop("ms")
            assert a == b
            out = e.plan_fetch(fin)
            for k in ("waypoints", "q", "qd", "qdd", "psg", "tau"):
                assert out[k].tobytes() == out0[k].tobytes(), k
            assert (fin.status, fin.n_waypoints, fin.n_traj, fin.first_fail, fin.goal_node,
                    fin.edge_steps, fin.n_nodes) == \
                (fin0.status, fin0.n_waypoints, fin0.n_traj, fin0.first_fail, fin0.goal_node,
                 fin0.edge_steps, fin0.n_nodes)
    finally:
        for e in es:
            e.close()


# ---- drop-in ---------------------------------------------------------------------------------
def _golden_fns(z, foreign_dynam=False):
    from torque_constrained_motion_planning_amd import panda_primitives as PP
    from torque_constrained_motion_planning_amd import utils as U
    mode, mass = int(z["mode"]), float(z["mass"])
    prob = U.Problem(U.PandaRobot(), list(z["obs"]), U.Payload(mass), mass, float(z["exec_time"]),
                     torque_test={0: "base", 1: "nov", 2: "rne"}[mode])
    resolutions = 0.2 ** np.ones(7)
    radius = resolutions / 2
    joints = U.get_arm_joints(prob.robot)
    dyn = PP.get_dynamics_fn_v5(prob, resolutions)
    if foreign_dynam:
        dyn = (lambda f: (lambda path, n: f(path, n)))(dyn)
    return dict(distance=U.get_distance_fn(prob.robot, joints, weights=np.reciprocal(radius)),
                sample=U.get_sample_fn(prob.robot, joints),
                extend=U.get_extend_fn(prob.robot, joints, resolutions=radius),
                collision=U.get_collision_fn(prob.robot, joints, list(z["obs"]),
                                             self_collisions=False),
                torque_fn=PP.select_torque_test(prob), dynam_fn=dyn)


@pytest.mark.parametrize("foreign_dynam", [False, True])
def test_drop_in_shortcut(foreign_dynam):
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_force_aware
    z = np.load(os.path.join(GOLDEN, "rrt_box4_nov2.npz"))
    f = _golden_fns(z, foreign_dynam)
    args = (tuple(z["start"]), tuple(z["goal"]), f["distance"], f["sample"], f["extend"],
            f["collision"], f["torque_fn"], f["dynam_fn"])
    kw = dict(radius=[0.01], max_time=50, max_iterations=int(z["iters"]))
    e = f["collision"].engine
    wps = []
    for shortcut in (False, True):
        random.seed(int(z["seed"]))
        np.random.seed(int(z["seed"]))
        path, vels, accels, psg = rrt_star_force_aware(*args, shortcut=shortcut, **kw)
        assert path is not None or shortcut
        wps.append(e.plan_fetch(e.plan_retrace())["waypoints"])
    plain, short = wps
    assert np.abs(plain - z["waypoints"]).max() < 1e-12
    c = dict(obs=np.asarray(z["obs"], dtype=np.float64).reshape(-1, 15), mode=int(z["mode"]),
             mass=float(z["mass"]))
    ref, st = reference(c, W=plain, a_max=512, passes=1)
    assert st["chords_used"] >= 1
    assert short.tobytes() == ref.tobytes()
    assert short[0].tobytes() == plain[0].tobytes() and short[-1].tobytes() == plain[-1].tobytes()
    assert SR.path_cost(short) <= SR.path_cost(plain)


def test_drop_in_shortcut_needs_native_callbacks():
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_force_aware
    z = np.load(os.path.join(GOLDEN, "rrt_box4_nov2.npz"))
    f = _golden_fns(z)
    dist = (lambda fn: (lambda a, b: fn(a, b)))(f["distance"])
    with pytest.raises(NotImplementedError, match="distance, extend, collision and torque"):
        rrt_star_force_aware(tuple(z["start"]), tuple(z["goal"]), dist, f["sample"], f["extend"],
                             f["collision"], f["torque_fn"], f["dynam_fn"], radius=[0.01],
                             max_time=50, max_iterations=int(z["iters"]), shortcut=True)


def test_batched_shortcut_record():
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_batched
    q = plan_query("box4")
    e = fresh()
    try:
        res, r, raw = rrt_star_batched(START, q["goal"], q["obs"], q["mode"], q["mass"], EXEC,
                                       SAMPLES, batch=BATCH, seed=q["seed"], engine=e,
                                       shortcut=True)
        sc = raw["shortcut"]
        assert isinstance(sc, _lib.ShortcutResult) and sc.status == 0
        assert sc.n_after == r.n_waypoints == len(raw["waypoints"]) and sc.chords_used >= 1
        _, r0, raw0 = rrt_star_batched(START, q["goal"], q["obs"], q["mode"], q["mass"], EXEC,
                                       SAMPLES, batch=BATCH, seed=q["seed"], engine=e)
        assert "shortcut" not in raw0 and r0.n_waypoints == sc.n_before
    finally:
        e.close()
