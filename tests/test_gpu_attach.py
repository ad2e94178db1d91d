"""GPU: bodies held by the gripper (tcmp_set_attachments) against the restatement
tests/attach_ref.py -- frames and depth of tests/collision_ref.py (numpy and qhull), the oracle's
walk for the arm and torque part of an edge -- on the cases of tests/attach_cases.py.

Depths (tcmp_attached_pd) are held to 1e-9 wherever either side says >= 0.03; flags, edges, the
trees of whole plans, the two planner loops, the round graphs and the refusals are exact."""
import os
import random

import numpy as np
import pytest

import attach_cases as K
import attach_ref as A
from conftest import GOLDEN, engine_with_split

pytestmark = pytest.mark.gpu

TOL64 = 1e-9
P = K.P
START = np.array([0, -np.pi / 4, 0.0, -6 * np.pi / 8, 0, np.pi / 2, np.pi / 4])
EMPTY = np.zeros((0, 15))
W = np.full(7, 10.0)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes()


def attach(eng, held):
    eng.set_attachments(*K.engine_args(held))


@pytest.fixture(scope="module")
def eng():
    from torque_constrained_motion_planning_amd import _lib
    e = _lib.Engine(0)
    yield e
    e.close()


# ---- 1. depths ---------------------------------------------------------------------------------
def test_depths(eng):
    k = K.depth_case()
    eng.set_scene(K.boxes(), K.mesh_pack())
    attach(eng, k.held)
    try:
        got = eng.attached_pd(k.q)
    finally:
        eng.set_attachments()
    assert got.shape == k.ref.shape == (200, 2, 19) and not np.isnan(got).any()
    m = (k.ref >= 0.03) | (got >= 0.03)
    err = np.abs(got[m] - k.ref[m])
    for name, sl in (("boxes", slice(0, 16)), ("meshes", slice(16, 19))):
        mm = m[:, :, sl]
        e = np.abs(got[:, :, sl][mm] - k.ref[:, :, sl][mm])
        print("attached_pd, %s: %d pairs at or above 0.03, max |device - reference| %.3g"
              % (name, mm.sum(), e.max()))
    assert m.sum() >= 30
    assert (err <= TOL64).all(), err.max()
    # a pair the reference's pre-test proves under 0.03 is under 0.03 on the device
    assert (got[~m] < 0.03).all()


# ---- 2. flags ----------------------------------------------------------------------------------
def test_flags(eng):
    k = K.flag_case()
    eng.set_scene(k.boxes)
    attach(eng, k.held)
    try:
        got = eng.collides(k.q)
    finally:
        eng.set_attachments()
    arm_only = eng.collides(k.q)
    use = ~k.near
    want = k.arm | k.held_hit
    bad = np.flatnonzero((got != want) & use)
    print("flags: %d cases, %d left out, %d held-only hits, %d wrong"
          % (len(want), (~use).sum(), (k.held_hit & ~k.arm & use).sum(), len(bad)))
    assert len(bad) == 0, (bad[:10], k.dmax[bad][:10])
    # without the attachment the same call is the arm's flag alone
    assert np.array_equal(arm_only, k.arm)


def test_small_body_flags_and_edges(eng):
    """A held body whose bounding ball is smaller than the threshold (Payload.coke's prism): the
    ball certificate must leave a centre inside an obstacle's box to the exact test."""
    from torque_constrained_motion_planning_amd.scene import Payload
    r = K.record()
    held = (K.small_body(),)
    assert np.allclose(held[0].verts, Payload.coke(1.0).collision_vertices())
    eng.set_scene(K.boxes())
    attach(eng, held)
    try:
        got = eng.collides(r["small_q"])
        ns, nt, last = eng.check_edges(r["small_a"], r["small_b"], K.MODE_RNE, K.MASS)
    finally:
        eng.set_attachments()
    d, arm = r["small_dmax"], r["small_arm"].astype(bool)
    want = arm | (d >= P)
    bad = np.flatnonzero(got != want)
    print("small body: %d flags, %d held hits, %d held only, %d wrong; %d edges, %d shortened"
          % (len(want), (d >= P).sum(), ((d >= P) & ~arm).sum(), len(bad), len(ns),
             (r["small_n_safe"] < r["small_arm_safe"]).sum()))
    assert len(bad) == 0, (bad[:10], d[bad][:10])
    assert np.array_equal(ns, r["small_n_safe"]) and np.array_equal(nt, r["small_n_steps"])
    assert bits(last) == bits(r["small_last"])


# ---- 3. edges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [None, 1, 2])
def test_edges(split):
    k = K.edge_case()
    e = engine_with_split(split)
    try:
        for s in k.sets:
            e.set_scene(k.boxes, K.mesh_pack() if s["with_mesh"] else None)
            attach(e, k.held)
            ns, nt, last = e.check_edges(s["a"], s["b"], K.MODE_RNE, K.MASS)
            e.set_attachments()
            arm_ns, arm_nt, _ = e.check_edges(s["a"], s["b"], K.MODE_RNE, K.MASS)
            bad = np.flatnonzero((ns != s["n_safe"]) | (nt != s["n_steps"]))
            assert len(bad) == 0, (split, s["with_mesh"], bad[:10], ns[bad][:10], s["n_safe"][bad][:10])
            assert bits(last) == bits(s["last"]), (split, s["with_mesh"])
            assert np.array_equal(arm_ns, s["arm_safe"]) and np.array_equal(arm_nt, s["n_steps"])
    finally:
        e.close()


# ---- 4. rounds ---------------------------------------------------------------------------------
def _dist(a, b):
    s = 0.0
    for k in range(7):
        d = b[k] - a[k]
        s += W[k] * (d * d)
    return np.sqrt(s)


def _plan(e, radius, run=None, seed=3, n=2048, batch=64):
    from torque_constrained_motion_planning_amd import _lib
    z = np.load(os.path.join(GOLDEN, "rrt_box16_rne5.npz"))
    st = e.plan_begin(z["start"], z["goal"], K.MODE_RNE, K.MASS, 5.0, max_nodes=n + 2,
                      max_batch=batch, seed=seed, radius=radius)
    assert st == _lib.PLAN_OK
    if run is None:
        return z
    if run == "graph":
        e.plan_run(n, batch)
    else:
        for _ in range(n // batch):
            e.plan_round(nb=batch, sync=False)
    return z


@pytest.mark.parametrize("radius", [0.01, 4.0])
def test_rounds(eng, radius):
    from torque_constrained_motion_planning_amd import _lib
    held = (K.tool_box(),)
    boxes = K.boxes()
    obs = A.obstacle_vertices(boxes)
    eng.set_scene(boxes)
    attach(eng, held)
    other = _lib.Engine(0)
    try:
        other.set_scene(boxes)
        attach(other, held)
        _plan(eng, radius)
        rounds = []
        for _ in range(32):
            eng.plan_round(nb=64, sync=False)
            cand, nn, _, snap = eng.plan_debug_round(64)
            rounds.append((cand, nn, snap, eng.plan_digest()[1]))
        cfg, cost, par, n_nodes = eng.plan_tree(2100)
        tgt, meta = eng.plan_tree_edges(2100)
        stats = eng.attach_stats()
        r = eng.plan_finish()
        # n_nodes is the sum of the accepted lanes: each round's edges once more through
        # tcmp_check_edges on another engine (a stale accepted count would leave holes)
        total, counted = 1, 0
        for cand, nn, snap, after in rounds:
            assert snap == total
            ns, nt, _ = other.check_edges(cfg[nn], cand, K.MODE_RNE, K.MASS)
            total += int((ns > 0).sum())
            counted += int(np.where(ns < nt, ns + 1, nt).sum())
            assert after == total
        assert n_nodes == total == len(cfg) and n_nodes > 200
        # the counted extend steps are the combined sequential walk's (n_safe' + 1 on a failure,
        # else n_steps) over the rounds' edges, plus the rewire walks' own
        assert r.edge_steps - r.rewire_steps == counted, (r.edge_steps, r.rewire_steps, counted)
        assert stats["shortened"] + stats["removed"] > 0 and stats["edges"] >= total - 1
    finally:
        eng.set_attachments()
        other.close()
    rewired = 0
    for i in range(1, n_nodes):
        p = par[i]
        assert 0 <= p < i
        n_steps, j, last = A.edge(cfg[p], tgt[i], held, boxes, obs, K.MODE_RNE, K.MASS)
        # every step of the node's edge passes the combined test and the next one fails it
        # (maximality): the restatement's combined walk ends exactly where the node's edge does
        assert (n_steps, j) == tuple(meta[i]) and j >= 1, (i, n_steps, j, meta[i])
        if bits(last) != bits(cfg[i]):
            # a rewired node keeps its configuration; its new edge was walked toward it and
            # accepted within the rewire's own 1e-6 (rrt_star.py:192)
            rewired += 1
            assert bits(tgt[i]) == bits(cfg[i]) and j == n_steps
            assert _dist(cfg[i], last) < 1e-6
        assert cost[i] == cost[p] + _dist(cfg[p], cfg[i]), i
    print("radius %g: %d nodes, %d rewires, %d nodes off their regenerated edge's bits"
          % (radius, n_nodes, r.n_rewires, rewired))
    assert rewired <= r.n_rewires
    if radius > 1:
        assert r.n_rewires > 0


# ---- 5. the two loops --------------------------------------------------------------------------
LOOP_SEED = 5  # chosen on the GPU among seeds 0..7: the attachment changes this seed's path


def _loop_args(attachments):
    from torque_constrained_motion_planning_amd import panda_primitives as PP
    from torque_constrained_motion_planning_amd import utils as U
    z = np.load(os.path.join(GOLDEN, "rrt_box16_rne5.npz"))
    mass = float(z["mass"])
    prob = U.Problem(U.PandaRobot(), list(z["obs"]), U.Payload(mass), mass, float(z["exec_time"]),
                     torque_test="rne")
    resolutions = 0.2 ** np.ones(7)
    radius = resolutions / 2
    joints = U.get_arm_joints(prob.robot)
    collision = U.get_collision_fn(prob.robot, joints, list(z["obs"]), attachments=attachments,
                                   self_collisions=False)
    return [tuple(z["start"]), tuple(z["goal"]),
            U.get_distance_fn(prob.robot, joints, weights=np.reciprocal(radius)),
            U.get_sample_fn(prob.robot, joints),
            U.get_extend_fn(prob.robot, joints, resolutions=radius), collision,
            PP.select_torque_test(prob), PP.get_dynamics_fn_v5(prob, resolutions)]


def _loop(args, host):
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_force_aware
    a = list(args)
    if host:
        fn = a[5]
        a[5] = lambda q, **kw: fn(q)  # a foreign callback: the host loop, one call per step
    random.seed(LOOP_SEED)
    np.random.seed(LOOP_SEED)
    return rrt_star_force_aware(*a, radius=[4.0], max_time=50, max_iterations=60)


def test_loops_agree():
    """The engine loop (k_att_edges, the ATT rewire) and the host loop (k_att_configs per
    configuration) return the same rows; the same query without the attachment another path."""
    from torque_constrained_motion_planning_amd.scene import Payload
    from torque_constrained_motion_planning_amd.utils import PANDA_TOOL_FRAME, Attachment
    body = Payload(K.MASS, size=A.TOOL_BOX)
    att = Attachment(None, PANDA_TOOL_FRAME, np.eye(4), body)
    with_att = _loop_args([att])
    without = _loop_args([])
    try:
        dev = _loop(with_att, False)
        host = _loop(with_att, True)
        plain = _loop(without, False)
    finally:
        for f in (with_att[5], without[5]):
            f.engine.close()
    assert dev[0] is not None and host[0] is not None and plain[0] is not None
    for x, y in zip(dev, host):
        assert bits(x) == bits(y)
    assert bits(dev[0]) != bits(plain[0])


# ---- 6. graphs ---------------------------------------------------------------------------------
KEEP = "keep"  # _digest: leave the engine's attachments as they are (a set bumps the generation)


def _digest(e, held, run, radius=4.0):
    if held is None:
        e.set_attachments()
    elif held is not KEEP:
        attach(e, held)
    _plan(e, radius, run=run, n=1024)
    d = e.plan_digest()
    r = e.plan_finish()
    return d, r


def test_graphs():
    from torque_constrained_motion_planning_amd import _lib
    held, shorter = (K.tool_box(),), (K.tool_box((0.08, 0.08, 0.12)),)
    e, fresh = _lib.Engine(0), _lib.Engine(0)
    try:
        for x in (e, fresh):
            x.set_scene(K.boxes())
        loop, _ = _digest(fresh, held, "rounds")
        c0 = e.attach_stats()["graph_captures"]
        d1, r1 = _digest(e, held, "graph")
        c1 = e.attach_stats()["graph_captures"]
        d2, r2 = _digest(e, KEEP, "graph")
        c2 = e.attach_stats()["graph_captures"]
        assert r1.graph_launches >= 1 and r2.graph_launches >= 1
        assert c1 > c0 and c2 == c1  # the first run captured, the second replayed that graph
        # setting the same attachment again bumps the generation: captured anew, the same tree
        d2b, _ = _digest(e, held, "graph")
        c2 = e.attach_stats()["graph_captures"]
        assert d2b == loop and c2 > c1
        assert d1 == loop and d2 == loop
        plain, _ = _digest(fresh, None, "rounds")
        loop_short, _ = _digest(fresh, shorter, "rounds")
        assert len({loop, plain, loop_short}) == 3  # the attachment, and its length, matter here
        # the same shape with another attachment (a shorter box): not the stale graph's result
        d3, r3 = _digest(e, shorter, "graph")
        assert d3 == loop_short and e.attach_stats()["graph_captures"] > c2  # captured anew
        d4, _ = _digest(e, None, "graph")
        assert d4 == plain
    finally:
        e.close()
        fresh.close()


# ---- 7. nothing set, nothing changed -----------------------------------------------------------
def test_nothing_set_nothing_changed():
    from torque_constrained_motion_planning_amd import _lib
    never, cleared = _lib.Engine(0), _lib.Engine(0)
    try:
        for radius in (0.01, 4.0):
            for run in ("rounds", "graph"):
                never.set_scene(K.boxes())
                cleared.set_scene(K.boxes())
                attach(cleared, (K.tool_box(),))
                a, _ = _digest(never, None, run, radius)
                b, _ = _digest(cleared, None, run, radius)  # set_attachments(n = 0) first
                assert a == b, (radius, run)
        # no obstacle: the held body cannot matter
        for x in (never, cleared):
            x.set_scene(EMPTY)
        a, _ = _digest(never, None, "rounds")
        b, _ = _digest(cleared, (K.tool_box(),), "rounds")
        assert a == b
    finally:
        never.close()
        cleared.close()


# ---- 8. refusals -------------------------------------------------------------------------------
def test_refusals(eng):
    from torque_constrained_motion_planning_amd import _lib
    z = np.load(os.path.join(GOLDEN, "rrt_box16_rne5.npz"))
    eng.set_scene(K.boxes())
    held = (K.tool_box(),)
    cfg = _lib.plan_cfg(z["start"], z["goal"], K.MODE_RNE, K.MASS, 5.0, 130, 64, seed=1)
    wp = np.stack([z["start"], z["goal"]])
    pose = eng.fk(z["goal"][None])

    def calls():
        yield "tcmp_plan_begin_many", lambda: _lib.plan_begin_many([eng], [cfg])
        yield "tcmp_repair_traj", lambda: eng.repair_traj(wp, 10, check_only=True)
        yield "tcmp_goal_search", lambda: eng.goal_search(pose, [0.0], z["start"], K.MODE_RNE, K.MASS)

    def plan_calls():
        yield "tcmp_plan_run_fused", lambda: _lib.plan_run_fused([eng], 64, 64)
        yield "tcmp_plan_run_group", lambda: _lib.plan_run_group([eng], 64, 64)
        yield "tcmp_plan_run_shared", lambda: eng.plan_run_shared(None, 64, 64)
        yield "tcmp_plan_repair", lambda: eng.plan_repair(check_only=True)
    attach(eng, held)
    try:
        for name, call in calls():
            with pytest.raises(_lib.TcmpError, match="%s.*attachment" % name):
                call()
        _plan(eng, 0.01, n=128)
        with pytest.raises(_lib.TcmpError, match="plan is open"):
            eng.set_attachments()
        for name, call in plan_calls():
            with pytest.raises(_lib.TcmpError, match="%s.*attachment" % name):
                call()
        assert eng.plan_digest()[1] == 1  # nothing ran
        eng.plan_run(128, 64)
        eng.plan_finish()
    finally:
        eng.synchronize()
    # cleared (the finish above ended the plan): every one of them works again
    eng.set_attachments()
    for name, call in calls():
        call()
    eng.plan_finish()  # (tcmp_plan_begin_many opened a plan)
    _plan(eng, 0.01, n=128)
    _lib.plan_run_fused([eng], 64, 64)
    _lib.plan_run_group([eng], 64, 64)
    with pytest.raises(_lib.TcmpError, match="null comm"):  # past the refusal: its own check
        eng.plan_run_shared(None, 64, 64)
    eng.plan_repair(check_only=True)
    eng.plan_finish()
    # the lock ends with any finish: begin_many / finish_many leave the set free to change
    assert _lib.plan_begin_many([eng], [cfg]) == [_lib.PLAN_OK]
    with pytest.raises(_lib.TcmpError, match="plan is open"):
        attach(eng, held)
    _lib.plan_finish_many([eng])
    attach(eng, held)
    eng.set_attachments()


def test_scene_and_attachments_must_fit():
    """The setters refuse a scene and a set whose LDS would not fit the rewiring's block, and
    change nothing; what they accept plans through its rounds, the rewiring included."""
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd.hull import hull_data
    rng = np.random.default_rng(3)
    far = np.concatenate([rng.uniform(5.0, 9.0, (300, 3)), np.tile(np.eye(3).ravel(), (300, 1)),
                          np.full((300, 3), 0.05)], axis=1)
    big = rng.normal(size=(64, 3))
    big = hull_data(0.05 * big / np.linalg.norm(big, axis=1)[:, None])
    one, four = K.engine_args((K.tool_box(),)), ([big] * 4, [7, 7, 6, 6], [np.eye(4)] * 4)
    e = _lib.Engine(0)
    try:
        e.set_scene(far[:200])
        e.set_attachments(*one)           # about 210 boxes fit with one small hull
        with pytest.raises(_lib.TcmpError, match="do not fit"):
            e.set_scene(far[:260])
        with pytest.raises(_lib.TcmpError, match="do not fit"):
            e.set_attachments(*four)      # four 64-vertex hulls: about 88
        assert e.attached_pd(START[None]).shape == (1, 1, 200)  # neither call changed anything
        _plan(e, 4.0, run="rounds", n=256)
        assert e.plan_finish().n_nodes > 1
        e.set_attachments()
        e.set_scene(far[:260])
        with pytest.raises(_lib.TcmpError, match="do not fit"):
            e.set_attachments(*one)
        e.set_scene(far[:80])
        e.set_attachments(*four)
        _plan(e, 4.0, run="rounds", n=256)
        assert e.plan_finish().n_nodes > 1
    finally:
        e.close()


def test_bad_attachments(eng):
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd.hull import hull_data
    eng.set_attachments()
    v, pl, ed = hull_data(A.box_body(A.TOOL_BOX))
    ok = np.eye(4)

    def bad(hull, link, T, what):
        with pytest.raises(_lib.TcmpError, match=what):
            eng.set_attachments([hull], [link], [T])
    bad((v, pl, ed), 10, ok, "parent_link")
    bad((v, pl, ed), -1, ok, "parent_link")
    S = ok.copy()
    S[0, 0] = 1.001
    bad((v, pl, ed), 7, S, "rotation")
    M = ok.copy()
    M[2, 2] = -1.0
    bad((v, pl, ed), 7, M, "reflection")
    p2 = pl.copy()
    p2[0, :3] *= 1.01
    bad((v, p2, ed), 7, ok, "unit normal")
    p3 = pl.copy()
    p3[0, 3] -= 0.01
    bad((v, p3, ed), 7, ok, "outside plane")
    e2 = ed.copy()
    e2[0, 1] = 8
    bad((v, pl, e2), 7, ok, "edge index")
    rng = np.random.default_rng(0)
    big = rng.normal(size=(65, 3))
    big /= np.linalg.norm(big, axis=1)[:, None]
    bad(hull_data(0.1 * big), 7, ok, "too large")
    with pytest.raises(_lib.TcmpError, match="count"):
        eng.set_attachments([(v, pl, ed)] * 5, [7] * 5, [ok] * 5)
    with pytest.raises(_lib.TcmpError, match="no attachments"):
        eng.attached_pd(START[None])
    # 64 vertices and 4 bodies are accepted
    eng.set_attachments([hull_data(0.1 * big[:64])] + [(v, pl, ed)] * 3, [7, 6, 0, 9], [ok] * 4)
    eng.set_scene(K.boxes())
    assert eng.attached_pd(START[None]).shape == (1, 4, 16)
    eng.set_attachments()
