"""GPU: best-parent goal connection over the whole tree (tcmp_connect_nodes, tcmp_plan_connect;
csrc/tcmp_connect.h) against the restatement in tests/connect_ref.py, whose edge checks are the
CPU oracle's check_edge (resolutions 0.1, weights 10: the planner's defaults, used throughout).

The selected ids and keys bit for bit; every count equal; verdicts and the winner's last point bit
for bit (the oracle's extend is the device's, as tests/test_gpu_shortcut.py relies on); costs
within 1e-12 relative (the project's tolerance for tree costs).
"""
import ctypes
import math
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, engine_with_split

import oracle as O  # noqa: E402  (test infrastructure)
import connect_ref as CR
import shortcut_ref as SR

pytestmark = pytest.mark.gpu

LO, HI, START = CR.LO, CR.HI, CR.START
NO_OBS = np.zeros((0, 15))
BASE = 0


def close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(b), 1e-300)


@pytest.fixture(scope="module")
def eng():
    from torque_constrained_motion_planning_amd import _lib
    e = _lib.Engine(0)
    e.set_timing(False)
    yield e
    e.close()


# ---- 1. selection alone ----------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 70001)
KS = (1, 2, 64, 1000, 65536)
PASSES = (1, 8)
KINDS = ("random", "tiled5", "equal", "bound_all_out", "bound_one_in", "bound_at_key",
         "more_than_eligible")


def selection_input(kind, T, rng):
    """-> (nodes, cost, goal, bound).  Nodes inside the joint limits, so every straight edge to
    the goal stays inside them: in the empty scene without a torque test every edge is valid."""
    G = LO + (HI - LO) * rng.random(7)
    if kind == "tiled5":
        # the threshold falls inside a tie group that spans blocks: index order decides
        five = LO + (HI - LO) * rng.random((5, 7))
        c5 = rng.random(5) * 3
        q, g = five[np.arange(T) % 5], c5[np.arange(T) % 5]
    elif kind == "equal":
        q, g = np.tile(LO + (HI - LO) * rng.random(7), (T, 1)), np.full(T, 1.25)
    else:
        q, g = LO + (HI - LO) * rng.random((T, 7)), rng.random(T) * 5
    key = np.sort(CR.keys(q, g, G))
    bound = {"bound_all_out": key[0],                 # strict: the smallest key is out too
             "bound_one_in": key[min(1, T - 1)],      # (T = 1: none)
             "bound_at_key": key[T // 2],             # that key and its equals are out
             }.get(kind, math.inf)
    return np.ascontiguousarray(q), np.ascontiguousarray(g), G, float(bound)


@pytest.mark.parametrize("kind", KINDS)
def test_selection_vs_restatement(eng, kind):
    from torque_constrained_motion_planning_amd import _lib
    eng.set_scene(NO_OBS)
    rng = np.random.default_rng(KINDS.index(kind) + 1)
    seen = set()
    for T in SIZES:
        q, g, G, bound = selection_input(kind, T, rng)
        key = CR.keys(q, g, G)
        grid = [(K, p) for K in KS for p in PASSES]
        if kind == "more_than_eligible":
            grid = [(K, p) for K, p in grid if K * p > T] or [(65536, 8)]
        for K, p in grid:
            ids, n_el = CR.select(key, bound, K, p)
            o = eng.connect_nodes(q, g, G, BASE, 0.0, bound=bound, max_candidates=K, passes=p)
            r = o["result"]
            M = len(ids)
            assert (r.n_nodes, r.n_eligible, r.n_selected) == (T, n_el, M), (T, K, p)
            assert o["ids"].tobytes() == ids.astype(np.int32).tobytes(), (T, K, p)
            assert o["keys"].tobytes() == key[ids].tobytes(), (T, K, p)
            if M == 0:
                assert (r.status, r.passes_run, r.n_tested, r.key_min) == (_lib.CONNECT_NONE, 0, 0, 0.0)
                assert (r.parent, r.rank, r.cost_after) == (-1, -1, 0.0) and o["node"] is None
                seen.add("none")
                continue
            # every edge is valid, so the first pass ends the stage and rank 0 wins it
            n0 = min(K, M)
            assert (r.status, r.passes_run, r.n_tested, r.n_valid) == (_lib.CONNECT_OK, 1, n0, n0)
            assert (r.rank, r.parent) == (0, ids[0]) and r.key_min == key[ids[0]]
            assert (o["nsafe"][:n0] > 0).all() and (o["nsafe"][:n0] == o["nsteps"][:n0]).all()
            assert (o["nsafe"][n0:] == -1).all() and (o["nsteps"][n0:] == -1).all()
            last, c = o["node"][:7], o["node"][7]
            assert CR.distance(last, G) < 1e-2 and c == r.cost_after
            assert close(c, g[ids[0]] + CR.distance(q[ids[0]], last)) and c < bound
            seen.add("stopped" if n0 < M else "whole")
    # (with K < T < K * passes every eligible node is selected and the first pass still stops)
    want = {"bound_all_out": {"none"}, "bound_one_in": {"none", "whole"}}.get(kind)
    assert seen == want if want else {"stopped", "whole"} <= seen, (kind, seen)


def test_selection_is_deterministic_and_checks_arguments(eng):
    from torque_constrained_motion_planning_amd import _lib
    eng.set_scene(NO_OBS)
    rng = np.random.default_rng(9)
    q, g, G, _ = selection_input("tiled5", 4097, rng)
    a = eng.connect_nodes(q, g, G, BASE, 0.0, max_candidates=1000, passes=2)
    b = eng.connect_nodes(q, g, G, BASE, 0.0, max_candidates=1000, passes=2)
    for k in ("ids", "keys", "nsafe", "nsteps", "node"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["result"].as_dict() == b["result"].as_dict()  # (timing is off: ms is 0)
    # an output too small: -4 with n_selected set
    r = _lib.ConnectResult()
    cfg = _lib.ConnectCfg(1000, 2)
    ids = np.zeros(10, dtype=np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    call = lambda n, cfg, cap: eng.L.tcmp_connect_nodes(  # noqa: E731
        eng.h, _lib._d(q), _lib._d(g), n, _lib._d(G), math.inf, None, None, 1e-2, BASE, 0.0,
        ctypes.byref(cfg), ids.ctypes.data_as(i32p), None, None, None, cap, None, ctypes.byref(r))
    assert call(len(q), cfg, 10) == -4 and r.n_selected == 2000
    # every output pointer may be null
    assert eng.L.tcmp_connect_nodes(eng.h, _lib._d(q), _lib._d(g), len(q), _lib._d(G), math.inf,
                                    None, None, 1e-2, BASE, 0.0, ctypes.byref(cfg), None, None,
                                    None, None, 0, None, ctypes.byref(r)) == 0
    assert (r.status, r.rank, r.n_selected) == (0, 0, 2000)
    assert call(0, cfg, 10) == -1 and eng.L.tcmp_last_error()
    for K, p in ((-1, 1), (65537, 1), (64, 9), (64, -1)):
        assert call(len(q), _lib.ConnectCfg(K, p), 10) == -1, (K, p)
    with pytest.raises(_lib.TcmpError, match="error -1"):
        eng.connect_nodes(q, -g - 1.0, G, BASE, 0.0)


# ---- 2. verdicts -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdict_case():
    q = CR.query(O, 16, 2)
    rng = np.random.default_rng(1)
    W = SR.zigzag(O, rng, 300, q["obs"], CR.MODE, CR.MASS, LO, HI)
    hop = [SR.dist(W[t], W[t + 1]) for t in range(len(W) - 1)]
    cost = np.concatenate([[0.0], np.cumsum(hop)]) * 0.05
    refs = {(K, p): CR.connect(W, cost, q["goal"], CR.oracle_check(O, q["obs"], CR.MODE, CR.MASS),
                               K=K, passes=p) for K, p in ((64, 4), (32, 8), (300, 1))}
    return q, W, cost, refs


def same_verdicts(o, ref):
    r, rr = o["result"].as_dict(), ref["result"]
    print({k: (r[k], rr[k]) for k in rr})
    for k in rr:
        if k not in ("cost_after", "cost_before", "key_min"):
            assert r[k] == rr[k], (k, r[k], rr[k])
    assert r["key_min"] == rr["key_min"] and r["cost_before"] == rr["cost_before"]
    assert close(r["cost_after"], rr["cost_after"])
    assert o["ids"].tobytes() == ref["ids"].tobytes()
    assert o["keys"].tobytes() == ref["keys"].tobytes()
    assert o["nsafe"].tobytes() == ref["nsafe"].tobytes()
    assert o["nsteps"].tobytes() == ref["nsteps"].tobytes()
    if rr["status"] == CR.OK:
        assert o["node"][:7].tobytes() == ref["node"][:7].tobytes()
        assert close(o["node"][7], ref["node"][7])
    else:
        assert o["node"] is None


def run_verdicts(e, case):
    q, W, cost, refs = case
    e.set_scene(q["obs"])
    for (K, p), ref in refs.items():
        o = e.connect_nodes(W, cost, q["goal"], CR.MODE, CR.MASS, max_candidates=K, passes=p)
        same_verdicts(o, ref)


def test_verdicts_vs_restatement(eng, verdict_case):
    refs = verdict_case[3]
    r = refs[(32, 8)]["result"]
    # a later pass wins, valid and invalid edges both occur, and ranks stay untested
    assert r["status"] == CR.OK and r["passes_run"] >= 2 and r["n_tested"] < r["n_selected"], \
        (r, "the fixture proves nothing")
    assert 0 < r["n_valid"] < r["n_tested"] and (refs[(32, 8)]["nsafe"] == -1).any()
    assert refs[(300, 1)]["result"]["n_tested"] == 300
    run_verdicts(eng, verdict_case)


@pytest.mark.parametrize("split", [1, 2])
def test_verdicts_edge_kernel_variants(split, verdict_case):
    """The candidates' edges through k_edges<., 1> and k_edges<., 2> (the default engine takes 4
    lanes per edge at these sizes)."""
    e = engine_with_split(split)
    try:
        run_verdicts(e, verdict_case)
    finally:
        e.close()


# ---- 3. the plan form on the five fixtures ---------------------------------------------------
def fresh(timing=False):
    from torque_constrained_motion_planning_amd import _lib
    e = _lib.Engine(0)
    e.set_timing(timing)  # off: every ms is 0, so whole results compare equal
    return e


def begin(e, q, max_nodes, batch=CR.BATCH):
    from torque_constrained_motion_planning_amd import _lib
    e.set_scene(q["obs"])
    e.set_self_collision(False)
    assert e.plan_begin(START, q["goal"], q["mode"], q["mass"], CR.EXEC, max_nodes=max_nodes,
                        max_batch=batch, seed=q["seed"]) == _lib.PLAN_OK


def grow(e, q, extra=1, samples=CR.SAMPLES, batch=CR.BATCH):
    begin(e, q, samples + 1 + extra, batch)
    e.plan_run(samples, batch)


def tree_of(e, cap=CR.SAMPLES + CR.BATCH + 8):
    cfg, cost, par, n = e.plan_tree(cap)
    assert n == len(cfg)
    return cfg.copy(), cost.copy(), par.copy()


def restate(e, q, K, passes, max_nodes):
    cfg, cost, par = tree_of(e)
    ref = CR.connect(cfg, cost, q["goal"], CR.oracle_check(O, q["obs"], q["mode"], q["mass"]),
                     K=K, passes=passes, goal_node=e.plan_goal()[0], max_nodes=max_nodes)
    return (cfg, cost, par), ref


def same_record(r, rr):
    r = r.as_dict()
    print({k: (r[k], rr[k]) for k in rr})
    for k in rr:
        if k != "cost_after":
            assert r[k] == rr[k], (k, r[k], rr[k])
    assert close(r["cost_after"], rr["cost_after"]) or r["cost_after"] == rr["cost_after"]


def check_path(q, e, tree, ref, fin, out):
    """The finished plan of a connected tree: the waypoints run through the winner's ancestors
    in order and end in the connecting edge's own points, their summed length is the new goal
    cost, and the trajectory is oracle.minjerk of them with its validation's verdict."""
    from torque_constrained_motion_planning_amd import _lib
    cfg, cost, par = tree
    wp = out["waypoints"]
    W = len(wp)
    assert fin.n_waypoints == W and wp[0].tobytes() == START.tobytes()
    i = ref["result"]["parent"]
    nt, ns = ref["meta"]
    # (the retrace regenerates the edge's first n_safe - 1 points and ends in the node itself)
    tail = np.array(SR.extend_points(cfg[i], q["goal"], nt)[:ns - 1] + [ref["node"][:7]])
    assert wp[W - ns:].tobytes() == tail.tobytes() and wp[W - ns - 1].tobytes() == cfg[i].tobytes()
    assert wp[-1].tobytes() == ref["node"][:7].tobytes()
    at = 0
    for a in CR.ancestors(par, i):
        while wp[at].tobytes() != cfg[a].tobytes():
            at += 1
            assert at < W - ns, ("ancestor %d is not on the path" % a)
    assert at == W - ns - 1
    assert abs(SR.path_cost(wp) - ref["node"][7]) <= 1e-9 * ref["node"][7]
    ni = int(CR.EXEC * 1000 / W)
    assert ni > 0 and fin.n_traj == (W - 1) * ni
    x, v, a = O.minjerk(wp, ni)
    for got, want in ((out["q"], x), (out["qd"], v), (out["qdd"], a)):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12
    ff = -1
    for k in range(len(x)):
        if not O.torque_ok(x[k], q["mode"], q["mass"], v[k], a[k]):
            ff = k
            break
    assert fin.first_fail == ff
    assert fin.status == (_lib.PLAN_VALIDATION_FAILED if ff >= 0 else _lib.PLAN_OK)


@pytest.mark.parametrize("name", list(CR.FIXTURES))
def test_plan_connect_vs_restatement(name):
    from torque_constrained_motion_planning_amd import _lib
    n_obs, seed, K, passes = CR.FIXTURES[name]
    q = CR.query(O, n_obs, seed)
    e, twin = fresh(), fresh()
    try:
        grow(e, q)
        grow(twin, q)
        tree, ref = restate(e, q, K, passes, CR.SAMPLES + 2)
        rr = ref["result"]
        assert CR.purpose(name, rr) is None, CR.purpose(name, rr)
        d0, n0 = e.plan_digest()
        assert (d0, n0) == twin.plan_digest() and n0 == len(tree[0])
        r = e.plan_connect(K, passes)
        same_record(r, rr)
        cfg, cost, par = tree_of(e)
        assert cfg[:n0].tobytes() == tree[0].tobytes() and cost[:n0].tobytes() == tree[1].tobytes()
        assert par[:n0].tobytes() == tree[2].tobytes()
        if rr["status"] == CR.OK:
            assert len(cfg) == n0 + 1 and e.plan_digest()[1] == n0 + 1
            assert e.plan_digest()[0] != d0
            assert cfg[n0].tobytes() == ref["node"][:7].tobytes() and par[n0] == rr["parent"]
            assert cost[n0] == r.cost_after and close(cost[n0], ref["node"][7])
            assert e.plan_goal() == (n0, r.cost_after)
            fin = e.plan_finish()
            assert (fin.goal_found, fin.goal_node, fin.n_nodes) == (1, n0, n0 + 1)
            assert fin.goal_cost == r.cost_after
            check_path(q, e, tree, ref, fin, e.plan_fetch(fin))
            # the plan's own counters are untouched
            ft = twin.plan_finish()
            for f in ("n_samples", "edge_steps", "pairs_tested", "pairs_sat", "pairs_exact",
                      "nn_pairs", "n_rewires", "rewire_steps", "launches_nearest"):
                assert getattr(fin, f) == getattr(ft, f), f
        else:
            # nothing changed: the digest, the tree and the finish of a twin that never called it
            assert e.plan_digest() == (d0, n0) and len(cfg) == n0
            assert e.plan_goal() == twin.plan_goal()
            a, b = e.plan_finish(), twin.plan_finish()
            assert a.as_dict() == b.as_dict()
            if a.status != _lib.PLAN_NO_GOAL:
                oa, ob = e.plan_fetch(a), twin.plan_fetch(b)
                for k in ("waypoints", "q", "qd", "qdd", "psg", "tau"):
                    assert oa[k].tobytes() == ob[k].tobytes(), k
    finally:
        e.close()
        twin.close()


def test_plan_connect_tree_full():
    """16 boxes, seed 12, 16 samples in rounds of 4: every sample is accepted, so a tree of
    max_nodes = 17 is full, no goal node exists, and the stage has a winner."""
    from torque_constrained_motion_planning_amd import _lib
    q = CR.query(O, 16, 12)
    e, twin = fresh(), fresh()
    try:
        grow(twin, q, extra=1, samples=16, batch=4)
        n0 = twin.plan_digest()[1]
        assert n0 == 17 and twin.plan_goal()[0] == -1, "the fixture proves nothing"
        grow(e, q, extra=0, samples=16, batch=4)
        assert e.plan_digest() == twin.plan_digest()
        tree, ref = restate(e, q, 64, 1, 17)
        assert ref["result"]["status"] == CR.TREE_FULL, (ref["result"], "the fixture proves nothing")
        r = e.plan_connect(64, 1)
        same_record(r, ref["result"])
        assert (r.status, r.goal_node_after, r.cost_after) == (_lib.CONNECT_TREE_FULL, -1, 0.0)
        assert e.plan_digest() == twin.plan_digest() and e.plan_goal() == twin.plan_goal()
        cfg, cost, par = tree_of(e)
        assert (cfg.tobytes(), cost.tobytes(), par.tobytes()) == tuple(x.tobytes() for x in tree)
        assert e.plan_finish().as_dict() == twin.plan_finish().as_dict()
        # with room for the node the same winner is appended
        rt = twin.plan_connect(64, 1)
        assert (rt.status, rt.parent, rt.rank) == (_lib.CONNECT_OK, r.parent, r.rank)
        assert twin.plan_goal()[0] == 17
    finally:
        e.close()
        twin.close()


# ---- 4. lifetime -----------------------------------------------------------------------------
def test_connect_then_shortcut_then_finish():
    from torque_constrained_motion_planning_amd import _lib
    q = CR.query(O, *CR.FIXTURES["rescues"][:2])
    e = fresh()
    try:
        grow(e, q)
        assert e.plan_shortcut().status == _lib.PLAN_NO_GOAL
        r = e.plan_connect(64, 1)
        assert r.status == _lib.CONNECT_OK
        sc = e.plan_shortcut()
        assert sc.status == 0 and sc.n_before >= 2 and sc.cost_after <= sc.cost_before
        assert close(sc.cost_before, r.cost_after) or abs(sc.cost_before - r.cost_after) < 1e-9
        fin = e.plan_finish()
        assert fin.goal_found == 1 and fin.n_waypoints == sc.n_after
        assert fin.status in (_lib.PLAN_OK, _lib.PLAN_VALIDATION_FAILED)
        wp = e.plan_fetch(fin)["waypoints"]
        assert wp[0].tobytes() == START.tobytes() and CR.distance(wp[-1], q["goal"]) < 1e-2
    finally:
        e.close()


def test_connect_after_finish_invalidates_the_rows():
    from torque_constrained_motion_planning_amd import _lib
    q = CR.query(O, *CR.FIXTURES["improves"][:2])
    e = fresh()
    try:
        grow(e, q)
        sc = e.plan_shortcut()  # (a stored list of the old path: the connection drops it)
        fin = e.plan_finish()
        assert fin.goal_found == 1 and fin.n_waypoints == sc.n_after
        assert e.plan_repair(check_only=True).status != _lib.REPAIR_NOT_APPLICABLE
        r = e.plan_connect(64, 1)
        assert r.status == _lib.CONNECT_OK
        assert e.plan_retime().status == _lib.RETIME_NOT_APPLICABLE
        assert e.plan_repair().status == _lib.REPAIR_NOT_APPLICABLE
        fin2 = e.plan_finish()
        assert fin2.goal_found == 1 and fin2.goal_cost == r.cost_after < fin.goal_cost
        wp = e.plan_fetch(fin2)["waypoints"]  # the tree's new path, not the stored list
        assert abs(SR.path_cost(wp) - r.cost_after) <= 1e-9 * r.cost_after
        assert e.plan_repair(check_only=True).status != _lib.REPAIR_NOT_APPLICABLE
        # nothing can beat a goal cost of key_min: NONE, and the finished rows stay valid
        r2 = e.plan_connect(64, 1)
        if r2.status == _lib.CONNECT_NONE:
            assert e.plan_repair(check_only=True).status != _lib.REPAIR_NOT_APPLICABLE
    finally:
        e.close()


@pytest.mark.parametrize("graphs", ["1", "0"])
def test_connect_then_one_more_round(graphs, monkeypatch):
    """The rounds after a connection see a tree one node larger than their samples account for:
    the host's bound on the snapshot, the capacity checks and the round graph's key follow."""
    from torque_constrained_motion_planning_amd import _lib
    monkeypatch.setenv("TCMP_GRAPHS", graphs)
    q = CR.query(O, *CR.FIXTURES["rescues"][:2])
    e = fresh()
    try:
        grow(e, q, extra=1 + CR.BATCH)
        r = e.plan_connect(64, 1)
        assert r.status == _lib.CONNECT_OK
        n1 = r.n_nodes + 1
        e.plan_run(CR.BATCH, CR.BATCH)
        cfg, cost, par = tree_of(e)
        assert len(cfg) > n1, "the round added nothing: the test proves nothing"
        assert par[0] == -1 and (par[1:] < np.arange(1, len(cfg))).all() and (par[1:] >= 0).all()
        for i in range(1, len(cfg)):
            assert close(cost[i], cost[par[i]] + CR.distance(cfg[par[i]], cfg[i])), i
        # the new node took part in the round's nearest search like any other
        g, c = e.plan_goal()
        assert c <= r.cost_after and CR.distance(cfg[g], q["goal"]) < 1e-2
        fin = e.plan_finish()
        assert fin.goal_found == 1 and fin.n_nodes == len(cfg)
        assert fin.status in (_lib.PLAN_OK, _lib.PLAN_VALIDATION_FAILED)
        # the tree is full for another round of this size
        with pytest.raises(_lib.TcmpError, match="error -3"):
            e.plan_run(CR.BATCH, CR.BATCH)
    finally:
        e.close()


def test_plan_connect_arguments():
    from torque_constrained_motion_planning_amd import _lib
    e = fresh()
    try:
        with pytest.raises(_lib.TcmpError, match="error -1"):
            e.plan_connect()
        q = CR.query(O, *CR.FIXTURES["no_eligible"][:2])
        grow(e, q, samples=256)
        for kw in (dict(max_candidates=-1), dict(max_candidates=65537), dict(passes=9),
                   dict(passes=-1)):
            with pytest.raises(_lib.TcmpError, match="error -1"):
                e.plan_connect(**kw)
        assert e.plan_connect(0, 0).status in (_lib.CONNECT_OK, _lib.CONNECT_NONE)
    finally:
        e.close()


# ---- 5. fleet --------------------------------------------------------------------------------
def test_plan_connect_fleet():
    """Two box plans grown in fused rounds and connected on their own engines == the same two
    queries on lone engines."""
    from torque_constrained_motion_planning_amd import _lib
    names = ("improves", "rescues")
    qs = [CR.query(O, *CR.FIXTURES[n][:2]) for n in names]
    lone = []
    for q in qs:
        e = fresh()
        grow(e, q)
        r = e.plan_connect(64, 1)
        fin = e.plan_finish()
        lone.append((r, tree_of(e), fin, e.plan_fetch(fin)))
        e.close()
    es = [fresh(), fresh()]
    try:
        for e, q in zip(es, qs):
            e.set_scene(q["obs"])
        st = _lib.plan_begin_many(es, [_lib.plan_cfg(START, q["goal"], q["mode"], q["mass"],
                                                     CR.EXEC, CR.SAMPLES + 2, CR.BATCH, q["seed"])
                                       for q in qs])
        assert st == [_lib.PLAN_OK] * 2
        _lib.plan_run_fused(es, CR.SAMPLES, CR.BATCH)
        rs = [e.plan_connect(64, 1) for e in es]
        trees = [tree_of(e) for e in es]
        fins = _lib.plan_finish_many(es)
        for e, r, tr, fin, (r0, tr0, fin0, out0) in zip(es, rs, trees, fins, lone):
            assert r0.status == _lib.CONNECT_OK
            assert r.as_dict() == r0.as_dict()
            for a, b in zip(tr, tr0):
                assert a.tobytes() == b.tobytes()
            out = e.plan_fetch(fin)
            for k in ("waypoints", "q", "qd", "qdd", "psg", "tau"):
                assert out[k].tobytes() == out0[k].tobytes(), k
            assert (fin.status, fin.n_waypoints, fin.n_traj, fin.first_fail, fin.goal_node,
                    fin.edge_steps, fin.n_nodes, fin.goal_cost) == \
                (fin0.status, fin0.n_waypoints, fin0.n_traj, fin0.first_fail, fin0.goal_node,
                 fin0.edge_steps, fin0.n_nodes, fin0.goal_cost)
    finally:
        for e in es:
            e.close()


# ---- 6. drop-in ------------------------------------------------------------------------------
def test_batched_connect_record():
    from torque_constrained_motion_planning_amd import _lib
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_batched
    q = CR.query(O, *CR.FIXTURES["rescues"][:2])
    e = fresh()
    try:
        args = (START, q["goal"], q["obs"], q["mode"], q["mass"], CR.EXEC, CR.SAMPLES)
        _, r0, raw0 = rrt_star_batched(*args, batch=CR.BATCH, seed=q["seed"], engine=e)
        assert r0.status == _lib.PLAN_NO_GOAL and not (raw0 and "connect" in raw0)
        res, r, raw = rrt_star_batched(*args, batch=CR.BATCH, seed=q["seed"], engine=e,
                                       connect=True, connect_candidates=64)
        cn = raw["connect"]
        assert isinstance(cn, _lib.ConnectResult) and cn.status == _lib.CONNECT_OK
        assert cn.n_nodes == r0.n_nodes and cn.goal_node_before == -1
        assert (r.goal_found, r.goal_node, r.n_nodes) == (1, cn.goal_node_after, cn.n_nodes + 1)
        assert r.goal_cost == cn.cost_after and len(raw["waypoints"]) == r.n_waypoints
        # one pass of one candidate finds nothing here: the record says so, the plan has no goal
        _, r1, raw1 = rrt_star_batched(*args, batch=CR.BATCH, seed=q["seed"], engine=e,
                                       connect=True, connect_candidates=1, connect_passes=1)
        assert raw1["connect"].status == _lib.CONNECT_NONE and raw1["connect"].n_tested == 1
        assert r1.status == _lib.PLAN_NO_GOAL and r1.n_nodes == r0.n_nodes
    finally:
        e.close()


def _golden_fns(z):
    from torque_constrained_motion_planning_amd import panda_primitives as PP
    from torque_constrained_motion_planning_amd import utils as U
    mode, mass = int(z["mode"]), float(z["mass"])
    prob = U.Problem(U.PandaRobot(), list(z["obs"]), U.Payload(mass), mass, float(z["exec_time"]),
                     torque_test={0: "base", 1: "nov", 2: "rne"}[mode])
    resolutions = 0.2 ** np.ones(7)
    radius = resolutions / 2
    joints = U.get_arm_joints(prob.robot)
    return dict(distance=U.get_distance_fn(prob.robot, joints, weights=np.reciprocal(radius)),
                sample=U.get_sample_fn(prob.robot, joints),
                extend=U.get_extend_fn(prob.robot, joints, resolutions=radius),
                collision=U.get_collision_fn(prob.robot, joints, list(z["obs"]),
                                             self_collisions=False),
                torque_fn=PP.select_torque_test(prob),
                dynam_fn=PP.get_dynamics_fn_v5(prob, resolutions))


def test_drop_in_connect():
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_force_aware
    z = np.load(os.path.join(GOLDEN, "rrt_box4_nov2.npz"))
    f = _golden_fns(z)
    args = (tuple(z["start"]), tuple(z["goal"]), f["distance"], f["sample"], f["extend"],
            f["collision"], f["torque_fn"], f["dynam_fn"])
    kw = dict(radius=[0.01], max_time=50, max_iterations=int(z["iters"]))
    e = f["collision"].engine
    goals = []
    for connect in (False, True):
        random.seed(int(z["seed"]))
        np.random.seed(int(z["seed"]))
        rrt_star_force_aware(*args, connect=connect, **kw)
        goals.append((e.plan_goal(), e.plan_digest()[1]))
    (g0, c0), n0 = goals[0]
    (g1, c1), n1 = goals[1]
    # the loop is the same; the stage either found a cheaper parent (one more node) or nothing
    assert g0 >= 0 and n1 in (n0, n0 + 1) and c1 <= c0
    assert (g1 == n0 and c1 < c0) if n1 == n0 + 1 else (g1, c1) == (g0, c0)
    with pytest.raises(TypeError):
        rrt_star_force_aware(*args, [0.01], 50, int(z["iters"]), .2, False, False, True)


def test_drop_in_connect_needs_native_callbacks():
    from torque_constrained_motion_planning_amd.rrt_star import rrt_star_force_aware
    z = np.load(os.path.join(GOLDEN, "rrt_box4_nov2.npz"))
    f = _golden_fns(z)
    dist = (lambda fn: (lambda a, b: fn(a, b)))(f["distance"])
    with pytest.raises(NotImplementedError, match="distance, extend, collision and torque"):
        rrt_star_force_aware(tuple(z["start"]), tuple(z["goal"]), dist, f["sample"], f["extend"],
                             f["collision"], f["torque_fn"], f["dynam_fn"], radius=[0.01],
                             max_time=50, max_iterations=int(z["iters"]), connect=True)
