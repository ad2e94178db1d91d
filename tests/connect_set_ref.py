"""Restatement of the goal-set connection (include/tcmp.h tcmp_connect_goal_set,
tcmp_plan_connect_goal_set), the reference of tests/test_connect_set_host.py and
tests/test_gpu_connect_set.py.  Nothing here imports the package; it builds on
tests/connect_ref.py's distance, select and oracle_check.

  nearest   s_ij = sum_k w_k * (d * d), d = G_jk - c_ik, k ascending, one fp64 operation after
            the other; j*(i) = the lowest j attaining min_j s_ij (strict <, j ascending; a NaN
            s_ij never wins)
  key       key_i = g_i + sqrt(s_{i j*})
  the rest  connect_ref's stage with G replaced per candidate by G_{j*(i)}: eligible key_i < B,
            the M = min(n_eligible, K * passes) smallest by (key, i), pass p tests ranks
            [p K, min(M, (p + 1) K)) with check(c_i, G_j*), valid iff n_safe > 0 and
            dist(last, G_j*) < tol, c = g_i + dist(c_i, last), the winner the valid one with c < B
            smallest by (c, rank), the first pass with a winner ends the stage
  per goal  near (eligible nodes whose j* it is), tested, valid (over the passes run)
"""
import math

import numpy as np

import connect_ref as CR

OK, NONE, TREE_FULL = CR.OK, CR.NONE, CR.TREE_FULL
W10 = CR.W10


def sums(cfg, G, w=W10):
    """s_ij for all rows at once, (T, n): the same operations in the same order, elementwise."""
    cfg = np.asarray(cfg, dtype=np.float64).reshape(-1, 7)
    G = np.asarray(G, dtype=np.float64).reshape(-1, 7)
    s = np.zeros((len(cfg), len(G)))
    for k in range(7):
        d = G[None, :, k] - cfg[:, None, k]
        s = s + np.float64(w[k]) * (d * d)
    return s


def nearest(cfg, G, w=W10):
    """-> (j* (T,), s_min (T,)); s_min = inf where no sum is below it (j* = 0 then)."""
    cfg = np.asarray(cfg, dtype=np.float64).reshape(-1, 7)
    G = np.asarray(G, dtype=np.float64).reshape(-1, 7)
    sm = np.full(len(cfg), np.inf)
    jm = np.zeros(len(cfg), dtype=np.int64)
    for j in range(len(G)):  # (one goal at a time: sums() of a large tree would not fit)
        s = np.zeros(len(cfg))
        for k in range(7):
            d = G[j, k] - cfg[:, k]
            s = s + np.float64(w[k]) * (d * d)
        with np.errstate(invalid="ignore"):
            lt = s < sm
        sm = np.where(lt, s, sm)
        jm = np.where(lt, j, jm)
    return jm, sm


def nearest_scalar(c, G, w=W10):
    """The definition as written, one node: -> (j*, s_min)."""
    sm, jm = math.inf, 0
    for j, g in enumerate(G):
        s = 0.0
        for k in range(7):
            d = float(g[k]) - float(c[k])
            s += float(w[k]) * (d * d)
        if s < sm:
            sm, jm = s, j
    return jm, sm


def keys(cfg, cost, G, w=W10):
    """-> (key (T,), j* (T,))"""
    jm, sm = nearest(cfg, G, w)
    return np.asarray(cost, dtype=np.float64) + np.sqrt(sm), jm


def connect_set(cfg, cost, goals, check, bound=math.inf, w=W10, tol=1e-2, K=1024, passes=1,
                goal_node=-1, max_nodes=None):
    """connect_ref.connect for a goal set.  -> its dict, with result["goal_index"] and
    result["n_goals"], `goal` (j* of the M selected, -1: not tested), `per_goal` ((3, n) int64:
    near, tested, valid) and on OK or TREE_FULL `tgt`, the winner's goal row."""
    cfg = np.asarray(cfg, dtype=np.float64).reshape(-1, 7)
    cost = np.asarray(cost, dtype=np.float64).reshape(-1)
    goals = np.asarray(goals, dtype=np.float64).reshape(-1, 7)
    T, n = len(cfg), len(goals)
    assert 1 <= n <= 256 and np.isfinite(goals).all()
    if goal_node >= 0:
        bound = float(cost[goal_node])
    key, jm = keys(cfg, cost, goals, w)
    ids, n_el = CR.select(key, bound, K, passes)
    M = len(ids)
    per = np.zeros((3, n), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        per[0] = np.bincount(jm[key < bound], minlength=n)
    nsafe = np.full(M, -1, dtype=np.int32)
    nsteps = np.full(M, -1, dtype=np.int32)
    gsel = np.full(M, -1, dtype=np.int32)
    r = dict(status=NONE, passes_run=0, n_nodes=T, n_eligible=n_el, n_selected=M, n_tested=0,
             n_valid=0, edge_steps=0, goal_node_before=goal_node, goal_node_after=goal_node,
             parent=-1, rank=-1, cost_before=float(cost[goal_node]) if goal_node >= 0 else 0.0,
             key_min=float(key[ids[0]]) if M else 0.0, n_goals=n, goal_index=-1)
    r["cost_after"] = r["cost_before"]
    node = meta = tgt = None
    for p in range(passes):
        if p * K >= M:
            break
        best = None
        for rank in range(p * K, min(M, (p + 1) * K)):
            i = int(ids[rank])
            j = int(jm[i])
            G = goals[j]
            ns, nt, last = check(cfg[i], G)
            nsafe[rank], nsteps[rank], gsel[rank] = ns, nt, j
            r["n_tested"] += 1
            per[1, j] += 1
            r["edge_steps"] += nt if ns == nt else ns + 1
            if ns > 0 and CR.distance(last, G, w) < tol:
                r["n_valid"] += 1
                per[2, j] += 1
                c = float(cost[i]) + CR.distance(cfg[i], last, w)
                if c < bound and (best is None or c < best[0]):
                    best = (c, rank, i, np.array(last, dtype=np.float64), nt, ns, j)
        r["passes_run"] = p + 1
        if best is not None:
            c, rank, i, last, nt, ns, j = best
            r["parent"], r["rank"], r["goal_index"] = i, rank, j
            node, meta, tgt = np.concatenate([last, [c]]), (nt, ns), goals[j].copy()
            if max_nodes is not None and T == max_nodes:
                r["status"] = TREE_FULL
            else:
                r["status"] = OK
                r["cost_after"] = c
                if max_nodes is not None:
                    r["goal_node_after"] = T
            break
    return dict(result=r, ids=ids.astype(np.int32), keys=key[ids], goal=gsel, nsafe=nsafe,
                nsteps=nsteps, node=node, meta=meta, tgt=tgt, per_goal=per)


# ---- the goal family of a query ---------------------------------------------------------------
N_FREE, N_GOALS, SPREAD = 32, 8, 1.0


def goal_family(O, q, n_goals=N_GOALS):
    """IK images of the query goal's own pose, the query goal at index 0: free values the goal's
    own q7, then the 31 midpoints of joint 7's range; every O.ik8 solution at joint 6's image
    (tcmp_goal_search's rule) through the limits, O.torque_ok and O.collision; sorted by the
    distance from START; kept greedily when more than SPREAD from every goal kept so far."""
    goal = np.asarray(q["goal"], dtype=np.float64)
    T = O.fk8(goal)
    lo7, hi7 = float(CR.LO[6]), float(CR.HI[6])
    free = [float(goal[6])] + [lo7 + (i + 0.5) / (N_FREE - 1) * (hi7 - lo7)
                               for i in range(N_FREE - 1)]
    cand = []
    for q7 in free:
        sols, _ = O.ik8(T, q7)
        for s in sols:
            s = np.array(s, dtype=np.float64)
            if s[5] < CR.LO[5] and s[5] + 2 * math.pi <= CR.HI[5]:
                s[5] = s[5] + 2 * math.pi
            if np.any(s < CR.LO) or np.any(CR.HI < s):
                continue
            if not O.torque_ok(s, CR.MODE, CR.MASS) or O.collision(s, q["obs"]):
                continue
            cand.append(s)
    cand.sort(key=lambda s: CR.distance(CR.START, s))
    kept = [goal]
    for s in cand:
        if len(kept) >= n_goals:
            break
        if all(CR.distance(g, s) > SPREAD for g in kept):
            kept.append(s)
    return np.array(kept)


# name: (boxes, scene / goal seed, K, passes) -- connect_ref's trees (B = 256, 3,072 samples)
FIXTURES = {
    "other_goal": (16, 2, 64, 1),   # a non-root parent at a rank > 0 wins with another goal,
                                    # cheaper than the single goal's connection
    "rescues4": (32, 2, 64, 1),     # no goal node; four goals are tested, one is reached
    "none2": (16, 11, 64, 1),       # no goal node; two goals are tested, none is reached
    "opens": (16, 1, 64, 1),        # the single goal has nothing eligible; the set connects
}


def purpose(name, r, per, single):
    """Does the fixture still serve its purpose?  r, per: the set's result and counts; single:
    connect_ref.connect's result on the query goal alone.  -> None, or what is wrong."""
    tested = int((per[1] > 0).sum())
    want = {
        "other_goal": r["status"] == OK and r["goal_index"] != 0 and r["rank"] > 0
        and r["parent"] != 0 and single["status"] == OK and r["cost_after"] < single["cost_after"],
        "rescues4": r["goal_node_before"] < 0 and r["status"] == OK and tested == 4,
        "none2": r["goal_node_before"] < 0 and r["status"] == NONE and tested == 2
        and r["n_valid"] == 0,
        "opens": single["status"] == NONE and single["n_eligible"] == 0 and r["status"] == OK,
    }[name]
    return None if want else (name, r, per.tolist(), single, "the fixture proves nothing")
