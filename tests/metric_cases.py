"""Distance weights and edge resolutions other than the planner's 10 / 0.1: the vectors, a plain
Python restatement of the reference's extend and safe path, and the cases that the host tests
(test_oracle_golden.py, test_shortcut_host.py, test_connect_host.py) and tests/test_gpu_metric.py
share.  Nothing here imports the package but the scene generators.

The reference takes both vectors per joint (utils.py:3003-3017 get_distance_fn, :3061-3077
get_extend_fn); its defaults are weights 1 and DEFAULT_RESOLUTION = radians(3) on every joint,
and its planner passes 10 and 0.1 (panda_primitives.py:333-337).
"""
import functools
import math

import numpy as np

import connect_ref as CR
import shortcut_ref as SR

LO, HI, START = CR.LO, CR.HI, CR.START
NO_OBS = np.zeros((0, 15))
ONES = np.ones(7)
W_NONUNI = np.array([10.0, 3.0, 7.5, 1.0, 20.0, 0.5, 10.0])
R_NONUNI = np.array([0.05, 0.1, 0.2, 0.1, 0.4, 0.3, 0.125])
DEFAULT_RESOLUTION = math.radians(3)     # utils.py:3061
RESOLUTIONS = {"uni005": 0.05 * ONES, "nonuni": R_NONUNI, "uni1": 1.0 * ONES}
MODE_RNE, MODE_BASE = 2, 0


# ---- utils.py:3031-3077 and rrt_star.py:90-98, restated ---------------------------------------
def extend_ref(q1, q2, resolutions):
    """list(get_extend_fn(resolutions)(q1, q2)): int(norm(diff / resolutions)) + 1 refine steps."""
    q1 = tuple(float(x) for x in q1)
    q2 = tuple(float(x) for x in q2)
    diff = tuple(b - a for b, a in zip(q2, q1))
    steps = int(np.linalg.norm(np.divide(diff, resolutions), ord=2))
    num_steps = steps + 1
    out = []
    q = q1
    for i in range(num_steps):
        positions = (1. / (num_steps - i)) * np.array(tuple(b - a for b, a in zip(q2, q))) + q
        q = tuple(positions)
        out.append(q)
    return out


def check_edge_ref(O, q1, q2, obs, mode, mass, resolutions):
    """safe_path_force_aware(extend(q1, q2), collision, torque) as check_edge reports it:
    (len(safe prefix), len(extend), prefix[-1] or None).  The collision and torque predicates are
    the oracle's, one configuration at a time; the walk is the reference's."""
    pts = extend_ref(q1, q2, resolutions)
    n = 0
    for q in pts:
        q = np.array(q, dtype=np.float64)
        if O.collision(q, obs, cull=2):
            break
        if not O.torque_ok(q, mode, mass):
            break
        n += 1
    return n, len(pts), (np.array(pts[n - 1]) if n else None)


def ref_check(O, obs, mode, mass, resolutions):
    """check(a, b) for shortcut_ref / connect_ref through check_edge_ref."""
    def check(a, b):
        ns, nt, last = check_edge_ref(O, a, b, obs, mode, mass, resolutions)
        return ns, nt, (last if ns else np.zeros(7))
    return check


# ---- edges -----------------------------------------------------------------------------------
def random_edges(rng, n):
    """n edges inside the joint limits: the first half `a + N(0, 0.3)` (clipped), the rest long."""
    a = LO + (HI - LO) * rng.random((n, 7))
    b = LO + (HI - LO) * rng.random((n, 7))
    b[:n // 2] = np.clip(a[:n // 2] + rng.normal(0, 0.3, (n // 2, 7)), LO, HI)
    return a, b


def hand_edges():
    """(from, to, resolutions, n_steps): an edge of no length is one step; one whose scaled norm
    is exactly an integer -- joint 6 moved by 3 * 0.125 at resolution 0.125, every number exact in
    binary -- takes that integer plus one."""
    q = START.copy()
    q[6] = 0.5
    to = q.copy()
    to[6] = 0.5 + 3 * 0.125
    assert (to[6] - q[6]) / R_NONUNI[6] == 3.0
    return [(q, q.copy(), R_NONUNI, 1), (q, to, R_NONUNI, 4)]


def box_scene(seed, n_obs):
    from torque_constrained_motion_planning_amd.scene import obstacle_array, random_box_scene
    if not n_obs:
        return NO_OBS
    return obstacle_array(random_box_scene(np.random.default_rng(seed), n_obs))


# ---- device-sampled rounds --------------------------------------------------------------------
# name: (batch, weights, resolutions, radius, boxes, torque mode, payload mass, query seed)
# The query seeds were picked on the CPU so that the oracle rewires in every case.
BATCHED = {
    "b256_nonuni_r4": (256, W_NONUNI, R_NONUNI, 4.0, 16, MODE_RNE, 5.0, 356),
    "b4096_nonuni_r4": (4096, W_NONUNI, R_NONUNI, 4.0, 16, MODE_RNE, 5.0, 4196),
    "b256_defaults_r1.5": (256, ONES, DEFAULT_RESOLUTION * ONES, 1.5, 8, MODE_RNE, 5.0, 357),
    "b1_nonuni_r6": (1, W_NONUNI, R_NONUNI, 6.0, 8, 1, 2.0, 101),
}


def batched_query(O, name):
    """tests/test_gpu_parity.py's recipe: the first draw of (goal, boxes) whose start and goal are
    collision-free and whose goal holds the payload.  -> dict of rrt_star_batched's arguments."""
    batch, w, res, radius, n_obs, mode, mass, seed = BATCHED[name]
    from torque_constrained_motion_planning_amd.scene import obstacle_array, random_box_scene
    rng = np.random.default_rng(seed)
    while True:
        goal = LO + (HI - LO) * rng.random(7)
        obs = obstacle_array(random_box_scene(rng, n_obs))
        if not (O.collision(START, obs) or O.collision(goal, obs)) and O.torque_ok(goal, mode, mass):
            break
    return dict(goal=goal, obs=obs, mode=mode, mass=mass, batch=batch, weights=w, resolutions=res,
                radius=radius, seed=1234 + batch,
                n_samples=3 * batch + 17 if batch > 1 else 600)


def batched_oracle(O, q):
    return O.rrt_run(START, q["goal"], q["n_samples"], q["obs"], q["mode"], q["mass"], 1.0,
                     batch=q["batch"], seed=q["seed"], cull=2, radius=q["radius"], tree=True,
                     threads=16 if q["batch"] >= 4096 else 1, weights=q["weights"],
                     resolutions=q["resolutions"])


# ---- the stages -------------------------------------------------------------------------------
SHORTCUT_SEED, CONNECT_SEED = 1, 1


@functools.lru_cache(maxsize=None)
def shortcut_case(O):
    """tests/test_gpu_shortcut.py's n40_box16 scene recipe (16 free boxes, rne 5 kg) with 40
    zig-zag vertices alone, so that chords and hops are edges of many steps, under the non-uniform
    weights and resolutions, with its restatement's result.  The seed was picked so that the
    restatement takes two chords, keeps an original hop and rejects hundreds of chords."""
    from torque_constrained_motion_planning_amd.scene import obstacle_array, random_box_scene
    rng = np.random.default_rng(SHORTCUT_SEED)
    obs = obstacle_array(random_box_scene(rng, 16, aligned=False))
    W = SR.zigzag(O, rng, 40, obs, MODE_RNE, 5.0, LO, HI, step=0.9, verts=True,
                  resolutions=R_NONUNI)
    ref, st = SR.shortcut(W, SR.oracle_check(O, obs, MODE_RNE, 5.0, R_NONUNI), 512, 1, W_NONUNI)
    return dict(obs=obs, mode=MODE_RNE, mass=5.0, W=W, ref=ref, st=st)


CONNECT_KP = ((32, 8), (300, 1))


@functools.lru_cache(maxsize=None)
def connect_case(O):
    """tests/test_gpu_connect.py's verdict recipe (connect_ref.query(16, 2), 300 zig-zag nodes
    with scaled path-length costs) under the non-uniform weights and resolutions, with the
    restatement's results for CONNECT_KP."""
    q = CR.query(O, 16, 2)
    rng = np.random.default_rng(CONNECT_SEED)
    W = SR.zigzag(O, rng, 300, q["obs"], CR.MODE, CR.MASS, LO, HI, resolutions=R_NONUNI)
    hop = [SR.dist(W[t], W[t + 1], W_NONUNI) for t in range(len(W) - 1)]
    cost = np.concatenate([[0.0], np.cumsum(hop)]) * 0.05
    check = CR.oracle_check(O, q["obs"], CR.MODE, CR.MASS, R_NONUNI)
    refs = {(K, p): CR.connect(W, cost, q["goal"], check, w=W_NONUNI, K=K, passes=p)
            for K, p in CONNECT_KP}
    return q, W, cost, refs
