"""An independent reference of the collision model, for tests only.

It shares no code, no constants and no algorithm with the engine, the oracle
(oracle/tcmp_oracle.c) or the package's hull.py: plain numpy and scipy over the data fixture
tests/golden/panda_collision_model.npz (the robot description's joint table and the collision
meshes' vertices, written by tests/golden/gen_collision_model.py).

The model's stated definition, restated here:

  * frames(q): every link's pose by the description's chain, per joint
    Trans(xyz) . Rpy(rpy) . Rz(q) (revolute), Trans(axis * opening) (the finger prismatic joints,
    held at the fixture's opening), identity (fixed);
  * a link's shape is the convex hull of its mesh vertices under its collision origin;
  * depth(A, B): the penetration depth of two convex point sets = the distance from the origin
    to the boundary of their Minkowski difference {a - b} when the origin is inside it, a
    negative number ("separated") otherwise;
  * flag: a joint outside its inclusive limits, or any pair's depth >= 0.04.

depth() builds the Minkowski difference's hull with qhull.  qhull gives the facet normals; each
facet's offset is then taken again as the exact support max_a n.a - min_b n.b of the difference
along that normal, so a rounded or merged facet plane (nearly coplanar facets, as with the thin
plate and the 1e-3 rad wedge of pair_hulls.degenerate_meshes) costs only the second order of the
normal's error.  A difference set qhull rejects as flat is joggled ("QJ") and treated the same
way; both inputs being solid, that path is not taken by any pair of the suite (QJ_USED counts).

A pre-test skips pairs that are provably below the threshold.  The depth of two bodies is at
most that of their bounding spheres, r_A + r_B - |c_A - c_B|, and at most their overlap
max_a n.a - min_b n.b along any one direction n (the line of centres and the coordinate axes
are tried); a pair with such a bound under SKIP_BELOW (0.03, a centimetre under the threshold)
is reported as -inf.
"""
import os

import numpy as np
from scipy.spatial import ConvexHull
from scipy.spatial import QhullError

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_PATH = os.path.join(HERE, "golden", "panda_collision_model.npz")

THRESHOLD = 0.04
SKIP_BELOW = 0.03
QJ_USED = [0]

# the moving collision links in the order the project numbers them, and the static base
LINKS = ("panda_link1", "panda_link2", "panda_link3", "panda_link4", "panda_link5", "panda_link6",
         "panda_link7", "panda_hand", "panda_leftfinger", "panda_rightfinger")
BASE = "panda_link0"
ARM_JOINTS = tuple("panda_joint%d" % i for i in range(1, 8))

_model = None


def model():
    global _model
    if _model is None:
        z = np.load(MODEL_PATH)
        m = {k: z[k] for k in z.files}
        m["joint_names"] = [str(s) for s in m["joint_names"]]
        m["joint_type"] = [str(s) for s in m["joint_type"]]
        m["joint_parent"] = [str(s) for s in m["joint_parent"]]
        m["joint_child"] = [str(s) for s in m["joint_child"]]
        m["coll_link"] = [str(s) for s in m["coll_link"]]
        m["coll_mesh"] = [str(s) for s in m["coll_mesh"]]
        _model = m
    return _model


def limits():
    """(lower (7,), upper (7,)) of the arm joints, the description's literals."""
    m = model()
    idx = [m["joint_names"].index(j) for j in ARM_JOINTS]
    return m["joint_lower"][idx].copy(), m["joint_upper"][idx].copy()


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    if axis == 0:
        return np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])
    if axis == 1:
        return np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def rpy(r):
    """URDF fixed-axis roll, pitch, yaw: Rz(yaw) Ry(pitch) Rx(roll)."""
    return _rot(2, r[2]) @ _rot(1, r[1]) @ _rot(0, r[0])


def _tf(R, p):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = p
    return T


def frames(q):
    """{link name: 4x4 pose in the base frame} of every link of the description at arm
    configuration q (7,), the fingers at the fixture's opening."""
    m = model()
    q = np.asarray(q, dtype=np.float64).reshape(7)
    out = {BASE: np.eye(4)}
    todo = list(range(len(m["joint_names"])))
    while todo:
        rest = []
        for j in todo:
            par = m["joint_parent"][j]
            if par not in out:
                rest.append(j)
                continue
            T = out[par] @ _tf(rpy(m["joint_rpy"][j]), m["joint_xyz"][j])
            name, kind, axis = m["joint_names"][j], m["joint_type"][j], m["joint_axis"][j]
            if kind == "revolute":
                assert np.array_equal(axis, [0.0, 0.0, 1.0]), name
                T = T @ _tf(_rot(2, q[ARM_JOINTS.index(name)]), np.zeros(3))
            elif kind == "prismatic":
                T = T @ _tf(np.eye(3), axis * float(m["finger_open"]))
            else:
                assert kind == "fixed", kind
            out[m["joint_child"][j]] = T
        assert len(rest) < len(todo), "the joint table is not a tree rooted at the base"
        todo = rest
    return out


def link_vertices(name):
    """A link's mesh vertices in its own frame, the collision origin applied."""
    m = model()
    k = m["coll_link"].index(name)
    v = m["verts_" + m["coll_mesh"][k]]
    return v @ rpy(m["coll_rpy"][k]).T + m["coll_xyz"][k]


def world_vertices(q):
    """The ten moving links' vertices in the base frame, in LINKS order."""
    fr = frames(q)
    return [link_vertices(n) @ fr[n][:3, :3].T + fr[n][:3, 3] for n in LINKS]


def base_vertices():
    return link_vertices(BASE)


def box_vertices(row):
    """The 8 corners of an obstacle row of 15: centre, rotation row-major (columns = axes), half."""
    row = np.asarray(row, dtype=np.float64).reshape(15)
    c, R, h = row[:3], row[3:12].reshape(3, 3), row[12:]
    s = np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0) for sz in (-1.0, 1.0)])
    return c + (s * h) @ R.T


def _sphere(v):
    c = 0.5 * (v.min(0) + v.max(0))
    return c, float(np.sqrt(((v - c) ** 2).sum(1).max()))


def sphere_bound(A, B):
    """An upper bound of depth(A, B): the depth of the bounding spheres, or the overlap along
    the line of centres or a coordinate axis where that is smaller."""
    ca, ra = _sphere(A)
    cb, rb = _sphere(B)
    dist = float(np.linalg.norm(ca - cb))
    n = np.concatenate([np.eye(3), -np.eye(3)])
    if dist > 0:
        n = np.concatenate([n, [(cb - ca) / dist]])
    return min(ra + rb - dist, float(((A @ n.T).max(0) - (B @ n.T).min(0)).min()))


def depth(A, B):
    """Penetration depth of conv(A) and conv(B), (n, 3) and (m, 3) points: the distance from the
    origin to the boundary of conv(A) - conv(B) when it lies inside; negative when the sets are
    separated (then only the sign has a meaning)."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    D = (A[:, None, :] - B[None, :, :]).reshape(-1, 3)
    try:
        h = ConvexHull(D)
    except QhullError:
        QJ_USED[0] += 1
        h = ConvexHull(D, qhull_options="QJ")
    n = np.unique(h.equations[:, :3], axis=0)
    n /= np.linalg.norm(n, axis=1)[:, None]
    support = (A @ n.T).max(0) - (B @ n.T).min(0)
    return float(support.min())


def pair_depths(q, boxes=None, meshes=None, self_pairs=None, body=False, prune=True):
    """Every pair's depth at q: moving links x boxes, moving links x meshes (vertex arrays in
    the base frame), the given self pairs (LINKS indices), and link0 x obstacles for `body`.
    Pairs the sphere pre-test proves under SKIP_BELOW are -inf.  Returns a flat array."""
    W = world_vertices(q)
    obstacles = [box_vertices(b) for b in np.asarray(boxes if boxes is not None else
                                                     np.zeros((0, 15))).reshape(-1, 15)]
    obstacles += [np.asarray(v, dtype=np.float64) for v in (meshes or [])]
    pairs = [(W[l], o) for l in range(len(LINKS)) for o in obstacles]
    pairs += [(W[a], W[b]) for a, b in (self_pairs or [])]
    if body:
        base = base_vertices()
        pairs += [(base, o) for o in obstacles]
    out = np.full(len(pairs), -np.inf)
    for i, (A, B) in enumerate(pairs):
        if prune and sphere_bound(A, B) < SKIP_BELOW:
            continue
        out[i] = depth(A, B)
    return out


def limits_violated(q):
    lo, hi = limits()
    q = np.asarray(q, dtype=np.float64).reshape(7)
    return bool(((q < lo) | (q > hi)).any())


def flag(q, boxes=None, meshes=None, self_pairs=None, body=False):
    """The collision flag of configuration q: outside the inclusive joint limits (not for
    `body`, the body-level check has no limit test), or max depth >= 0.04."""
    if not body and limits_violated(q):
        return True
    d = pair_depths(q, boxes, meshes, self_pairs, body)
    return bool(len(d) and d.max() >= THRESHOLD)
