"""Restatement of the held-body (attachment) model, for tests only.

Frames and depth come from tests/collision_ref.py (numpy and qhull over the description's joint
table; nothing shared with the engine): a held body is a set of vertices in its own (child)
frame, placed on a link of the description at parent_from_child, its world pose at q being
frames(q)[parent] @ parent_from_child; its depth against an obstacle is collision_ref.depth of
the two vertex sets; the held flag is any depth >= 0.04.  No joint-limit test, no test against
the robot's links, none among held bodies.

The edge rule: safe_path_force_aware(extend(a, b)) with the attachments in collision_fn is the
arm-and-torque walk (oracle.check_edge) cut at the first step of its accepted prefix whose held
flag is set; the prefix is regenerated in numpy as r * (q2 - q) + q, r = 1 / (n - i)."""
import numpy as np

import collision_ref as C

P = C.THRESHOLD
# the tool frame (panda_grasptarget) in panda_hand: the description's fixed joint, xyz 0 0 0.105
HAND_FROM_TOOL = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.105],
                           [0.0, 0.0, 0.0, 1.0]])
TOOL_BOX = (0.08, 0.08, 0.20)


def box_body(size):
    """The 8 corners of a box of full extents `size` about its frame's origin."""
    h = 0.5 * np.asarray(size, dtype=np.float64)
    return np.array([[sx, sy, sz] for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)
                     for sz in (-1.0, 1.0)]) * h


def prism_body(radius, height, sides=16):
    """A regular prism circumscribed about the cylinder (radius, height) along z."""
    a = 2.0 * np.pi * (np.arange(sides) + 0.5) / sides
    r = radius / np.cos(np.pi / sides)
    return np.array([[r * np.cos(t), r * np.sin(t), z] for z in (-0.5 * height, 0.5 * height)
                     for t in a])


class Held:
    """verts (n, 3) in the child frame; link: index into collision_ref.LINKS; pfc: 4x4."""

    def __init__(self, verts, link, parent_from_child):
        self.verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
        self.link = int(link)
        self.pfc = np.asarray(parent_from_child, dtype=np.float64).reshape(4, 4)


def on_tool(verts, tool_from_child=None):
    """A body on the tool frame: the hand's link, hand_from_tool folded into the placement."""
    T = np.eye(4) if tool_from_child is None else np.asarray(tool_from_child, dtype=np.float64)
    return Held(verts, C.LINKS.index("panda_hand"), HAND_FROM_TOOL @ T)


_chain = {}


def link_frame(q, name):
    """collision_ref.frames(q)[name] for one link: the same chain, per joint
    Trans(xyz) Rpy(rpy) then Rz(q) / Trans(axis * opening) / nothing, walked from the link up to
    the base with each joint's constant factor built once (tests/test_attach_host.py holds it to
    frames(), which builds every link's pose and every factor per call)."""
    if name not in _chain:
        m = C.model()
        steps, link = [], name
        while link != C.BASE:
            j = m["joint_child"].index(link)
            T0 = C._tf(C.rpy(m["joint_rpy"][j]), m["joint_xyz"][j])
            kind, arm, slide = m["joint_type"][j], None, None
            if kind == "revolute":
                arm = C.ARM_JOINTS.index(m["joint_names"][j])
            elif kind == "prismatic":
                slide = C._tf(np.eye(3), m["joint_axis"][j] * float(m["finger_open"]))
            steps.append((T0, arm, slide))
            link = m["joint_parent"][j]
        _chain[name] = steps[::-1]
    T = np.eye(4)
    for T0, arm, slide in _chain[name]:
        T = T @ T0
        if arm is not None:
            T = T @ C._tf(C._rot(2, q[arm]), np.zeros(3))
        elif slide is not None:
            T = T @ slide
    return T


def world_vertices(h, q, fr=None):
    T = (link_frame(q, C.LINKS[h.link]) if fr is None else fr[C.LINKS[h.link]]) @ h.pfc
    return h.verts @ T[:3, :3].T + T[:3, 3]


class Obstacles(list):
    """The scene as vertex sets (the boxes' corners, then the meshes' vertices), with each
    set's bounding sphere as collision_ref's pre-test takes it."""

    def __init__(self, boxes=None, meshes=None):
        rows = np.asarray(boxes if boxes is not None else np.zeros((0, 15))).reshape(-1, 15)
        super().__init__([C.box_vertices(b) for b in rows] +
                         [np.asarray(v, dtype=np.float64) for v in (meshes or [])])
        sph = [C._sphere(v) for v in self]
        self.centre = np.array([s[0] for s in sph]).reshape(-1, 3)
        self.radius = np.array([s[1] for s in sph])


def obstacle_vertices(boxes=None, meshes=None):
    return Obstacles(boxes, meshes)


def depths(held, q, obstacles, prune=True):
    """(n_held, n_obstacles) depths at q; pairs the sphere pre-test of collision_ref proves
    under SKIP_BELOW are -inf (prune=False: every pair's depth).  The bounding spheres' own
    bound, r_A + r_B - |c_A - c_B|, is taken for all obstacles at once before sphere_bound."""
    out = np.full((len(held), len(obstacles)), -np.inf)
    for i, h in enumerate(held):
        A = world_vertices(h, q)
        todo = range(len(obstacles))
        if prune and len(obstacles):
            ca, ra = C._sphere(A)
            ball = ra + obstacles.radius - np.linalg.norm(obstacles.centre - ca, axis=1)
            todo = np.flatnonzero(ball >= C.SKIP_BELOW)
        for j in todo:
            B = obstacles[j]
            if prune and C.sphere_bound(A, B) < C.SKIP_BELOW:
                continue
            out[i, j] = C.depth(A, B)
    return out


def held_flag(held, q, obstacles):
    d = depths(held, q, obstacles)
    return bool(d.size and d.max() >= P)


def refine(q, q2, n, i):
    """One step of get_refine_fn (utils.py:3037), numpy's own arithmetic."""
    r = 1.0 / (n - i)
    return r * (np.asarray(q2, dtype=np.float64) - q) + q


def prefix(a, b, n_steps, count):
    """The configurations after 1 .. count refine steps from a toward b."""
    q = np.asarray(a, dtype=np.float64).copy()
    out = []
    for i in range(count):
        q = refine(q, b, n_steps, i)
        out.append(q)
    return out


def cut(a, b, n_steps, n_safe, flag_fn):
    """The edge rule on an arm walk's (n_steps, n_safe): n_safe' = the first step of 0 ..
    n_safe - 1 whose configuration flag_fn flags (n_safe if none), last' = the configuration
    after n_safe' refine steps, counted extend steps = the combined sequential walk's."""
    steps = prefix(a, b, n_steps, n_safe)
    j = n_safe
    for i, q in enumerate(steps):
        if flag_fn(q):
            j = i
            break
    last = np.asarray(a, dtype=np.float64).copy() if j == 0 else steps[j - 1]
    counted = j + 1 if j < n_steps else n_steps
    return j, last, counted


def edge(a, b, held, boxes, obstacles, mode, mass):
    """(n_steps, n_safe', last') of the combined walk; the arm and torque part is the oracle's
    check_edge over `boxes` and whatever meshes the caller installed with oracle.set_meshes,
    the held part this module's over `obstacles` (the same scene as vertex sets)."""
    import oracle as O
    n_safe, n_steps, _ = O.check_edge(a, b, boxes, mode, mass)
    j, last, _ = cut(a, b, n_steps, n_safe, lambda q: held_flag(held, q, obstacles))
    return n_steps, j, last
