#!/usr/bin/env python3
"""Generate the data fixtures of the independent collision reference (tests/collision_ref.py).

Dev-time only, like gen_golden.py: it reads the reference project's robot description
(src/models/panda_mod.urdf) and collision meshes (src/models/meshes/panda/collision/*.stl),
which never reach the GPU machine.  Usage:

  python tests/golden/gen_collision_model.py REFERENCE_SRC model    # panda_collision_model.npz
  python tests/golden/gen_collision_model.py REFERENCE_SRC probes   # collision_probes.npz

panda_collision_model.npz (data only):
  verts_<mesh>        unique vertices of <mesh>.stl (link0..link7, hand, finger): the file's
                      float32 values, stored exactly as float64
  joint_*             panda_joint1..8, panda_hand_joint, panda_finger_joint1/2: name, type,
                      parent, child, origin xyz / rpy (the file's own truncated literals), axis,
                      lower / upper limit (NaN on fixed joints)
  coll_*              per collision element: link, mesh, origin xyz / rpy (the right finger's
                      rpy 0 0 3.14159265359)
  finger_open         the finger joints' position while planning, with finger_open_source: the
                      reference's open_arm (panda_primitives.py:320-322) sets every gripper joint
                      to get_max_limit, i.e. the `upper` of panda_finger_joint1/2 = 0.04

collision_probes.npz: poses at chosen depths, found with collision_ref alone (the oracle gives
only the list of self pairs, as index pairs):
  link_*   per moving link 4 in-limit configurations with one box each (half extents 0.02..0.15,
           random rotation), slid along a random line until the link's depth is 0.04 + d for d in
           LINK_D; kept only if every other link stays below 0.04 - 5e-3 at all eight positions
  base_*   the same for panda_link0, 3 boxes, every moving link below 0.04 - 5e-3
  self_*   per probed self pair a joint-space line from a clear configuration to one where the
           pair is deep, solved for depth 0.04 + d, d in SELF_D, every other pair below 0.04 - 5e-3
Each family stores the configurations, the box rows (15 doubles), the probed link or pair, d and
the depth reached.
"""
import os
import struct
import sys
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)

MESHES = ("link0", "link1", "link2", "link3", "link4", "link5", "link6", "link7", "hand", "finger")
JOINTS = tuple("panda_joint%d" % i for i in range(1, 9)) + (
    "panda_hand_joint", "panda_finger_joint1", "panda_finger_joint2")
OPEN_SOURCE = ("panda_primitives.py:320-322 open_arm: every gripper joint goes to its maximum "
               "limit -> the upper limit of panda_finger_joint1 / panda_finger_joint2 "
               "(panda_mod.urdf:70, :77)")

LINK_D = (1e-7, -1e-7, 1e-6, -1e-6, 3e-5, -3e-5, 5e-3, -5e-3)
SELF_D = (1e-6, -1e-6, 3e-5, -3e-5, 5e-3, -5e-3)
CLEAR = 0.04 - 5e-3
TOL = 2e-12


def read_stl(path):
    d = open(path, "rb").read()
    cnt = struct.unpack("<I", d[80:84])[0]
    tri = np.frombuffer(d[84:84 + cnt * 50], dtype=np.dtype(
        [("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    return np.unique(tri["v"].reshape(-1, 3), axis=0).astype(np.float64)


def floats(s, n=3):
    v = [float(x) for x in s.split()]
    assert len(v) == n, s
    return v


def gen_model(ref_src):
    out = {}
    for m in MESHES:
        out["verts_" + m] = read_stl(os.path.join(ref_src, "models", "meshes", "panda", "collision",
                                                  m + ".stl"))
    root = ET.parse(os.path.join(ref_src, "models", "panda_mod.urdf")).getroot()
    joints = {j.get("name"): j for j in root.findall("joint")}
    J = {k: [] for k in ("type", "parent", "child", "xyz", "rpy", "axis", "lower", "upper")}
    for name in JOINTS:
        j = joints[name]
        o, ax, lim = j.find("origin"), j.find("axis"), j.find("limit")
        J["type"].append(j.get("type"))
        J["parent"].append(j.find("parent").get("link"))
        J["child"].append(j.find("child").get("link"))
        J["xyz"].append(floats(o.get("xyz")))
        J["rpy"].append(floats(o.get("rpy")))
        J["axis"].append(floats(ax.get("xyz")) if ax is not None else [0.0, 0.0, 0.0])
        fixed = j.get("type") == "fixed"
        J["lower"].append(np.nan if fixed else float(lim.get("lower")))
        J["upper"].append(np.nan if fixed else float(lim.get("upper")))
    out["joint_names"] = np.array(JOINTS)
    for k in ("type", "parent", "child"):
        out["joint_" + k] = np.array(J[k])
    for k in ("xyz", "rpy", "axis", "lower", "upper"):
        out["joint_" + k] = np.array(J[k], dtype=np.float64)
    cl, cm, cx, cr = [], [], [], []
    for link in root.findall("link"):
        c = link.find("collision")
        if c is None:
            continue
        o = c.find("origin")
        cl.append(link.get("name"))
        cm.append(os.path.splitext(os.path.basename(c.find("geometry/mesh").get("filename")))[0])
        cx.append(floats(o.get("xyz")) if o is not None else [0.0, 0.0, 0.0])
        cr.append(floats(o.get("rpy")) if o is not None else [0.0, 0.0, 0.0])
    out["coll_link"] = np.array(cl)
    out["coll_mesh"] = np.array(cm)
    out["coll_xyz"] = np.array(cx, dtype=np.float64)
    out["coll_rpy"] = np.array(cr, dtype=np.float64)
    # the opening: the upper limit of the finger joints (see OPEN_SOURCE); both must agree
    f1, f2 = JOINTS.index("panda_finger_joint1"), JOINTS.index("panda_finger_joint2")
    assert J["upper"][f1] == J["upper"][f2]
    out["finger_open"] = np.float64(J["upper"][f1])
    out["finger_open_source"] = np.array(OPEN_SOURCE)
    path = os.path.join(HERE, "panda_collision_model.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; finger_open", out["finger_open"])


# ---- probes ---------------------------------------------------------------------------------

def solve(f, lo, hi, flo, fhi, target):
    """t in [lo, hi] with f(t) = target to TOL, given f(lo) >= target > f(hi): false position and
    bisection steps alternate (the bracket is kept, so a root is found whatever f's shape)."""
    best_t, best_f = (lo, flo) if abs(flo - target) < abs(fhi - target) else (hi, fhi)
    for it in range(200):
        if abs(best_f - target) <= TOL:
            break
        mid = 0.5 * (lo + hi)
        t = lo + (hi - lo) * (flo - target) / (flo - fhi) if it % 2 == 0 else mid
        if not lo < t < hi:
            t = mid
        if not lo < t < hi:
            break
        ft = f(t)
        if abs(ft - target) < abs(best_f - target):
            best_t, best_f = t, ft
        if ft >= target:
            lo, flo = t, ft
        else:
            hi, fhi = t, ft
    return best_t, best_f


def rand_rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def slide_probes(C, rng, target_verts, other_verts, reach=0.6):
    """One box slid along a random line out of the hull `target_verts`: box rows and depths for
    every d of LINK_D, or None when the line never gets deep enough or another hull comes
    within CLEAR."""
    half = rng.uniform(0.02, 0.15, 3)
    R = rand_rot(rng)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    c0 = target_verts.mean(0)

    def row(t):
        return np.concatenate([c0 + t * u, R.ravel(), half])

    def f(t):
        return C.depth(target_verts, C.box_vertices(row(t)))
    grid = np.linspace(0.0, reach, 25)
    D = np.array([f(t) for t in grid])
    peak = int(D.argmax())
    if D[peak] < 0.04 + 5e-3 + 1e-4 or D[-1] >= CLEAR:
        return None
    rows, reached = [], []
    for d in LINK_D:
        k = peak + int(np.argmax(D[peak:] < 0.04 + d))
        t, ft = solve(f, grid[k - 1], grid[k], D[k - 1], D[k], 0.04 + d)
        if abs(ft - (0.04 + d)) > 1e-9 or (ft >= 0.04) != (d > 0):
            return None
        b = C.box_vertices(row(t))
        for o in other_verts:
            if C.sphere_bound(o, b) >= CLEAR and C.depth(o, b) >= CLEAR:
                return None
        rows.append(row(t)); reached.append(ft)
    return np.array(rows), np.array(reached)


def gen_probes():
    import collision_ref as C
    import oracle as O  # only for the list of self pairs (index pairs)
    rng = np.random.default_rng(20261)
    lo, hi = C.limits()
    out = {}
    # link probes
    q_l, box_l, link_l, d_l, ref_l = [], [], [], [], []
    for link in range(10):
        got = tries = 0
        while got < 4:
            tries += 1
            q = lo + (hi - lo) * rng.random(7)
            W = C.world_vertices(q)
            r = slide_probes(C, rng, W[link], [W[o] for o in range(10) if o != link])
            if r is None:
                continue
            got += 1
            for k, d in enumerate(LINK_D):
                q_l.append(q); box_l.append(r[0][k]); link_l.append(link); d_l.append(d)
                ref_l.append(r[1][k])
        print("link", link, "tries", tries, flush=True)
    out.update(link_q=np.array(q_l), link_box=np.array(box_l), link_link=np.array(link_l),
               link_d=np.array(d_l), link_ref=np.array(ref_l))
    # link0 probes: the arm clear of the box
    q_l, box_l, d_l, ref_l = [], [], [], []
    base = C.base_vertices()
    got = tries = 0
    while got < 3:
        tries += 1
        q = lo + (hi - lo) * rng.random(7)
        r = slide_probes(C, rng, base, C.world_vertices(q))
        if r is None:
            continue
        got += 1
        for k, d in enumerate(LINK_D):
            q_l.append(q); box_l.append(r[0][k]); d_l.append(d); ref_l.append(r[1][k])
    print("link0 tries", tries, flush=True)
    out.update(base_q=np.array(q_l), base_box=np.array(box_l), base_d=np.array(d_l),
               base_ref=np.array(ref_l))
    # self probes
    pairs = O.self_pairs()
    out["self_pairs"] = np.array(pairs)
    clear = np.array([0, -np.pi / 4, 0.0, -6 * np.pi / 8, 0, np.pi / 2, np.pi / 4])

    def depths(q, skip=None):
        W = C.world_vertices(q)
        return np.array([-np.inf if (p == skip or C.sphere_bound(W[p[0]], W[p[1]]) < CLEAR)
                         else C.depth(W[p[0]], W[p[1]]) for p in pairs])
    assert depths(clear).max() < CLEAR
    q_l, pair_l, d_l, ref_l = [], [], [], []
    done = set()
    tries = 0
    while len(done) < 5:
        tries += 1
        qb = lo + (hi - lo) * rng.random(7)
        D = depths(qb)
        k = int(D.argmax())
        if D[k] < 0.04 + 5e-3 + 1e-4 or pairs[k] in done:
            continue
        a, b = pairs[k]

        def f(t):
            W = C.world_vertices(clear + t * (qb - clear))
            return C.depth(W[a], W[b])
        # walk back from the deep end to the last point below each target
        grid = np.linspace(1.0, 0.0, 41)
        G = np.array([f(t) for t in grid])
        rows = []
        for d in SELF_D:
            j = int(np.argmax(G < 0.04 + d))
            if j == 0:
                rows = None
                break
            s, fs = solve(lambda s: f(grid[j - 1] - s), 0.0, grid[j - 1] - grid[j], G[j - 1], G[j],
                          0.04 + d)
            q = clear + (grid[j - 1] - s) * (qb - clear)
            if abs(fs - (0.04 + d)) > 1e-9 or (fs >= 0.04) != (d > 0) or \
                    depths(q, skip=pairs[k]).max() >= CLEAR:
                rows = None
                break
            rows.append((q, d, fs))
        if rows is None:
            continue
        done.add(pairs[k])
        for q, d, fs in rows:
            q_l.append(q); pair_l.append(pairs[k]); d_l.append(d); ref_l.append(fs)
        print("self pair", pairs[k], "tries", tries, flush=True)
    out.update(self_q=np.array(q_l), self_pair=np.array(pair_l), self_d=np.array(d_l),
               self_ref=np.array(ref_l))
    path = os.path.join(HERE, "collision_probes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; QJ used", C.QJ_USED[0])
    for fam in ("link", "base", "self"):
        print(fam, len(out[fam + "_d"]), "probes, max |reached - (0.04 + d)| %.3g"
              % np.abs(out[fam + "_ref"] - 0.04 - out[fam + "_d"]).max())


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[2] not in ("model", "probes"):
        sys.exit(__doc__)
    if sys.argv[2] == "model":
        gen_model(sys.argv[1])
    else:
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        gen_probes()
