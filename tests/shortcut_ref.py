"""Restatement of the force-aware shortcut pass (include/tcmp.h tcmp_shortcut_path), the
reference of tests/test_shortcut_host.py and tests/test_gpu_shortcut.py.  Nothing here imports
the package: chord checks come from the CPU oracle (oracle.check_edge), distances are orc_dist
restated in scalar fp64 in its loop order, the dynamic program and the splice are plain loops.
The extend resolutions and the distance weights w are parameters; left out they are the
planner's 0.1 and 10.

One pass over W[0..n-1]:
  anchors  a_k = min(k s, n - 1), s = 1 if n <= A_max else ceil((n - 1) / (A_max - 1)),
           k = 0 .. A - 1, A = ceil((n - 1) / s) + 1
  orig[k]  sum of dist(W[t], W[t+1]) for t = a_k .. a_{k+1} - 1, left to right
  chords   (k, l), k < l, a_l - a_k >= 2; valid iff n_safe == n_steps and
           dist(W[a_l], last) < 1e-6; length dist(W[a_k], W[a_l])
  DP       cost[0] = 0; best = cost[l-1] + orig[l-1]; k ascending, strict <
  splice   original hops copied; a chord's n_steps - 1 refine points, then W[a_l] itself
Passes stop after one that used no chord.
"""
import numpy as np

W10 = (10.0,) * 7


def dist(a, b, w=W10):
    """sqrt(sum_k w_k * (d_k * d_k)), k = 0..6 in order, no contraction (orc_dist)."""
    s = np.float64(0.0)
    for k in range(7):
        d = np.float64(b[k]) - np.float64(a[k])
        s = s + np.float64(w[k]) * (d * d)
    return float(np.sqrt(s))


def anchors(n, a_max):
    s = 1 if n <= a_max else -(-(n - 1) // (a_max - 1))
    A = -(-(n - 1) // s) + 1
    return [min(k * s, n - 1) for k in range(A)], s


def extend_points(a, b, n_steps):
    """The first n_steps - 1 points of extend(a, b) (utils.py:3031-3041 refine, n_steps steps)."""
    q = np.array(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    out = []
    for i in range(n_steps - 1):
        r = np.float64(1.0) / np.float64(n_steps - i)
        q = r * (b - q) + q
        out.append(q.copy())
    return out


def dp(orig, chords):
    """orig[k]: cost of the original hop k -> k + 1 (A - 1 of them); chords: {(k, l): length} of
    the valid ones.  -> (cost list, predecessor list: -1 = the original hop, else k)."""
    A = len(orig) + 1
    cost = [0.0] * A
    pred = [-1] * A
    for l in range(1, A):
        best = cost[l - 1] + orig[l - 1]
        p = -1
        for k in range(l):
            if (k, l) in chords and cost[k] + chords[(k, l)] < best:
                best = cost[k] + chords[(k, l)]
                p = k
        cost[l] = best
        pred[l] = p
    return cost, pred


def hops(pred):
    """Start-to-goal hops (k, l, is_chord) of the predecessor walk back from the last anchor."""
    out = []
    l = len(pred) - 1
    while l > 0:
        if pred[l] < 0:
            out.append((l - 1, l, False))
            l -= 1
        else:
            out.append((pred[l], l, True))
            l = pred[l]
    return out[::-1]


def splice(W, anc, hop_list, n_steps_of):
    new = [np.array(W[0], dtype=np.float64)]
    for k, l, is_chord in hop_list:
        if is_chord:
            new.extend(extend_points(W[anc[k]], W[anc[l]], n_steps_of[(k, l)]))
            new.append(np.array(W[anc[l]], dtype=np.float64))
        else:
            for t in range(anc[k] + 1, anc[l] + 1):
                new.append(np.array(W[t], dtype=np.float64))
    return np.array(new).reshape(-1, 7)


def one_pass(W, check, a_max, w=W10):
    """check(a, b) -> (n_safe, n_steps, last).  -> (new list, stats of the pass)."""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 7)
    n = len(W)
    anc, _ = anchors(n, a_max)
    A = len(anc)
    orig = []
    for k in range(A - 1):
        acc = 0.0
        for t in range(anc[k], anc[k + 1]):
            acc = acc + dist(W[t], W[t + 1], w)
        orig.append(acc)
    valid, n_steps_of = {}, {}
    tested = steps = 0
    for l in range(A):
        for k in range(l):
            if anc[l] - anc[k] < 2:
                continue
            tested += 1
            ns, nt, last = check(W[anc[k]], W[anc[l]])
            steps += nt if ns == nt else ns + 1
            if ns == nt and dist(W[anc[l]], last, w) < 1e-6:
                valid[(k, l)] = dist(W[anc[k]], W[anc[l]], w)
                n_steps_of[(k, l)] = nt
    cost, pred = dp(orig, valid)
    hl = hops(pred)
    new = splice(W, anc, hl, n_steps_of)
    before = 0.0
    for o in orig:
        before = before + o
    return new, dict(n_anchors=A, tested=tested, valid=len(valid),
                     used=sum(1 for h in hl if h[2]), steps=steps, hops=len(hl),
                     cost_before=before, cost_after=cost[A - 1])


def shortcut(W, check, a_max=512, passes=1, w=W10):
    W = np.asarray(W, dtype=np.float64).reshape(-1, 7)
    tot = dict(passes_run=0, n_before=len(W), chords_tested=0, chords_valid=0, chords_used=0,
               chord_steps=0, max_hops=0)
    for p in range(passes):
        W, st = one_pass(W, check, a_max, w)
        if p == 0:
            tot["n_anchors"] = st["n_anchors"]
            tot["cost_before"] = st["cost_before"]
        tot["passes_run"] = p + 1
        tot["cost_after"] = st["cost_after"]
        tot["chords_tested"] += st["tested"]
        tot["chords_valid"] += st["valid"]
        tot["chords_used"] += st["used"]
        tot["chord_steps"] += st["steps"]
        tot["max_hops"] = max(tot["max_hops"], st["hops"])
        if st["used"] == 0:
            break
    tot["n_after"] = len(W)
    return W, tot


def oracle_check(O, obs, mode, mass, resolutions=None):
    """check(a, b) through the CPU oracle's check_edge (Gauss-map exact test, cull=2)."""
    def check(a, b):
        return O.check_edge(a, b, obs, mode, mass, cull=2, resolutions=resolutions)
    return check


def path_cost(W, w=W10):
    c = 0.0
    for t in range(len(W) - 1):
        c = c + dist(W[t], W[t + 1], w)
    return c


def zigzag(O, rng, n, obs, mode, mass, lo, hi, step=0.9, verts=False, free=False,
           resolutions=None):
    """A polyline of n points: zig-zag vertices at most `step` apart per joint, joined by the
    extend rule's points (verts: the vertices alone).  Every vertex is collision-free and within
    the torque limits and every hop's edge is safe, so the original hops are valid edges --
    unless free: then the vertices are unconstrained draws."""
    def ok(q):
        return not O.collision(q, obs, cull=2) and O.torque_ok(q, mode, mass)
    while True:
        v = lo + (hi - lo) * rng.random(7)
        if free or ok(v):
            break
    pts = [v]
    while len(pts) < n:
        for _ in range(2000):
            nv = np.clip(v + rng.uniform(-step, step, 7), lo, hi)
            ns, nt, _ = O.check_edge(v, nv, obs, mode, mass, cull=2, resolutions=resolutions)
            if free or ns == nt:
                break
        else:
            raise RuntimeError("no valid hop found")
        if not verts:
            pts.extend(extend_points(v, nv, nt))
        pts.append(nv)
        v = nv
    return np.array(pts[:n]).reshape(-1, 7)
