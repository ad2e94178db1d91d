"""What the IK edge tests share (tests/test_ik_edges_host.py, tests/test_gpu_ik_edges.py and the
fixture's generator tests/golden/gen_ik_edges.py): the pose reference in numpy.longdouble, the
fixture's layout and the comparisons.  Plain numpy; nothing here loads a library.

Pose reference: fk_ld is the DH chain of rne.py:47-54 (get_tf_mat, rows 0..7; the twist angles
are the fp64 values +-np.pi/2 the reference writes) evaluated in numpy.longdouble.  Every pose a
test computes at run time goes through it; tests/test_ik_edges_host.py checks it once against
fk_golden.npz.

Fixture tests/golden/ik_edges.npz (written by gen_ik_edges.py), n cases in family order:
  family (n,) index into FAMILIES      q (n, 7) the generating configuration
  pose (n, 12) fp64: fk_ld(q) rounded (families B and X: then moved), R row-major then p
  free (n,) the free value (q[6])      count (n,) the reference's number of solutions
  sols (n, 8, 7) the reference's solutions packed in branch order 4*i4 + 2*i6 + i2
  resid (n, 8) the reference's own pose residual per solution (at 50 digits)
"""
import os

import numpy as np

LD = np.longdouble
PI = np.pi
FAMILIES = ("G", "W", "F6", "F6n", "F4", "F4n", "F46", "S", "Z", "B", "X")
N_PER_FAMILY = 64
FOLD = ("F6", "F6n", "F4", "F4n", "F46", "B")   # soundness by the reference's residual
PARITY = ("G", "W", "Z")                        # slot-by-slot comparison is well conditioned
SHOULDER_BAND = 1e-7                            # |q2| up to here: only q1 + q3 is compared

LO = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
HI = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])

# rne.py:47-54: (a, d, alpha) per row; theta = q_i, row 7 (the flange) theta = 0
DH = ((0.0, 0.333, 0.0), (0.0, 0.0, -PI / 2), (0.0, 0.316, PI / 2), (0.0825, 0.0, PI / 2),
      (-0.0825, 0.384, -PI / 2), (0.0, 0.0, PI / 2), (0.088, 0.0, PI / 2), (0.0, 0.107, 0.0))


def tf_ld(row, theta):
    """get_tf_mat (rne.py:32-44) in longdouble."""
    a, d, al = (LD(v) for v in DH[row])
    q = LD(theta)
    c, s, ca, sa = np.cos(q), np.sin(q), np.cos(al), np.sin(al)
    z, one = LD(0), LD(1)
    return np.array([[c, -s, z, a],
                     [s * ca, c * ca, -sa, -sa * d],
                     [s * sa, c * sa, ca, ca * d],
                     [z, z, z, one]], dtype=LD)


def fk_ld(q):
    """T_0^8 (4, 4) longdouble of q (7,)."""
    T = np.eye(4, dtype=LD)
    for row in range(8):
        T = T @ tf_ld(row, q[row] if row < 7 else 0.0)
    return T


def pose12(T):
    """(4, 4) -> the (12,) fp64 row tcmp_ik takes: R row-major, p."""
    T = np.asarray(T)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(np.float64)


def pose44(row):
    T = np.eye(4)
    T[:3, :3] = np.asarray(row[:9]).reshape(3, 3)
    T[:3, 3] = row[9:12]
    return T


def pose_err(q, row):
    """max |fk_ld(q) - pose| over the 12 entries, as a float."""
    T = fk_ld(q)
    d = np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]) - np.asarray(row, dtype=LD)
    return float(np.abs(d).max())


def ang_dist(a, b):
    """|a - b| mod 2 pi, elementwise, in [0, pi]."""
    d = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64) + PI) % (2 * PI) - PI
    return np.abs(d)


def shoulder_dist(sol, q):
    """Joint-space distance of a solution from q (max over joints, mod 2 pi).  Where
    |q[1]| <= SHOULDER_BAND joints 1 and 3 turn about (nearly) the same axis and only their sum
    is determined: q1 + q3 is compared in their place."""
    sol = np.asarray(sol, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    if abs(q[1]) <= SHOULDER_BAND:
        rest = ang_dist(sol[[1, 3, 4, 5, 6]], q[[1, 3, 4, 5, 6]]).max()
        return float(max(rest, ang_dist(sol[0] + sol[2], q[0] + q[2])))
    return float(ang_dist(sol, q).max())


def nearest(sols, q):
    """The smallest shoulder_dist of a solution set from q; inf for an empty set."""
    return min((shoulder_dist(s, q) for s in sols), default=float("inf"))


def pair_sets(A, B):
    """Pair two solution sets (k, 7) one to one, closest pairs first; the largest paired distance
    (mod 2 pi, max over joints).  inf when the sizes differ."""
    A = np.asarray(A, dtype=np.float64).reshape(-1, 7)
    B = np.asarray(B, dtype=np.float64).reshape(-1, 7)
    if len(A) != len(B):
        return float("inf")
    if not len(A):
        return 0.0
    D = np.array([[ang_dist(a, b).max() for b in B] for a in A])
    worst = 0.0
    for _ in range(len(A)):
        i, j = np.unravel_index(np.argmin(D), D.shape)
        worst = max(worst, float(D[i, j]))
        D[i, :] = np.inf
        D[:, j] = np.inf
    return worst


def just_outside(sols):
    """How many solutions sit outside the joint limits by at most 1e-8 (a generating joint
    exactly on its limit; reported, never asserted)."""
    s = np.asarray(sols, dtype=np.float64).reshape(-1, 7)
    inside = ((s >= LO) & (s <= HI)).all(axis=1)
    near = ((s >= LO - 1e-8) & (s <= HI + 1e-8)).all(axis=1)
    return int((near & ~inside).sum())


class Fixture:
    """ik_edges.npz, with the per-family views the tests use."""

    def __init__(self, path=None):
        if path is None:
            path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "ik_edges.npz")
        z = np.load(path)
        for k in ("family", "q", "pose", "free", "count", "sols", "resid"):
            setattr(self, k, z[k])
        self.n = len(self.q)
        self.names = [FAMILIES[f] for f in self.family]

    def rows(self, fam):
        return [i for i in range(self.n) if self.names[i] == fam]

    def family_resid(self, fam):
        """The largest reference residual over the family's solutions."""
        r = [self.resid[i, :self.count[i]].max() for i in self.rows(fam) if self.count[i]]
        return float(max(r)) if r else 0.0

    def sound_bound(self, fam):
        """Assertion 2's bound: 1e-9, or for the fold families twice the reference's own
        residual (the clamp moves the pose) plus 1e-9."""
        return 2.0 * self.family_resid(fam) + 1e-9 if fam in FOLD else 1e-9

    def complete_bound(self, fam):
        """Assertion 3's bound: present or absent (1e-2 rad) at a fold, else 1e-8."""
        return 1e-2 if fam in FOLD else 1e-8


def check_case(fx, i, sols, cnt):
    """Assertions 1-4 on one case: sols (8, 7), cnt from the solver under test.  Returns
    (pose residual, distance from the generating q) for the caller's report."""
    fam = fx.names[i]
    assert cnt == fx.count[i], (fam, i, int(cnt), int(fx.count[i]))
    if cnt == 0:
        return 0.0, 0.0
    got = np.asarray(sols)[:cnt]
    res = max(pose_err(s, fx.pose[i]) for s in got)
    assert res <= fx.sound_bound(fam), (fam, i, res, fx.sound_bound(fam))
    assert np.all(np.abs(got[:, :6]) <= PI) and np.all(got[:, 6] == fx.free[i]), (fam, i)
    miss = nearest(got, fx.q[i])
    assert miss <= fx.complete_bound(fam), (fam, i, miss)
    if fam in PARITY:
        d = ang_dist(got, fx.sols[i, :cnt]).max()
        assert d <= 1e-9, (fam, i, d)
    return res, miss
