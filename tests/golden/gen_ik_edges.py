#!/usr/bin/env python3
"""Generate tests/golden/ik_edges.npz: IK at the folds, the shoulder singularity and the edges of
the acceptance band, solved at 50 digits (mpmath).  Dev-time only; the tests read the fixture.

The solver below is the closed form of the Panda's IK with joint 7 fixed, written from the
geometry (csrc/tcmp_ik.h's header comment) over the DH chain of tests/ik_ref.py, with right
angles exact:

  wrist point   frame 7 has frame 8's orientation and O7 = p - d8 z8; one DH step back with the
                given q7 gives R6 and O6 (= O5).  u = O2 - O6, O2 = (0, 0, d1).
  elbow         |O2 - O5|^2 depends on q4 alone and is A + B cos q4 + C sin q4; the three
                coefficients are read off the sub-chain 2..5 at q4 = 0, pi/2, pi.  So
                cos(q4 - psi) = C4 = (|u|^2 - A) / hypot(B, C), psi = atan2(C, B):
                q4 = psi + acos C4 (i4 = 0), psi - acos C4 (i4 = 1).
  joint 6       the z5 component K(q4) of O2 - O5 does not depend on q5; seen from frame 6 it is
                s6 u6x + c6 u6y = r6 sin(q6 + beta), so sin(q6 + beta) = S6 = K / r6:
                q6 = asin S6 - beta (i6 = 0), pi - asin S6 - beta (i6 = 1).
  joint 5       the part of O2 - O5 normal to z5 has the direction w(q4) at q5 = 0 and turns by
                -q5 in frame 5: q5 = angle(w) - angle(u5 in-plane).
  shoulder      R3 = R6 (R_3^6)^T = Rz(q1) Ry(q2) Rz(q3): q2 = atan2(+-sb, R3[2][2]) with
                sb = |R3[0:2, 2]| (i2 = 0: +), q1 = atan2 of +-R3[0:2, 2], and q3 from row 1 of
                Rz(-q1) R3, which is (s3, c3, 0).

Acceptance rule (the contract csrc/tcmp_ik.h and oracle/tcmp_oracle_ik.c implement in fp64):
  * |C4| and |S6| up to 1 + BAND (1e-7, the reference solver's IKFAST_SINCOS_THRESH) are
    clamped to +-1; beyond it the branch does not exist.  At an exact fold both merging
    branches are emitted, so a solution can appear twice.
  * sb <= SHOULDER (1e-12): q1 = 0 and q3 carries q1 + q3.
  * angles in (-pi, pi]; solutions packed in branch order 4*i4 + 2*i6 + i2.

Families (64 cases each, seed 20240611, unpinned joints at least 1e-3 inside the limits; the
generating q7 is the free value):
  G    generic                          W    q6 in (pi + 0.05, 3.70): the solver reports q6 - 2 pi
  F6   q5 = +-pi/2                      F6n  q5 = +-pi/2 +- 10^-k, k = 4..12
  F4   q4 = -phi (full extension)       F4n  q4 = -phi +- 10^-k, k = 4..12
  F46  both folds at once               S    q2 in {0, +-1e-13, +-1e-11, +-1e-9, +-1e-7, +-1e-5}
  Z    exact-zero trig: q1, q3, q7 in {0, +-pi/2}, q2 in {0, +-pi/2} (q1 = 0 where q2 = 0: the
       shoulder convention), q4 = -pi/2, q5 = 0 (+-pi/2 is the joint-6 fold: family F6),
       q6 in {0, pi/2}; then TOP_HOLDING_LEFT_ARM and (0, 0, 0, -pi/2, 0, pi/2, 0)
  B    the band: the first 32 F4 poses moved along O6 - O2 by 1e-9 m (inside: C4 - 1 ~ 6e-9,
       solutions expected) and by 1e-4 m (outside: ~ 6e-4, count 0)
  X    G poses moved 2 m along x: out of reach, count 0

No case is dropped: a draw that fails one of the assertions below means the family's definition
is wrong.  Prints the per-family maxima of the reference's own residual and of its distance from
the generating q.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ik_ref as R  # noqa: E402

mp.mp.dps = 50
BAND = mp.mpf("1e-7")
SHOULDER = mp.mpf("1e-12")
SEED = 20240611
TOP_HOLDING_LEFT_ARM = [0, -np.pi / 4, 0.0, -6 * np.pi / 8, 0, np.pi / 2, np.pi / 4]


def tf(row, theta, exact=True):
    """One DH step (rotation 3x3, translation 3); exact: right angles exact, else the chain's
    fp64 twist values (the pose reference's)."""
    a, d, al = R.DH[row]
    a, d = mp.mpf(a), mp.mpf(d)
    if exact:
        ca, sa = mp.mpf(0) if al else mp.mpf(1), mp.mpf(int(np.sign(al)))
    else:
        ca, sa = mp.cos(mp.mpf(al)), mp.sin(mp.mpf(al))
    c, s = mp.cos(theta), mp.sin(theta)
    return (mp.matrix([[c, -s, 0], [s * ca, c * ca, -sa], [s * sa, c * sa, ca]]),
            mp.matrix([a, -sa * d, ca * d]))


def chain(rows, thetas, exact=True):
    Rm, t = mp.eye(3), mp.matrix([0, 0, 0])
    for row, th in zip(rows, thetas):
        Ri, ti = tf(row, th, exact)
        t = t + Rm * ti
        Rm = Rm * Ri
    return Rm, t


def fk_mp(q):
    """The pose reference's chain at 50 digits (fp64 twist values)."""
    return chain(range(8), [mp.mpf(float(v)) for v in q] + [mp.mpf(0)], exact=False)


def wrap(a):
    while a > mp.pi:
        a -= 2 * mp.pi
    while a <= -mp.pi:
        a += 2 * mp.pi
    return a


def o2_in_frame5(q4):
    """O2 - O5 in frame 5 coordinates at q3 = q5 = 0."""
    Rm, t = chain((2, 3, 4), (0, q4, 0))
    return Rm.T * (-t)


def elbow_coefficients():
    f = [sum(v * v for v in o2_in_frame5(x)) for x in (mp.mpf(0), mp.pi / 2, mp.pi)]
    A = (f[0] + f[2]) / 2
    return A, (f[0] - f[2]) / 2, f[1] - A


A4, B4, C4S = elbow_coefficients()
R4, PSI = mp.hypot(B4, C4S), mp.atan2(C4S, B4)
PHI = -PSI


def clamp_band(x):
    """None outside the band, else x clamped to [-1, 1]."""
    if abs(x) > 1 + BAND:
        return None
    return max(mp.mpf(-1), min(mp.mpf(1), x))


def ik_mp(pose, q7):
    """(solutions in branch order, the fold quantities seen: [C4, S6 per q4 branch])."""
    Rm = mp.matrix(3, 3)
    for i in range(3):
        for j in range(3):
            Rm[i, j] = mp.mpf(float(pose[3 * i + j]))
    p = mp.matrix([mp.mpf(float(v)) for v in pose[9:12]])
    q7 = mp.mpf(float(q7))
    d1, d8 = mp.mpf(R.DH[0][1]), mp.mpf(R.DH[7][1])
    R67, t67 = tf(6, q7)
    R6 = Rm * R67.T
    O6 = p - d8 * Rm[:, 2] - R6 * t67
    u = mp.matrix([0, 0, d1]) - O6
    folds = [(sum(v * v for v in u) - A4) / R4]
    c4 = clamp_band(folds[0])
    sols = []
    if c4 is None:
        return sols, folds
    u6 = R6.T * u
    r6, beta = mp.hypot(u6[0], u6[1]), mp.atan2(u6[1], u6[0])
    for s4 in (1, -1):
        q4 = wrap(PSI + s4 * mp.acos(c4))
        w = o2_in_frame5(q4)
        assert r6 > 0
        folds.append(w[2] / r6)
        s6 = clamp_band(folds[-1])
        if s6 is None:
            continue
        for i6 in (0, 1):
            q6 = wrap(mp.pi - mp.asin(s6) - beta if i6 else mp.asin(s6) - beta)
            R56, _ = tf(5, q6)
            u5 = R56 * u6
            q5 = wrap(mp.atan2(w[1], w[0]) - mp.atan2(u5[1], u5[0]))
            R36, _ = chain((3, 4, 5), (q4, q5, q6))
            R3 = R6 * R36.T
            sb = mp.hypot(R3[0, 2], R3[1, 2])
            for sgn in (1, -1):
                q2 = mp.atan2(sgn * sb, R3[2, 2])
                q1 = mp.atan2(sgn * R3[1, 2], sgn * R3[0, 2]) if sb > SHOULDER else mp.mpf(0)
                c1, s1 = mp.cos(q1), mp.sin(q1)
                q3 = mp.atan2(c1 * R3[1, 0] - s1 * R3[0, 0], c1 * R3[1, 1] - s1 * R3[0, 1])
                sols.append([q1, q2, q3, q4, q5, q6, q7])
    return sols, folds


def residual(sol, pose):
    Rm, t = fk_mp(sol)
    got = [Rm[i, j] for i in range(3) for j in range(3)] + list(t)
    return float(max(abs(g - mp.mpf(float(v))) for g, v in zip(got, pose)))


def solve_case(pose, free):
    """(count, sols (8, 7) fp64, resid (8,), folds)."""
    sols, folds = ik_mp(pose, free)
    out, res = np.zeros((8, 7)), np.zeros(8)
    for k, s in enumerate(sols):
        out[k] = [float(v) for v in s]
        out[k, 6] = free
        res[k] = residual(s[:6] + [mp.mpf(float(free))], pose)
    return len(sols), out, res, folds


# ---- the families -------------------------------------------------------------------------------
def draw(rng):
    return R.LO + 1e-3 + (R.HI - R.LO - 2e-3) * rng.random(7)


def family_q(fam, j, rng, made):
    """Case j of a family (its generating q)."""
    q = draw(rng)
    phi = float(PHI)
    sign = 1.0 if j % 2 == 0 else -1.0
    k = 4 + (j // 4) % 9               # 4..12, each with both signs of the fold and the offset
    off = (1.0 if (j // 2) % 2 == 0 else -1.0) * 10.0 ** -k
    if fam == "W":
        q[5] = np.pi + 0.05 + (3.70 - np.pi - 0.05) * (0.001 + 0.998 * rng.random())
    elif fam == "F6":
        q[4] = sign * np.pi / 2
    elif fam == "F6n":
        q[4] = sign * np.pi / 2 + off
    elif fam == "F4":
        q[3] = -phi
    elif fam == "F4n":
        q[3] = -phi + off
    elif fam == "F46":
        q[4] = sign * np.pi / 2
        q[3] = -phi
    elif fam == "S":
        vals = [0.0] + [s * 10.0 ** -e for e in (13, 11, 9, 7, 5) for s in (1.0, -1.0)]
        q[1] = vals[j % len(vals)]
    elif fam == "Z":
        if j == R.N_PER_FAMILY - 2:
            return np.array(TOP_HOLDING_LEFT_ARM, dtype=np.float64)
        if j == R.N_PER_FAMILY - 1:
            return np.array([0, 0, 0, -np.pi / 2, 0, np.pi / 2, 0])
        tri = (0.0, np.pi / 2, -np.pi / 2)
        q = np.array([tri[rng.integers(3)], tri[rng.integers(3)], tri[rng.integers(3)],
                      -np.pi / 2, 0.0, (0.0, np.pi / 2)[rng.integers(2)], tri[rng.integers(3)]])
        if q[1] == 0.0:
            q[0] = 0.0
    elif fam in ("B", "X"):
        return made["F4" if fam == "B" else "G"][j % 32 if fam == "B" else j].copy()
    return q


def family_pose(fam, j, q):
    T = R.fk_ld(q)
    if fam == "X":
        T[0, 3] += R.LD(2.0)
    if fam == "B":
        # O6 = O7 - a7 x6: along O6 - O2 the pose's position moves, its rotation stays
        T6 = np.eye(4, dtype=R.LD)
        for row in range(6):
            T6 = T6 @ R.tf_ld(row, q[row])
        d = T6[:3, 3] - np.array([0, 0, R.DH[0][1]], dtype=R.LD)
        T[:3, 3] += R.LD(1e-9 if j < 32 else 1e-4) * d / np.sqrt((d * d).sum())
    return R.pose12(T)


PINNED = {"W": [5], "F6": [4], "F6n": [4], "F4": [3], "F4n": [3], "F46": [3, 4], "S": [1],
          "Z": list(range(7)), "B": [3]}


def all_cases():
    """Every case's (family, j, q, pose) in fixture order; cheap (no mpmath)."""
    rng = np.random.default_rng(SEED)
    made, out = {}, []
    for fam in R.FAMILIES:
        made[fam] = []
        for j in range(R.N_PER_FAMILY):
            q = family_q(fam, j, rng, made)
            made[fam].append(q)
            free_j = [i for i in range(7) if i not in PINNED.get(fam, [])]
            assert np.all(q[free_j] >= R.LO[free_j] + 1e-3 - 1e-15), (fam, j)
            assert np.all(q[free_j] <= R.HI[free_j] - 1e-3 + 1e-15), (fam, j)
            assert np.all(q >= R.LO) and np.all(q <= R.HI), (fam, j)
            if fam == "W":
                assert np.pi + 0.05 < q[5] < 3.70
            out.append((fam, j, q, family_pose(fam, j, q)))
    return out


def checked_case(fam, j, q, pose):
    """solve_case plus the conditions the reference alone must meet.  Returns (count, sols,
    resid, distance from q)."""
    n, s, r, folds = solve_case(pose, q[6])
    # every fold quantity at least 10x from the band's edge, on either side
    for x in folds:
        e = abs(x) - 1
        assert e <= BAND / 10 or e >= BAND * 10, (fam, j, float(e))
    if fam == "X" or (fam == "B" and j >= 32):
        assert n == 0, (fam, j, n)
        return n, s, r, 0.0
    assert n > 0, (fam, j)
    miss = R.nearest(s[:n], q)
    if fam in R.FOLD:
        assert miss <= 1e-3, (fam, j, miss)
    else:
        assert miss <= 1e-8, (fam, j, miss)
        assert r[:n].max() <= 1e-9, (fam, j, r[:n].max())
    if fam == "S":   # the shoulder switch is decided the same way in fp64 and here
        sb = abs(np.sin(q[1]))
        assert sb <= float(SHOULDER) / 5 or sb >= float(SHOULDER) * 5, (fam, j)
    return n, s, r, miss


def main():
    cases = all_cases()
    counts, sols, resid = [], [], []
    worst = {fam: [0.0, 0.0] for fam in R.FAMILIES}
    for fam, j, q, pose in cases:
        n, s, r, miss = checked_case(fam, j, q, pose)
        counts.append(n)
        sols.append(s)
        resid.append(r)
        if n:
            worst[fam] = [max(worst[fam][0], r[:n].max()), max(worst[fam][1], miss)]
    print("%-4s %5s %12s %12s" % ("fam", "n", "max resid", "max miss"))
    for fam in R.FAMILIES:
        print("%-4s %5d %12.3e %12.3e" % (fam, R.N_PER_FAMILY, worst[fam][0], worst[fam][1]))
    out = os.path.join(HERE, "ik_edges.npz")
    np.savez_compressed(out,
                        family=np.array([R.FAMILIES.index(c[0]) for c in cases], dtype=np.int8),
                        q=np.array([c[2] for c in cases]), pose=np.array([c[3] for c in cases]),
                        free=np.array([c[2][6] for c in cases]),
                        count=np.array(counts, dtype=np.int32), sols=np.array(sols),
                        resid=np.array(resid))
    print("wrote %s (%d cases, %d bytes)" % (out, len(cases), os.path.getsize(out)))


if __name__ == "__main__":
    main()
