"""The torque test in high precision, and what the torque-limit tests share (tests/
test_torque_limits_host.py, tests/test_gpu_torque_limits.py and the fixture's generator tests/
golden/gen_torque_limits.py).  Plain numpy (mpmath for the 50-digit cross-check); nothing here
loads a library, and nothing is shared with oracle/tcmp_oracle.c or the kernels: the model
numbers below are this file's own copy.

rne_hp restates rne(q, qd, qdd) of the reference (rne.py:198-252) body by body in 6-vectors
ordered (linear, angular) as the reference writes them: the DH rows of rne.py:47-54 with the twist
angles the fp64 values +-np.pi/2, q taken as the exact fp64 value, link 7's quirk (rne.py:226-227)
and the payload body of add_payload (rne.py:181-188: mass m at the frame of the hand, centre of
mass 0, inertia new_inertia([0, 0, 0.14 + 0.025], m)).  A body of mass 0 and inertia 0 adds exact
zeros, so "no payload" is the payload body at mass 0.

The three decision rules (panda_primitives.py:13-16, 60-116, 118-193):
  nov (mode 1)  rne(q, 0, 0), the payload body only when mass > 0.01
  rne (mode 2)  rne(q, qd, qdd), the payload body only when mass > 0.01
  dyn (mode 3)  rne(q, qd, qdd) without payload + J^T [0, 0, m g, 0, 0, 0] at panda_grasptarget,
                no mass threshold.  The reference takes M, C and g from panda_dynamics_model,
                which it does not ship: as everywhere in this project they are rne.py's, so the
                Jacobian term has no reference vector (unpinned against pdm).  J's linear z row is
                (z_i x (p_target - o_i))_z over the URDF joint frames (panda_mod.urdf:121-294,
                grasp target 0.105 above the hand, :87-91); the host test checks it against a
                finite difference of target_z, this file's own FK.
  joints 1..6 fail with `>=`; joint 7 is never tested.

Every function takes rows: q, qd, qdd (n, 7) fp64 and mass (n,), and a number context: LDC
(numpy.longdouble) or mpc(digits) (object arrays of mpmath.mpf).
"""
import os

import numpy as np

LD = np.longdouble
PI = np.pi
MODE_BASE, MODE_NOV, MODE_RNE, MODE_DYN = 0, 1, 2, 3
EFFORT = (87.0, 87.0, 87.0, 87.0, 12.0, 12.0, 12.0)   # panda_mod.urdf joint limits, effort
N_TESTED = 6                                           # range(len(max_limits) - 1)
PAYLOAD_MIN = 0.01                                     # panda_primitives.py:142, 178
GRAV = 9.81                                            # rne.py:199
PAYLOAD_R = 0.14 + 0.025                               # rne.py:182, 187, as the reference adds them
CLEAR = 0.5                                            # Nm: every non-deciding comparison
LO = np.array([-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973])
HI = np.array([2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973])

# rne.py:47-54: (a, d, alpha); theta = q_i, row 7 (the flange) theta = 0
DH = ((0.0, 0.333, 0.0), (0.0, 0.0, -PI / 2), (0.0, 0.316, PI / 2), (0.0825, 0.0, PI / 2),
      (-0.0825, 0.384, -PI / 2), (0.0, 0.0, PI / 2), (0.088, 0.0, PI / 2), (0.0, 0.107, 0.0))
# rne.py:125-136, bodies 1..9 (7 links, the massless flange, the hand); body 10 is the payload
MASS = (4.970684, 0.646926, 3.228604, 3.587895, 1.225946, 1.666555, 7.35522e-01, 0.0, 0.68)
# rne.py:107-118
COM = ((3.875e-03, 2.081e-03, -0.1750), (-3.141e-03, -2.872e-02, 3.495e-03),
       (2.7518e-02, 3.9252e-02, -6.6502e-02), (-5.317e-02, 1.04419e-01, 2.7454e-02),
       (-1.1953e-02, 4.1065e-02, -3.8437e-02), (6.0149e-02, -1.4117e-02, -1.0517e-02),
       (1.0517e-02, -4.252e-03, 6.1597e-02), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
# rne.py:65-75: ixx, ixy, ixz, iyy, iyz, izz
INERTIA = ((7.0337e-01, -1.3900e-04, 6.7720e-03, 7.0661e-01, 1.9169e-02, 9.1170e-03),
           (7.9620e-03, -3.9250e-03, 1.0254e-02, 2.8110e-02, 7.0400e-04, 2.5995e-02),
           (3.7242e-02, -4.7610e-03, -1.1396e-02, 3.6155e-02, -1.2805e-02, 1.0830e-02),
           (2.5853e-02, 7.7960e-03, -1.3320e-03, 1.9552e-02, 8.6410e-03, 2.8323e-02),
           (3.5549e-02, -2.1170e-03, -4.0370e-03, 2.9474e-02, 2.2900e-04, 8.6270e-03),
           (1.9640e-03, 1.0900e-04, -1.1580e-03, 4.3540e-03, 3.4100e-04, 5.4330e-03),
           (1.2516e-02, -4.2800e-04, -1.1960e-03, 1.0027e-02, -7.4100e-04, 4.8150e-03),
           (0.001, 0.0, 0.0, 0.001, 0.0, 0.001),
           (0.1, 0.0, 0.0, 0.1, 0.0, 0.1))
# panda_mod.urdf joint1..7 origins: xyz and the roll of rpy (the URDF's own 11 decimals)
URDF_XYZ = ((0.0, 0.0, 0.333), (0.0, 0.0, 0.0), (0.0, -0.316, 0.0), (0.0825, 0.0, 0.0),
            (-0.0825, 0.384, 0.0), (0.0, 0.0, 0.0), (0.088, 0.0, 0.0))
URDF_ROLL = (0.0, -1.57079632679, 1.57079632679, 1.57079632679, -1.57079632679, 1.57079632679,
             1.57079632679)
URDF_FLANGE_Z, URDF_TARGET_Z = 0.107, 0.105            # joint8 (:294), grasptarget_hand (:90)


# ---- number contexts ---------------------------------------------------------------------------
class _LongDouble:
    name = "longdouble"

    @staticmethod
    def conv(x):
        a = np.asarray(x)
        return a if a.dtype == LD else a.astype(np.float64).astype(LD)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape, dtype=LD)

    sin = staticmethod(np.sin)
    cos = staticmethod(np.cos)

    @staticmethod
    def num(x):
        return LD(float(x))


LDC = _LongDouble()


def mpc(digits=50):
    """The same arithmetic on object arrays of mpmath.mpf at `digits` decimal digits."""
    import mpmath

    mpmath.mp.dps = digits
    mpf = mpmath.mpf

    class _Mp:
        name = "mpmath%d" % digits
        conv = staticmethod(np.frompyfunc(lambda v: mpf(float(v)), 1, 1))
        sin = staticmethod(np.frompyfunc(mpmath.sin, 1, 1))
        cos = staticmethod(np.frompyfunc(mpmath.cos, 1, 1))

        @staticmethod
        def zeros(shape):
            a = np.empty(shape, dtype=object)
            a.fill(mpf(0))
            return a

        @staticmethod
        def num(x):
            return mpf(float(x))

    c = _Mp()
    c.conv = lambda x: _Mp.conv(np.asarray(x, dtype=np.float64)).astype(object)
    return c


# ---- 6-vector algebra on rows (rne.py:4-27) -----------------------------------------------------
def _skew(cx, v):
    """(n, 3) -> (n, 3, 3), rne.py:4-7."""
    S = cx.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1] = -v[..., 2]
    S[..., 0, 2] = v[..., 1]
    S[..., 1, 0] = v[..., 2]
    S[..., 1, 2] = -v[..., 0]
    S[..., 2, 0] = -v[..., 1]
    S[..., 2, 1] = v[..., 0]
    return S


def _mv(M, v):
    return np.matmul(M, v[..., None])[..., 0]


def _mtv(M, v):
    return np.matmul(np.swapaxes(M, -1, -2), v[..., None])[..., 0]


def _adjoint(cx, R, t):
    """rne.py:9-14: [[R, skew(t) R], [0, R]]."""
    A = cx.zeros(R.shape[:-2] + (6, 6))
    A[..., :3, :3] = R
    A[..., 3:, 3:] = R
    A[..., :3, 3:] = np.matmul(_skew(cx, t), R)
    return A


def _crm(cx, v):
    """rne.py:21-24."""
    M = cx.zeros(v.shape[:-1] + (6, 6))
    W = _skew(cx, v[..., 3:])
    M[..., :3, :3] = W
    M[..., :3, 3:] = _skew(cx, v[..., :3])
    M[..., 3:, 3:] = W
    return M


def _spatial_inertia(cx, m, c, I6):
    """rne.py:16-19 for one body of constant numbers -> (6, 6)."""
    m = cx.num(m)
    cv = cx.zeros((3,))
    for k in range(3):
        cv[k] = cx.num(c[k])
    C = _skew(cx, cv)
    I3 = cx.zeros((3, 3))
    for (r, k), x in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), I6):
        I3[r, k] = I3[k, r] = cx.num(x)
    M = cx.zeros((6, 6))
    for k in range(3):
        M[k, k] = m
    M[:3, 3:] = m * C.T
    M[3:, :3] = m * C
    M[3:, 3:] = I3 + m * np.matmul(C, C.T)
    return M


def _xup(cx, row, theta, n):
    """get_parent_to_child_transform(q, row, row + 1) (rne.py:46-63): the inverse of DH row
    `row`, identity past the flange -> (R (n, 3, 3), t (n, 3))."""
    R = cx.zeros((n, 3, 3))
    t = cx.zeros((n, 3))
    if row >= 8:
        for k in range(3):
            R[:, k, k] = cx.num(1.0)
        return R, t
    a, d, al = (cx.num(v) for v in DH[row])
    al1 = cx.conv(np.array([DH[row][2]]))
    ca, sa = cx.cos(al1)[0], cx.sin(al1)[0]
    c, s = cx.cos(theta), cx.sin(theta)
    T = cx.zeros((n, 3, 3))                  # get_tf_mat's rotation (rne.py:39-41)
    T[:, 0, 0] = c
    T[:, 0, 1] = -s
    T[:, 1, 0] = s * ca
    T[:, 1, 1] = c * ca
    T[:, 1, 2] = -sa
    T[:, 2, 0] = s * sa
    T[:, 2, 1] = c * sa
    T[:, 2, 2] = ca
    p = cx.zeros((n, 3))
    p[:, 0] = a
    p[:, 1] = -sa * d
    p[:, 2] = ca * d
    R = np.swapaxes(T, -1, -2).copy()
    t = -_mv(R, p)
    return R, t


def rne_hp(q, qd, qdd, payload, cx=LDC):
    """rne(q, qd, qdd) with the payload body at mass payload (n,) (0: none) -> (n, 7) in cx."""
    q = cx.conv(np.atleast_2d(q))
    qd = cx.conv(np.atleast_2d(qd))
    qdd = cx.conv(np.atleast_2d(qdd))
    n = len(q)
    mp = cx.conv(np.broadcast_to(np.asarray(payload, dtype=np.float64), (n,)))
    zero = cx.zeros((n,))
    Ad, v, a, f = [], [], [], []
    unit = cx.zeros((6, 6))                  # the payload body per kg (rne.py:85-100, 187)
    r2 = cx.num(PAYLOAD_R) * cx.num(PAYLOAD_R)
    for k in range(3):
        unit[k, k] = cx.num(1.0)
    unit[3, 3] = unit[4, 4] = r2
    for i in range(1, 11):
        b = i - 1
        R, t = _xup(cx, b, q[:, b] if b < 7 else zero, n)
        if i == 7:
            t[:, 2] = zero                   # rne.py:226-227
        A = _adjoint(cx, R, t)
        vJ = cx.zeros((n, 6))
        acc = cx.zeros((n, 6))
        if b < 7:
            vJ[:, 5] = qd[:, b]
            acc[:, 5] = qdd[:, b]
        if i == 1:
            g = cx.zeros((n, 6))
            g[:, 2] = cx.num(GRAV)           # -a_grav
            vi = vJ
            ai = _mv(A, g) + acc
        else:
            vi = _mv(A, v[-1]) + vJ
            ai = _mv(A, a[-1]) + acc + _mv(_crm(cx, vi), vJ)
        if b < 9:
            M = _spatial_inertia(cx, MASS[b], COM[b], INERTIA[b])
        else:
            M = mp[:, None, None] * unit
        fi = _mv(M, ai) - _mtv(_crm(cx, vi), _mv(M, vi))    # I a + crf(v) I v, crf = -crm^T
        Ad.append(A); v.append(vi); a.append(ai); f.append(fi)
    tau = cx.zeros((n, 10))
    for i in range(10, 0, -1):               # rne.py:247-251
        b = i - 1
        tau[:, b] = f[b][:, 5]
        if i != 1:
            f[b - 1] = f[b - 1] + _mtv(Ad[b], f[b])
    return tau[:, :7]


# ---- dyn's force term over the URDF frames -------------------------------------------------------
def urdf_frames(q, cx=LDC):
    """(z (n, 7, 3) joint axes, o (n, 7, 3) joint frame origins, target (n, 3)): the URDF chain
    Rx(roll_j) Rz(q_j) after each joint origin; the grasp target 0.107 + 0.105 along link 7's z."""
    q = cx.conv(np.atleast_2d(q))
    n = len(q)
    R = cx.zeros((n, 3, 3))
    for k in range(3):
        R[:, k, k] = cx.num(1.0)
    p = cx.zeros((n, 3))
    z, o = cx.zeros((n, 7, 3)), cx.zeros((n, 7, 3))
    for j in range(7):
        roll = cx.conv(np.array([URDF_ROLL[j]]))
        cr, sr = cx.cos(roll)[0], cx.sin(roll)[0]
        c, s = cx.cos(q[:, j]), cx.sin(q[:, j])
        L = cx.zeros((n, 3, 3))
        L[:, 0, 0] = c
        L[:, 0, 1] = -s
        L[:, 1, 0] = cr * s
        L[:, 1, 1] = cr * c
        L[:, 1, 2] = -sr
        L[:, 2, 0] = sr * s
        L[:, 2, 1] = sr * c
        L[:, 2, 2] = cr
        xyz = cx.zeros((n, 3))
        for k in range(3):
            xyz[:, k] = cx.num(URDF_XYZ[j][k])
        p = _mv(R, xyz) + p
        R = np.matmul(R, L)
        z[:, j] = R[:, :, 2]
        o[:, j] = p
    target = p + R[:, :, 2] * (cx.num(URDF_FLANGE_Z) + cx.num(URDF_TARGET_Z))
    return z, o, target


def target_z(q, cx=LDC):
    """The grasp target's height (n,): what the host test differentiates."""
    return urdf_frames(q, cx)[2][:, 2]


def dyn_force_term(q, mass, cx=LDC):
    """J^T [0, 0, m g, 0, 0, 0] (n, 7): m g (z_i x (target - o_i))_z."""
    z, o, target = urdf_frames(q, cx)
    n = len(z)
    m = cx.conv(np.broadcast_to(np.asarray(mass, dtype=np.float64), (n,)))
    r = target[:, None, :] - o
    return (m * cx.num(GRAV))[:, None] * (z[:, :, 0] * r[:, :, 1] - z[:, :, 1] * r[:, :, 0])


# ---- the decision rules --------------------------------------------------------------------------
def mode_torques(q, qd, qdd, mode, mass, cx=LDC):
    """The seven torques the test of `mode` (n,) compares, rows of mixed modes and masses."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float64))
    n = len(q)
    mode = np.broadcast_to(np.asarray(mode), (n,))
    mass = np.broadcast_to(np.asarray(mass, dtype=np.float64), (n,))
    qd = np.zeros_like(q) if qd is None else np.atleast_2d(np.asarray(qd, dtype=np.float64))
    qdd = np.zeros_like(q) if qdd is None else np.atleast_2d(np.asarray(qdd, dtype=np.float64))
    rates = (mode != MODE_NOV)[:, None]
    body = np.where((mode != MODE_DYN) & (mass > PAYLOAD_MIN), mass, 0.0)
    tau = rne_hp(q, np.where(rates, qd, 0.0), np.where(rates, qdd, 0.0), body, cx)
    if (mode == MODE_DYN).any():
        tau = tau + dyn_force_term(q, np.where(mode == MODE_DYN, mass, 0.0), cx)
    return tau


def margins(tau):
    """|tau_j| - L_j over the six tested joints (n, 6), in tau's own precision."""
    return np.abs(tau[:, :N_TESTED]) - np.array(EFFORT[:N_TESTED])


def decide(tau):
    """True = the row passes: no tested joint with |tau| >= L."""
    return ~(margins(tau) >= 0).any(axis=1)


def f64(a):
    return np.asarray(a, dtype=np.float64) if a.dtype != object else \
        np.array([float(x) for x in a.flat]).reshape(a.shape)


# ---- the fixture -----------------------------------------------------------------------------------
FAMILIES = ("static", "static_j1", "dynamic", "dyn_static", "dyn_dynamic", "threshold_rne",
            "threshold_dyn", "joint7")
PROBES = ("static", "dynamic", "dyn_static", "dyn_dynamic")     # families of (side, level) variants
STATIC = ("static", "static_j1")                                # nov rows that run as rne too
BASE_KEYS = ("b_family", "b_q", "b_qd", "b_qdd", "b_mode", "b_mass", "b_joint", "b_sign", "b_var",
             "b_x", "b_margin")
EDGE_KEYS = ("e_mode", "e_joint", "e_kpos", "e_a", "e_b", "e_k", "e_sign", "e_xa", "e_xb", "e_margin",
             "e_clear_before", "e_clear_after", "e_mass")
GOAL_KEYS = ("g_base", "g_x", "g_margin")
REWIRE_KEYS = ("r_a", "r_goal", "r_uC", "r_uS", "r_margin", "r_mode", "r_mass", "r_joint", "r_k",
               "r_radius", "r_parent")
SCALAR_KEYS = ("levels", "j3_payload", "j4_payload", "oracle_dev", "band", "delta_min",
               "ref_uncertainty")
# Nm inside asked of every other step of an edge, and of its start, when the probe is the first
# or a middle step (the last step: CLEAR, all of them).  A step moves the arm by less than 0.1
# rad, so a torque that rises 0.5 Nm into its limit over one step and falls 0.5 Nm over the next
# needs |d2 tau / ds2| >= 100 Nm/rad2 along the edge; a search of a million edges through
# near-limit configurations found one.  The probe step is made the peak of the edge's profile
# instead, and its neighbours clear it by what the curvature gives: still 5e8 times delta_min and
# four orders above an fp32 rounding of 87 Nm, so every decision stays exact.
EDGE_CLEAR_PEAK = 0.05


def fixture_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "torque_limits.npz")


class Fixture:
    """torque_limits.npz (written by gen_torque_limits.py), expanded into rows and edges.

    Stored, one entry per base: b_family (index into FAMILIES), b_q, b_qd, b_qdd (7 each), b_mode,
    b_mass, b_joint (the deciding joint, 0-based), b_sign (of its torque), b_var (the scalar x:
    >= 0 the angle of that joint, -1 a factor on b_qdd, -2 none), b_x and b_margin (one column
    per variant (side, level), levels outermost, side +1 then -1; NaN where a family has fewer).
    Per edge base: e_a, e_b, e_mode, e_mass, e_joint, e_sign, e_k (the probe's step), e_kpos
    (0 first, 1 middle, 2 last), e_xa, e_xb (both ends' angle e_joint per variant: the edge
    shifted along that joint), e_margin,
    e_clear_before / e_clear_after (Nm inside of the other steps).  Scalars: levels, oracle_dev,
    band (64 oracle_dev), delta_min, ref_uncertainty, j3_payload, j4_payload.
    g_base, g_x, g_margin: the static bases of families 1 and 3 at a further level, 1e-3 Nm
    (columns: fails, passes), for tcmp_goal_search.  r_*: the rewire case (gen_torque_limits.
    rewire_case): start r_a, goal r_goal, the uniform draws r_uC and r_uS (one row per variant:
    fails, passes) of rounds 2 and 3, r_parent the new node's expected parent per variant.

    Rows (n): family, base, q, qd, qdd, mode, mass, joint, sign, side (+1 fails, -1 passes, 0 no
    probe), delta, margin (|tau_j| - L_j in the reference; NaN where not recorded), ok.
      threshold_*: two rows per base, the passing mass (rne 0.01, dyn 0) then the failing one.
      joint7: three rows per base: nov, rne, dyn.
    Edges (m): ea, eb, emode, emass, ejoint, ek, ekpos, eside, edelta, emargin, steps (list of
    (nsteps, 7): the reference's extend restated, tests/metric_cases.py), nsteps, nsafe, last."""

    def __init__(self, path=None, arrays=None):
        z = arrays if arrays is not None else np.load(path or fixture_path())
        for k in BASE_KEYS + EDGE_KEYS + SCALAR_KEYS + GOAL_KEYS + REWIRE_KEYS:
            if k in z:
                setattr(self, k, np.asarray(z[k]))
        self.band = float(z["band"]) if "band" in z else None
        self.delta_min = float(z["delta_min"]) if "delta_min" in z else None
        lv = [float(x) for x in self.levels]
        var = [(s, d) for d in lv for s in (1, -1)]
        R = {k: [] for k in ("family", "base", "q", "qd", "qdd", "mode", "mass", "joint", "sign",
                             "side", "delta", "margin", "ok")}

        def row(b, q, qd, qdd, mode, mass, side, delta, margin, ok):
            for k, v in zip(R, (self.b_family[b], b, q, qd, qdd, mode, mass, self.b_joint[b],
                                self.b_sign[b], side, delta, margin, ok)):
                R[k].append(v)

        for b in range(len(self.b_q)):
            fam = FAMILIES[self.b_family[b]]
            q, qd, qdd0 = self.b_q[b], self.b_qd[b], self.b_qdd[b]
            mode, mass = int(self.b_mode[b]), float(self.b_mass[b])
            if fam in PROBES:
                for v, (side, delta) in enumerate(var):
                    x = self.b_x[b, v]
                    qq, aa = q.copy(), qdd0
                    if self.b_var[b] >= 0:
                        qq[self.b_var[b]] = x
                    else:
                        aa = qdd0 * x
                    row(b, qq, qd, aa, mode, mass, side, delta, self.b_margin[b, v], side < 0)
            elif fam in ("threshold_rne", "threshold_dyn"):
                aa = qdd0 * self.b_x[b, 0]
                m_pass = PAYLOAD_MIN if fam == "threshold_rne" else 0.0
                row(b, q, qd, aa, mode, m_pass, -1, 0.0, np.nan, True)
                row(b, q, qd, aa, mode, mass, 1, 0.0, self.b_margin[b, 0], False)
            elif fam == "joint7":
                for m in (MODE_NOV, MODE_RNE, MODE_DYN):
                    row(b, q, qd, qdd0, m, mass, 0, 0.0, self.b_margin[b, 0], True)
            else:
                row(b, q, qd, qdd0, mode, mass, 0, 0.0, self.b_margin[b, 0], True)
        for k, v in R.items():
            setattr(self, k, np.array(v))
        self.n = len(self.q)
        self.names = [FAMILIES[f] for f in self.family]
        self._edges(var)
        self._goals()

    def _goals(self):
        """The goal search's rows: the static probes of families 1 and 3 at 1e-6 (from the rows)
        and at 1e-3 (g_x: fails, passes): gq, gmode, gmass, gjoint, gside, gdelta, gok."""
        i = self.rows("static", "dyn_static")
        i = i[self.delta[i] == 1e-6]
        G = [[self.q[r], self.mode[r], self.mass[r], self.joint[r], self.side[r], 1e-6] for r in i]
        for r, b in enumerate(getattr(self, "g_base", ())):
            for c, side in enumerate((1, -1)):
                q = self.b_q[b].copy()
                q[self.b_var[b]] = self.g_x[r, c]
                G.append([q, self.b_mode[b], self.b_mass[b], self.b_joint[b], side, 1e-3])
        for c, k in enumerate(("gq", "gmode", "gmass", "gjoint", "gside", "gdelta")):
            setattr(self, k, np.array([g[c] for g in G]))
        self.gok = self.gside < 0

    def _edges(self, var):
        import metric_cases as MC
        E = {k: [] for k in ("ebase", "ea", "eb", "emode", "emass", "ejoint", "ek", "ekpos",
                             "eside", "edelta", "emargin", "nsteps", "nsafe", "last")}
        self.steps = []
        for e in range(len(getattr(self, "e_a", ()))):
            for v, (side, delta) in enumerate(var):
                a, b = self.e_a[e].copy(), self.e_b[e].copy()
                a[self.e_joint[e]] = self.e_xa[e, v]
                b[self.e_joint[e]] = self.e_xb[e, v]
                st = np.array(MC.extend_ref(a, b, 0.1 * np.ones(7)), dtype=np.float64)
                ns = len(st) if side < 0 else int(self.e_k[e])
                self.steps.append(st)
                for k, x in zip(E, (e, a, b, self.e_mode[e], self.e_mass[e],
                                    self.e_joint[e], self.e_k[e], self.e_kpos[e], side, delta,
                                    self.e_margin[e, v], len(st), ns,
                                    st[ns - 1] if ns else np.full(7, np.nan))):
                    E[k].append(x)
        for k, v in E.items():
            setattr(self, k, np.array(v))
        self.m = len(self.steps)

    def rows(self, *fams):
        return np.array([i for i in range(self.n) if self.names[i] in fams], dtype=np.int64)


def ld_minus_mp(a_ld, a_mp):
    """max |a_ld - a_mp| as a float: a longdouble array against an mpmath one, no rounding of
    either (a longdouble is split into two fp64 parts)."""
    import mpmath
    worst = 0.0
    for x, y in zip(np.asarray(a_ld).flat, np.asarray(a_mp).flat):
        hi = float(x)
        lo = float(x - LD(hi))
        worst = max(worst, float(abs(mpmath.mpf(hi) + mpmath.mpf(lo) - y)))
    return worst
