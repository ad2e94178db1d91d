"""GPU: tcmp_ik / tcmp_fk (k_ik, k_fk8; csrc/tcmp_ik.h) at the folds, the shoulder singularity and
the edges of the acceptance band.  Reads only tests/golden/ik_edges.npz (a 50-digit restatement
of the closed form; tests/golden/gen_ik_edges.py) and tests/ik_ref.py, whose fk_ld (the DH chain
in numpy.longdouble) is the pose reference; the CPU oracle is not involved.  704 lanes in all.

Per case (ik_ref.check_case): 1. the count equals the reference's; 2. every solution maps back
to the requested pose through fk_ld -- 1e-9, or at a fold twice the reference's own residual plus
1e-9, since the clamp itself moves the pose; 3. some solution is the generating q mod 2 pi --
1e-8 (q1 + q3 where |q2| <= 1e-7), or at a fold 1e-2 rad, which separates a present branch from
an absent one; 4. families G, W, Z: every solution within 1e-9 of the reference's in the same
slot.  Then 5. closure, 6. launch shapes, 7. FK.

The reference's own residuals in the fixture, per family (the generator prints them):
  G 6.0e-16  W 4.4e-16  F6 1.8e-14  F6n 4.4e-16  F4 4.6e-16  F4n 5.1e-16  F46 9.6e-9
  S 2.0e-13  Z 3.8e-16  B (inside) 4.7e-9
so the fold bounds are 1e-9 except F46 (2.0e-8) and B (1.05e-8).
"""
import numpy as np
import pytest

import ik_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from torque_constrained_motion_planning_amd import _lib
    return _lib.engine(0)


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def solved(eng, fx):
    """The whole fixture in one call: (sols (n, 8, 7), count (n,))."""
    return eng.ik(fx.pose, fx.free)


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_ik_edges(fx, solved, fam):
    """Assertions 1-4."""
    sols, cnt = solved
    worst_r = worst_m = 0.0
    outside = 0
    for i in fx.rows(fam):
        r, m = R.check_case(fx, i, sols[i], cnt[i])
        worst_r, worst_m = max(worst_r, r), max(worst_m, m)
        outside += R.just_outside(sols[i, :cnt[i]])
    print("%s: pose residual %.3e (bound %.3e), distance from q %.3e (bound %.0e), "
          "%d solutions within 1e-8 outside a limit"
          % (fam, worst_r, fx.sound_bound(fam), worst_m, fx.complete_bound(fam), outside))


def test_wide_joint6_comes_back_as_the_lower_image(fx, solved):
    """Family W: tcmp_ik's range is (-pi, pi], so the generating q6 > pi is reported as
    q6 - 2 pi, below joint 6's lower limit."""
    sols, cnt = solved
    for i in fx.rows("W"):
        got = sols[i, :cnt[i]]
        k = int(np.argmin([R.shoulder_dist(s, fx.q[i]) for s in got]))
        assert abs(got[k, 5] - (fx.q[i, 5] - 2 * np.pi)) < 1e-8, i
        assert got[k, 5] < R.LO[5]


def test_closure(eng, fx, solved):
    """Assertion 5: ik(fk(solution k), q7) returns the same set, for 16 generic cases."""
    sols, cnt = solved
    rows = fx.rows("G")[:16]
    src = [(i, k) for i in rows for k in range(cnt[i])]
    poses = eng.fk(np.array([sols[i, k] for i, k in src]))
    again, cnt2 = eng.ik(poses, np.array([fx.free[i] for i, _ in src]))
    for j, (i, k) in enumerate(src):
        assert R.pair_sets(again[j, :cnt2[j]], sols[i, :cnt[i]]) <= 1e-8, (i, k)


def test_launch_shapes(eng, fx, solved):
    """Assertion 6: k_ik's and k_fk8's tail guard and lane independence -- the one-call result
    is bit-identical to calls of 255, 256 and 257 rows covering the fixture and to single rows."""
    sols, cnt = solved
    fk = eng.fk(fx.q)
    spans = [(a, min(a + n, fx.n)) for n in (255, 256, 257) for a in range(0, fx.n, n)]
    spans += [(a, a + 1) for a in range(0, fx.n, 16)] + [(fx.n - 1, fx.n)]
    for a, b in spans:
        s, c = eng.ik(fx.pose[a:b], fx.free[a:b])
        assert (c == cnt[a:b]).all(), (a, b)
        live = np.arange(8)[None, :] < c[:, None]        # (slots past the count are unspecified)
        assert s[live].tobytes() == sols[a:b][live].tobytes(), (a, b)
        assert eng.fk(fx.q[a:b]).tobytes() == fk[a:b].tobytes(), (a, b)


def test_fk_matches_fk_ld(eng, fx):
    """Assertion 7: every generating q, the exact zeros of family Z included."""
    P = eng.fk(fx.q)
    for i in range(fx.n):
        T = R.fk_ld(fx.q[i])
        ref = np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])
        assert float(np.abs(ref - P[i].astype(R.LD)).max()) < 1e-12, (fx.names[i], i)
