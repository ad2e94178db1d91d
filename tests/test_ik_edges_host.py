"""CPU: the oracle's ik8 / fk8 at the folds, the shoulder singularity and the edges of the
acceptance band, against tests/golden/ik_edges.npz (a 50-digit restatement of the closed form;
tests/golden/gen_ik_edges.py) and the longdouble pose reference of tests/ik_ref.py.

Per case (ik_ref.check_case): 1. the count equals the reference's; 2. every solution maps back
to the requested pose through fk_ld -- 1e-9, or at a fold twice the reference's own residual plus
1e-9, since the clamp itself moves the pose; 3. some solution is the generating q mod 2 pi --
1e-8 (q1 + q3 where |q2| <= 1e-7), or at a fold 1e-2 rad, which separates a present branch from
an absent one (an absent branch leaves the nearest solution about 1.4 rad away); 4. families G,
W, Z: every solution within 1e-9 of the reference's in the same slot.

The reference's own residuals in the fixture, per family (the generator prints them):
  G 6.0e-16  W 4.4e-16  F6 1.8e-14  F6n 4.4e-16  F4 4.6e-16  F4n 5.1e-16  F46 9.6e-9
  S 2.0e-13  Z 3.8e-16  B (inside) 4.7e-9
so the fold bounds are 1e-9 except F46 (2.0e-8) and B (1.05e-8).
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN

import oracle as O  # noqa: E402  (test infrastructure)
import ik_ref as R


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def solved(fx):
    """The oracle on every case, once: (sols (n, 8, 7), count (n,))."""
    sols = np.zeros((fx.n, 8, 7))
    cnt = np.zeros(fx.n, dtype=np.int32)
    for i in range(fx.n):
        s, _ = O.ik8(R.pose44(fx.pose[i]), fx.free[i])
        sols[i, :len(s)] = s
        cnt[i] = len(s)
    return sols, cnt


def test_fixture_layout(fx):
    assert fx.n == len(R.FAMILIES) * R.N_PER_FAMILY
    for f, fam in enumerate(R.FAMILIES):
        assert fx.rows(fam) == list(range(f * R.N_PER_FAMILY, (f + 1) * R.N_PER_FAMILY))
    assert (fx.free == fx.q[:, 6]).all()
    assert ((fx.q >= R.LO) & (fx.q <= R.HI)).all()
    assert (fx.count[fx.rows("X")] == 0).all()
    b = fx.rows("B")
    assert (fx.count[b[:32]] > 0).all() and (fx.count[b[32:]] == 0).all()
    for fam in R.FAMILIES[:9]:
        assert (fx.count[fx.rows(fam)] > 0).all(), fam
    w = fx.rows("W")
    assert (fx.q[w, 5] > np.pi + 0.05).all() and (fx.q[w, 5] < 3.70).all()
    assert os.path.getsize(os.path.join(GOLDEN, "ik_edges.npz")) < (1 << 20)


def test_fk_ld_matches_reference_dh():
    z = np.load(os.path.join(GOLDEN, "fk_golden.npz"))
    for q, T in zip(z["q"], z["T"]):
        assert np.abs(R.fk_ld(q) - T).max() < 1e-12


def test_fixture_poses_are_fk_ld(fx):
    """Families G..Z: the stored pose is fk_ld(q) rounded (1 ulp of slack for another libm)."""
    for fam in R.FAMILIES[:9]:
        for i in fx.rows(fam):
            assert np.abs(R.pose12(R.fk_ld(fx.q[i])) - fx.pose[i]).max() <= 4.5e-16, (fam, i)


def test_oracle_fk8_matches_fk_ld(fx):
    """Assertion 7 on the CPU: every generating q, the exact zeros of family Z included."""
    for i in range(fx.n):
        T = O.fk8(fx.q[i])
        assert np.abs(R.fk_ld(fx.q[i]) - T).max() < 1e-12, (fx.names[i], i)


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_oracle_ik_edges(fx, solved, fam):
    """Assertions 1-4."""
    sols, cnt = solved
    worst_r = worst_m = 0.0
    outside = 0
    for i in fx.rows(fam):
        r, m = R.check_case(fx, i, sols[i], cnt[i])
        worst_r, worst_m = max(worst_r, r), max(worst_m, m)
        got = sols[i, :cnt[i]]
        outside += R.just_outside(got)
    print("%s: pose residual %.3e (bound %.3e), distance from q %.3e (bound %.0e), "
          "%d solutions within 1e-8 outside a limit"
          % (fam, worst_r, fx.sound_bound(fam), worst_m, fx.complete_bound(fam), outside))


def test_wide_joint6_comes_back_as_the_lower_image(fx, solved):
    """Family W: tcmp_ik's range is (-pi, pi], so the generating q6 > pi is reported as q6 - 2 pi
    (below joint 6's lower limit); the goal search takes the image back (tests/goal_ref.py)."""
    sols, cnt = solved
    for i in fx.rows("W"):
        got = sols[i, :cnt[i]]
        k = int(np.argmin([R.shoulder_dist(s, fx.q[i]) for s in got]))
        assert abs(got[k, 5] - (fx.q[i, 5] - 2 * np.pi)) < 1e-8, i
        assert got[k, 5] < R.LO[5]


def test_closure(fx, solved):
    """Assertion 5: ik(fk(solution k), q7) returns the same set."""
    sols, cnt = solved
    for i in fx.rows("G")[:16]:
        for k in range(cnt[i]):
            s, _ = O.ik8(O.fk8(sols[i, k]), fx.free[i])
            assert R.pair_sets(s, sols[i, :cnt[i]]) <= 1e-8, (i, k)


def test_regenerate_a_sample_with_mpmath(fx):
    """The first 8 cases of every family solved again at 50 digits: the committed fixture is the
    generator's output."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("gen_ik_edges",
                                                  os.path.join(GOLDEN, "gen_ik_edges.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = gen.all_cases()
    assert len(cases) == fx.n
    for i, (fam, j, q, pose) in enumerate(cases):
        assert fam == fx.names[i] and (q == fx.q[i]).all(), i
        assert np.abs(pose - fx.pose[i]).max() <= 4.5e-16, i
        if j < 8:
            n, s, r, _ = gen.checked_case(fam, j, q, fx.pose[i])
            assert n == fx.count[i], i
            assert np.abs(s - fx.sols[i]).max() <= 1e-14 and np.abs(r - fx.resid[i]).max() <= 1e-14, i
