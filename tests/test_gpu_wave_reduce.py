"""The device's fp32 wave reductions (csrc/tcmp_device.h: wave_minf, wave_maxf, wave_minf_bc and
the multi-value wave_minmax3 of the exact test's box-face stage) through
tcmp_debug_wave_reduce: one wave per row of 64 lanes x 6 columns, against numpy.min / numpy.max
over the lanes with exact equality (`==`, so -0 equals +0: the helpers' contract leaves the sign
of a zero result open).  The helpers reduce order-preserving integer keys in six DPP steps; the
cases put the extreme in every lane (a wrong row or bank mask loses some lanes), at the
identities, at zeros of both signs, in the denormals, and in columns that are each other's
negation.  No NaN inputs: the contract excludes them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from torque_constrained_motion_planning_amd import _lib
    e = _lib.Engine(0)
    yield e
    e.close()


def _check(eng, v):
    """v (n, 64, 6) float32: columns 0..2 are reduced as minima, 3..5 as maxima, column 0
    also by the three single-value helpers."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    assert not np.isnan(v).any()
    out = eng.debug_wave_reduce(v)
    assert out.shape == (len(v), 9) and out.dtype == np.float32
    mn, mx = v.min(axis=1), v.max(axis=1)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            assert (out[:, c] == mn[:, c]).all(), ("min3", c)
            assert (out[:, 3 + c] == mx[:, 3 + c]).all(), ("max3", c)
        assert (out[:, 6] == mn[:, 0]).all(), "wave_minf"
        assert (out[:, 7] == mx[:, 0]).all(), "wave_maxf"
        assert (out[:, 8] == mn[:, 0]).all(), "wave_minf_bc"
    return out


def _random(rng, shape):
    """both signs, magnitudes log-uniform over 1e-30..1e30"""
    mag = 10.0 ** rng.uniform(-30.0, 30.0, size=shape)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def test_random_waves(eng):
    rng = np.random.default_rng(1)
    v = _random(rng, (256, 64, 6))
    assert np.isfinite(v).all() and (v != 0).all()
    _check(eng, v)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_extreme_in_each_lane(eng, sign):
    """wave l holds its extreme value in lane l only (the minimum for sign -1 read as minima,
    the maximum for sign +1 read as maxima; every column, so both kinds see both)."""
    rng = np.random.default_rng(2)
    v = rng.uniform(-1.0, 1.0, size=(64, 64, 6)).astype(np.float32)
    for lane in range(64):
        v[lane, lane, :] = sign * (2.0 + lane)
    out = _check(eng, v)
    want = sign * (2.0 + np.arange(64, dtype=np.float32))
    cols = [3, 4, 5, 7] if sign > 0 else [0, 1, 2, 6, 8]
    for c in cols:
        assert (out[:, c] == want).all(), c


def test_all_equal(eng):
    vals = np.array([0.0, -0.0, 1.0, -1.0, 3.4e38, -3.4e38, 1e-45, -1e-45, np.inf, -np.inf],
                    dtype=np.float32)
    v = np.broadcast_to(vals[:, None, None], (len(vals), 64, 6))
    out = _check(eng, v)
    assert (out == vals[:, None]).all()


def test_identities(eng):
    """all lanes but one at the identity of min (+inf) / of max (-inf); the lone lane moves
    over the wave and holds a value of either sign, or the other infinity"""
    rng = np.random.default_rng(3)
    lone = np.array([1.5, -1.5, 1e-38, -1e30, np.inf, -np.inf], dtype=np.float32)
    rows = []
    for ident in (np.inf, -np.inf):
        for lane in (0, 1, 15, 16, 31, 32, 47, 48, 62, 63):
            for x in lone:
                w = np.full((64, 6), ident, dtype=np.float32)
                w[lane, :] = x
                rows.append(w)
    _check(eng, np.stack(rows))
    # and identities in some lanes of otherwise random waves (partially filled hulls)
    v = _random(rng, (64, 64, 6))
    v[:, :, :3][rng.random((64, 64, 3)) < 0.5] = np.inf
    v[:, :, 3:][rng.random((64, 64, 3)) < 0.5] = -np.inf
    _check(eng, v)


def test_zeros_of_both_signs(eng):
    rng = np.random.default_rng(4)
    z = np.where(rng.random((32, 64, 6)) < 0.5, 0.0, -0.0).astype(np.float32)
    _check(eng, z)
    # zeros as the extreme among values of one sign
    pos = np.abs(_random(rng, (32, 64, 6)))
    m = rng.random((32, 64, 6)) < 0.2
    pos[m] = z[m]
    _check(eng, pos)
    _check(eng, -pos)


def test_denormals(eng):
    rng = np.random.default_rng(5)
    bits = rng.integers(1, 1 << 23, size=(64, 64, 6), dtype=np.int64).astype(np.uint32)
    bits |= (rng.integers(0, 2, size=bits.shape, dtype=np.int64).astype(np.uint32) << np.uint32(31))
    v = bits.view(np.float32)
    assert (np.abs(v) < np.finfo(np.float32).tiny).all() and (v != 0).all()
    out = _check(eng, v)
    assert (out != 0).all()  # nothing flushed
    # denormals next to normal values and zeros
    w = v.copy()
    m = rng.random(w.shape)
    w[m < 0.1] = 0.0
    w[m > 0.9] = _random(rng, w.shape)[m > 0.9]
    _check(eng, w)


def test_negated_columns(eng):
    """a minimum and a maximum over the same magnitudes: columns 3..5 are -columns 0..2, so
    max(col 3 + c) == -min(col c) bit for bit"""
    rng = np.random.default_rng(6)
    a = _random(rng, (128, 64, 3))
    v = np.concatenate([a, -a], axis=2)
    out = _check(eng, v)
    assert (out[:, 3:6] == -out[:, 0:3]).all()
    assert (out[:, 7] == v[:, :, 0].max(axis=1)).all()


def test_rejects_bad_shapes(eng):
    with pytest.raises(ValueError):
        eng.debug_wave_reduce(np.zeros((2, 32, 6), dtype=np.float32))
    assert eng.debug_wave_reduce(np.zeros((0, 64, 6), dtype=np.float32)).shape == (0, 9)
