"""CPU tests of the HPSS references (tests/hpss_reference.py): the medians are
scipy.ndimage.median_filter(mode='reflect') exactly, also where the window is
longer than the axis; the float32 soft mask agrees with librosa's formula in
float64 on the same medians; the hard masks and the zero rules by hand."""
import numpy as np
import pytest

import hpss_reference as H


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("F,bins,w", [(1, 5, 31), (7, 129, 31), (31, 33, 31), (40, 201, 63), (100, 513, 17),
                                      (3, 3, 63), (9, 9, 1)])
def test_medians_equal_scipy_reflect(F, bins, w):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(F * 1000 + bins + w)
    m = np.abs(rng.standard_normal((F, bins))).astype(np.float32)
    m[rng.random((F, bins)) < 0.2] = 0          # ties
    h, p = H.medians32(m, w, w)
    assert np.array_equal(bits(h), bits(ndimage.median_filter(m, size=(w, 1), mode="reflect")))
    assert np.array_equal(bits(p), bits(ndimage.median_filter(m, size=(1, w), mode="reflect")))


def test_ext_is_the_reflect_map():
    assert H.ext(np.arange(-9, 9), 3).tolist() == [2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2]
    assert H.ext(np.arange(-3, 4), 1).tolist() == [0] * 7


@pytest.mark.parametrize("power", [1, 2])
def test_soft_mask_float32_against_float64(power):
    """At most four float32 roundings (a, b, a + b; power 2: the squares, whose
    relative errors add to the two quotients') on values <= 1: |mask32 - mask64|
    <= 4 * 2^-24.  Seen over 10^6 random pairs per power: 1.50 * 2^-24 (power 1)
    and 1.49 * 2^-24 (power 2)."""
    rng = np.random.default_rng(power)
    n = 1_000_000
    X = (np.abs(rng.standard_normal(n)) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    R = (X * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    got = H.softmask32(X, R, power, True)
    want = H.softmask64(X, R, power, True)
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"power {power}: max |mask32 - mask64| = {err / H.U32:.3f} * 2^-24")
    assert err <= 4 * H.U32
    assert np.all((got >= 0) & (got <= 1))


def test_hard_masks_and_ties():
    X = np.array([1, 2, 3, 0, 5], np.float32)
    R = np.array([2, 2, 1, 0, np.inf], np.float32)
    assert H.softmask32(X, R, H.HARD, True).tolist() == [0, 0, 1, 0, 0]
    assert H.softmask32(R, X, H.HARD, True).tolist() == [1, 0, 0, 0, 1]   # a tie gives 0 in both


def test_zero_rules():
    z = np.zeros(3, np.float32)
    tiny = np.full(3, 1e-39, np.float32)  # below FLT_MIN
    for power in (1, 2):
        assert H.softmask32(z, z, power, True).tolist() == [0.5] * 3       # split_zeros
        assert H.softmask32(z, z, power, False).tolist() == [0.0] * 3
        assert H.softmask32(tiny, tiny, power, True).tolist() == [0.5] * 3
        one = np.ones(3, np.float32)
        assert H.softmask32(z, one, power, True).tolist() == [0.0] * 3
        assert H.softmask32(one, z, power, True).tolist() == [1.0] * 3
        assert H.softmask32(one, one, power, True).tolist() == [0.5] * 3


def test_masks32_end_to_end_small():
    """(1, 1) windows with margins 1: h = p = m, so every mask is 0.5; margins (2, 3.7)
    turn the split rule off and push both masks down."""
    Z = H.make_spectrum(256, 2, 9, nasty=True)
    mh, mp = H.masks32(Z, 1, 1, 2, 1.0, 1.0)
    assert np.all(mh == 0.5) and np.all(mp == 0.5)
    mh, mp = H.masks32(Z, 1, 1, 1, 2.0, 3.7)
    m = H.magnitude32(Z)
    assert np.all(mh[m == 0] == 0) and np.all(mp[m == 0] == 0)
    assert np.all((mh >= 0) & (mh <= 0.5)) and np.all((mp >= 0) & (mp <= 0.5))
    # sanitize: the NaN / Inf / tiny components count as 0
    assert m[-1, 0, 3] == 1 and m[-1, 0, 4] == 1 and m[-1, 1, 5] == 2 and m[-1, 1, 6] == 0
    assert np.all(m[-1, :, 64:96] == 5)
