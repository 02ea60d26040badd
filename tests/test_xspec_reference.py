"""CPU checks of the cross-spectral estimator's numpy reference (tests/xspec_reference.py):
the float32 restatement of the contract stays within 4e-6 (coherence), 1e-6 (PHAT W) and
2e-6 of a plane's own maximum of the float64 model; a delayed pair's lag is recovered
exactly under PHAT with a peak above 0.9, a runner-up below 0.1 and |frac| below 0.01; H1
of a short FIR system gives its taps within 2e-3 with the coherence above 0.98; a run cut
anywhere and carried equals the uncut run bit for bit; the peak's edge cases.  No device."""
import numpy as np
import pytest

import xspec_reference as R

SHAPES = [(256, 128), (512, 128), (1024, 256), (2048, 512)]


def _c64(X):
    return X.astype(np.complex64)


def _spectra(N, H, F, D=5):
    a, b = R.delayed_pair(R.length(N, H, F), D)
    w = R.hann(N)
    return R.stft(a, N, H, w), R.stft(b, N, H, w)


@pytest.mark.parametrize("alpha", [0.0, 0.9])
@pytest.mark.parametrize("N,H", SHAPES)
def test_float32_restatement_against_float64(N, H, alpha):
    A, B = _spectra(N, H, 24)
    s64 = R.accumulate(A, B, alpha, np.float64)
    s32 = R.accumulate(_c64(A), _c64(B), alpha, np.float32)
    assert s32.dtype == np.float32 and s32.shape == (4, N // 2 + 1)
    planes = max(np.abs(s32[j].astype(np.float64) - s64[j]).max() / np.abs(s64[j]).max() for j in range(4))
    c64, _, w64 = R.derive(s64, R.PHAT, np.float64)
    c32, _, w32 = R.derive(s32, R.PHAT, np.float32)
    assert c32.dtype == np.float32 and w32.dtype == np.complex64
    dc, dw = np.abs(c32 - c64).max(), np.abs(w32 - w64).max()
    print(f"{N}/{H} alpha={alpha}: planes {planes:.2e} of their maximum, coherence {dc:.2e}, W {dw:.2e}")
    assert dc <= 4e-6
    assert dw <= 1e-6
    assert planes <= 2e-6


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("N,H", SHAPES)
def test_delay_recovery(N, H, dt):
    w = R.hann(N)
    for D in (0, 1, -20, 37, N // 4):
        a, b = R.delayed_pair(R.length(N, H, 24), D)
        A, B = R.stft(a, N, H, w), R.stft(b, N, H, w)
        if dt is np.float32:
            A, B = _c64(A), _c64(B)
        rows, cc = R.delay(R.accumulate(A, B, 0.0, dt), N, R.PHAT, N // 2 - 1, dt)
        lag, frac, val = (float(v) for v in rows)
        ru = R.runner_up(cc, N // 2 - 1, int(lag))
        print(f"{N}/{H} {dt.__name__} D={D}: lag {lag:.0f} frac {frac:+.2e} peak {val:.4f} runner-up {ru:.4f}")
        assert lag == D
        assert val >= 0.9
        assert ru <= 0.1
        assert abs(frac) <= 0.01


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("N,H", SHAPES[:3])
def test_h1_recovery(N, H, dt):
    a, b = R.fir_pair(R.length(N, H, 60))
    w = R.hann(N)
    A, B = R.stft(a, N, H, w), R.stft(b, N, H, w)
    if dt is np.float32:
        A, B = _c64(A), _c64(B)
    C, H1, _ = R.derive(R.accumulate(A, B, 0.0, dt), R.NONE, dt)
    h = np.fft.irfft(H1.astype(np.complex128), N)
    taps, rest = np.abs(h[:8] - R.FIR).max(), np.abs(h[8:]).max()
    print(f"{N}/{H} {dt.__name__}: taps within {taps:.2e}, elsewhere {rest:.2e}, min coherence {C.min():.4f}")
    assert taps <= 2e-3
    assert rest <= 2e-3
    assert C.min() >= 0.98


@pytest.mark.parametrize("alpha", [0.0, 0.9])
def test_cut_and_carry_equals_the_uncut_run(alpha):
    A, B = (_c64(X) for X in _spectra(256, 128, 26))
    st = R.accumulate(A, B, alpha)
    for F1 in range(1, 26):
        sa = R.accumulate(A[:F1], B[:F1], alpha)
        sb = R.accumulate(A[F1:], B[F1:], alpha, state=sa)
        assert np.array_equal(sb.view(np.uint32), st.view(np.uint32)), F1


def test_batched_pairs_and_shared_reference_equal_each_alone():
    A, B = (_c64(X) for X in _spectra(256, 128, 12))
    B3 = np.stack([B, B * np.float32(0.25), B[::-1].copy()])
    s3 = R.accumulate(A, B3, 0.9)
    assert s3.shape == (3, 4, 129)
    assert np.array_equal(s3, R.accumulate(np.stack([A, A, A]), B3, 0.9))
    for i in range(3):
        assert np.array_equal(s3[i], R.accumulate(A, B3[i], 0.9))


def test_zero_columns_clamp_at_tiny():
    st = R.accumulate(np.zeros((5, 7), np.complex64), np.zeros((5, 7), np.complex64))
    assert np.all(st == 0)
    for wt in (R.NONE, R.PHAT):
        C, H1, W = R.derive(st, wt)
        assert np.all(C == 0) and np.all(H1 == 0) and np.all(W == 0)


def test_welch_planes_are_plain_sums_and_factors():
    assert R.factors(0.0) == (1.0, 1.0)
    lam, om = R.factors(0.9)
    assert lam == np.float32(0.9) and om == np.float32(1.0 - 0.9) and om != np.float32(1) - lam
    A, B = (_c64(X) for X in _spectra(256, 128, 6))
    st = R.accumulate(A, B)
    want = np.zeros_like(st[0])
    for f in range(6):
        want = want + R.terms(A[f], B[f])[0]
    assert np.array_equal(st[0], want)


def test_peak_edge_cases():
    n, m = 64, 31
    base = np.linspace(-1.0, -0.5, n).astype(np.float32)

    def at(j):
        return (j - m) % n

    cc = base.copy()
    cc[[at(3), at(40), at(62)]] = 5.0  # equal maxima: the smallest j wins
    assert R.peak_row(cc, m)[0] == 3 - m
    cc = base.copy()
    cc[at(0)] = 7.0
    assert R.peak_row(cc, m)[0] == -m
    cc = base.copy()
    cc[at(2 * m)] = 7.0
    assert R.peak_row(cc, m)[0] == m
    cc = base.copy()
    cc[at(10)], cc[at(20)] = np.nan, 3.0  # a NaN elsewhere never wins
    row = R.peak_row(cc, m)
    assert row[0] == 20 - m and row[2] == 3.0
    flat = np.full(n, 0.25, np.float32)  # den = 0
    assert np.array_equal(R.peak_row(flat, m), np.array([-m, 0.0, 0.25], np.float32))
    cc = np.zeros(n, np.float32)  # an exact parabola through (-1, 1), (0, 2), (1, 2): frac = +0.5
    cc[at(m - 1)], cc[at(m)], cc[at(m + 1)] = 1.0, 2.0, 2.0
    row = R.peak_row(cc, m)
    assert row[0] == 0 and row[1] == np.float32(0.5) and row[2] == 2.0
    assert R.peak_row(cc, 1)[0] == 0
