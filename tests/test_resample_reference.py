"""The float64 reference of the resampler (tests/resample_reference.py) against an
independent formulation: scipy.signal.upfirdn over the prototype filter the
polyphase rows are samples of; the rows' DC gain; and a tone's frequency."""
import numpy as np
import pytest

import resample_reference as RR

CASES = [(160, 147), (147, 160), (1, 2), (2, 1), (3, 1), (1, 3), (7, 5), (89, 84), (1, 64)]
LENGTHS = (1, 5, 1000, 1777)


def zeros_of(U, D):
    return {(7, 5): 4, (1, 64): 4, (3, 1): 6, (1, 3): 6}.get((U, D), 16)  # (the GPU test's filters)


@pytest.mark.parametrize("U,D", CASES)
def test_reference_equals_upfirdn(U, D):
    """Row r of the table is the prototype g sampled at r / U: g[(j U - r) + W U] =
    h[r][j + W - 1].  x upsampled by U and filtered with g, read at W U + m D, is
    output m.  The issue's prototype agreed to <= 1.4e-15."""
    signal = pytest.importorskip("scipy.signal")
    zeros = zeros_of(U, D)
    _, _, W, K, _ = RR.geometry(U, D, zeros)
    h, _ = RR.table(U, D, zeros)
    g = np.zeros(2 * W * U + 1)
    for r in range(U):
        for i in range(K):
            g[((i - W + 1) * U - r) + W * U] = h[r, i]
    rng = np.random.default_rng(U * 131 + D)
    for T in LENGTHS:
        x = rng.uniform(-1.0, 1.0, T)
        y, _ = RR.resample(x, U, D, W, h)
        L = RR.output_length(T, U, D)
        assert y.shape == (L,) and L == -(-T * U // D)
        z = signal.upfirdn(g, x, up=U, down=1)
        want = z[W * U + np.arange(L) * D]
        err = float(np.abs(y - want).max())
        print(f"U/D {U}/{D} T {T}: max |ref - upfirdn| = {err:.3g}")
        assert err <= 1.4e-15, (U, D, T, err)


@pytest.mark.parametrize("window", ["hann", "kaiser"])
def test_rows_sum_to_one(window):
    """Every phase has unit DC gain to within the window's leakage: the prototype's
    worst row was 1.0020 at 7/5 with zeros = 4 and 1.00003 at zeros = 16."""
    for U, D in CASES + [(1021, 1024)]:
        for zeros in (4, 6, 16):
            h, tau = RR.table(U, D, zeros, window=window)
            s = h.sum(1)
            assert float(np.abs(s - 1.0).max()) <= 2.5e-3, (U, D, zeros, s.min(), s.max())
            assert np.all(h[np.abs(tau) >= zeros] == 0.0)


def test_tone_keeps_its_frequency():
    """1 kHz at 44.1 kHz is 1 kHz at 48 kHz: the peak of the middle 4096 samples'
    spectrum sits in the bin of 1000 Hz (test_sinusoid_keeps_its_pitch's method)."""
    U, D, W, K, _ = RR.geometry(48000, 44100)
    assert (U, D, W, K) == (160, 147, 17, 34)
    h, _ = RR.table(U, D)
    T = 12000
    x = np.sin(2 * np.pi * 1000.0 / 44100.0 * np.arange(T))
    y, _ = RR.resample(x, U, D, W, h)
    assert len(y) == RR.output_length(T, U, D) == 13062
    mid = y[len(y) // 2 - 2048:len(y) // 2 + 2048]
    spec = np.abs(np.fft.rfft(mid * np.hanning(4096)))
    assert int(np.argmax(spec)) == round(1000.0 / 48000.0 * 4096)
    assert 0.95 < np.abs(mid).max() < 1.05
