"""CPU checks of the noise suppressor's numpy reference (tests/denoise_reference.py): the
float32 restatement of the contract stays within 1e-4 of the float64 model in G; on the
long input the model removes at least 15 dB of the noise in the gaps and lifts the SNR
inside the bursts by at least 10 dB; g_min = 1 is the identity; a run cut anywhere and
carried equals the uncut run bit for bit.  No device."""
import numpy as np
import pytest

import denoise_reference as R

SHAPES = [(256, 128, 40, 8), (512, 128, 40, 8), (1024, 256, 40, 8)]
LONG = (512, 128, 500, 62)


def _spectra(N, H, F):
    s, v, on = R.bursts(N, H, F)
    w = R.sqrt_hann(N)
    x = (s + v).astype(np.float32).astype(np.float64)
    return R.stft(x, N, H, w), s, v, on, w


@pytest.fixture(scope="module")
def long_run():
    N, H, F, L = LONG
    X, s, v, on, w = _spectra(N, H, F)
    G64, _ = R.gains(R.power(X, np.float64), np.float64, window=L)
    G32, _ = R.gains(R.power(X, np.float32), np.float32, window=L)
    return dict(N=N, H=H, X=X, s=s, v=v, on=on, w=w, G64=G64, G32=G32)


@pytest.mark.parametrize("N,H,F,L", SHAPES)
def test_float32_restatement_within_1e4_of_float64(N, H, F, L):
    X = _spectra(N, H, F)[0]
    G64, _ = R.gains(R.power(X, np.float64), np.float64, window=L)
    G32, st = R.gains(R.power(X, np.float32), np.float32, window=L)
    assert G32.dtype == np.float32 and st.dtype == np.float32 and st.shape == (6, N // 2 + 1)
    d = np.abs(G32.astype(np.float64) - G64)
    print(f"{N}/{H} F={F} L={L}: max |G32 - G64| = {d.max():.2e}")
    assert d.max() <= 1e-4
    assert G64.min() >= 0.1 and G64.max() <= 1.0


def test_float32_restatement_long_run(long_run):
    d = np.abs(long_run["G32"].astype(np.float64) - long_run["G64"])
    print(f"long run: max |G32 - G64| = {d.max():.2e}")
    assert d.max() <= 1e-4


def test_model_suppresses_gaps_and_lifts_bursts(long_run):
    r = long_run
    nr_gap, snr_gain = R.behaviour(r["G64"], r["s"], r["v"], r["on"], r["N"], r["H"], r["w"])
    print(f"gap noise reduction {nr_gap:.1f} dB, in-burst SNR gain {snr_gain:+.1f} dB")
    assert nr_gap >= 15.0
    assert snr_gain >= 10.0
    assert nr_gap <= 20.0 + 0.5  # g_min = 0.1 is a 20 dB floor


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_gmin_one_is_the_identity(dt):
    X = _spectra(256, 128, 40)[0]
    G, _ = R.gains(R.power(X, dt), dt, window=8, g_min=1.0)
    assert G.dtype == dt and np.all(G == dt(1))


def test_cut_and_carry_equals_the_uncut_run():
    N, H, F, L = 256, 128, 3 * 8 + 2, 8
    P = R.power(_spectra(N, H, F)[0], np.float32)
    G, st = R.gains(P, np.float32, window=L)
    for F1 in range(1, F):
        Ga, sa = R.gains(P[:F1], np.float32, window=L)
        Gb, sb = R.gains(P[F1:], np.float32, state=sa, k0=F1, window=L)
        assert np.array_equal(np.concatenate([Ga, Gb]).view(np.uint32), G.view(np.uint32)), F1
        assert np.array_equal(sb.view(np.uint32), st.view(np.uint32)), F1


def test_zero_columns_clamp_to_gmin():
    P = np.zeros((10, 5), np.float32)
    G, st = R.gains(P, np.float32, window=4)
    assert np.all(G == np.float32(0.1)) and np.all(st == 0)


def test_batched_streams_equal_each_alone():
    P = R.power(_spectra(256, 128, 20)[0], np.float32)
    P3 = np.stack([P, P * np.float32(0.25), P[::-1].copy()])
    G3, s3 = R.gains(P3, np.float32, window=8)
    for i in range(3):
        G, st = R.gains(P3[i], np.float32, window=8)
        assert np.array_equal(G, G3[i]) and np.array_equal(st, s3[i])
