"""CPU tests of the WPE reference (tests/wpe_reference.py): the float64 model's RLS step
equals a direct transcription of the OnlineWPE equations, and its offline steps equal the
normal equations solved by linalg.solve, within 1e-9; the float32 restatement run in
float64 equals the model (so the restatement is the same algorithm); where a run is cut
does not change a bit of the restatement; and on the reverberant scene of the issue the
model improves on the input.  The figures the GPU tests' bars come from (the float32
restatement against the model on that scene) are measured here and held to the
figures DESIGN 3s tables.  No GPU."""
import numpy as np
import pytest

import wpe_reference as W

RNG = np.random.default_rng(11)


def spectra(lead, M, F, bins, scale=1.0):
    Y = RNG.standard_normal(lead + (M, F, bins)) + 1j * RNG.standard_normal(lead + (M, F, bins))
    # a little reverberation along the frames, so that the prediction has something to find
    for t in range(1, F):
        Y[..., t, :] += 0.6 * Y[..., t - 1, :]
    return scale * Y


def test_model_rls_equals_the_online_wpe_equations():
    M, K, D, F, bins, alpha, floor = 2, 3, 2, 14, 5, 0.99, 1e-10
    Y = spectra((), M, F, bins)
    out, Q, G = W.model_rls(Y, K, D, alpha, floor)
    L = M * K
    for b in range(bins):
        Qb, Gb = np.eye(L, dtype=np.complex128), np.zeros((L, M), np.complex128)
        for t in range(F):
            y = np.array([Y[l % M, t - D - l // M, b] if t - D - l // M >= 0 else 0.0 for l in range(L)])
            x = Y[:, t, b]
            pred = x - Gb.conj().T @ y
            power = max(np.mean(np.abs(x) ** 2), floor)
            nominator = Qb @ y
            denominator = alpha * power + np.real(y.conj() @ Qb @ y)
            kal = nominator / max(denominator, W.TINY)
            Qb = (Qb - np.outer(kal, y.conj()) @ Qb) / alpha
            Gb = Gb + np.outer(kal, pred.conj())
            assert np.abs(out[:, t, b] - pred).max() <= 1e-9 * max(1.0, np.abs(pred).max())
        assert np.abs(Q[b] - Qb).max() <= 1e-9 * np.abs(Qb).max()
        assert np.abs(G[b] - Gb).max() <= 1e-9 * max(1.0, np.abs(Gb).max())


def test_model_offline_equals_the_normal_equations():
    M, K, D, F, bins, loading, floor = 3, 2, 1, 20, 4, 1e-3, 1e-10
    Y = spectra((), M, F, bins)
    Z = W.model_offline(Y, K, D, 1, loading, floor)
    L = M * K
    for b in range(bins):
        lam = np.maximum(np.mean(np.abs(Y[:, :, b]) ** 2, axis=0), floor)
        Yt = np.zeros((L, F), np.complex128)
        for l in range(L):
            for t in range(F):
                if t - D - l // M >= 0:
                    Yt[l, t] = Y[l % M, t - D - l // M, b]
        R = (Yt / lam) @ Yt.conj().T
        P = (Yt / lam) @ Y[:, :, b].conj().T
        A = R + loading * np.real(np.trace(R)) / L * np.eye(L)
        G = np.linalg.solve(A, P)
        X = Y[:, :, b] - G.conj().T @ Yt
        assert np.abs(Z[:, :, b] - X).max() <= 1e-9 * np.abs(X).max()


def test_restatement_in_float64_equals_the_model():
    M, K, D, F, bins = 2, 3, 2, 16, 6
    Y = spectra((2,), M, F, bins)
    dt = np.float64
    Z = W.dereverb_spec(Y, K, D, 2, 1e-3, 1e-10, dt)
    Zm = W.model_offline(Y, K, D, 2, 1e-3, 1e-10)
    assert np.abs(Z - Zm).max() <= 1e-9 * np.abs(Zm).max()
    S = W.accumulate(Y, W.power(Y, 1e-10, dt), K, D, dt=dt)
    R, P = W.model_stats(Y, Y, K, D)
    L = M * K
    assert np.abs(W.cov_full(S[..., :L * L, :], L) - R).max() <= 1e-9 * np.abs(R).max()
    Pp = S[..., L * L:, :].reshape(2, L, M, 2, bins)
    Pc = np.moveaxis(Pp[..., 0, :] + 1j * Pp[..., 1, :], -1, -3)
    assert np.abs(Pc - P).max() <= 1e-9 * np.abs(P).max()
    out, Q, G = W.rls(Y, W.eye_cov((2,), M, K, bins, dt), np.zeros((2, L, M, bins), np.complex128), K, D, 0.99, dt=dt)
    om, Qm, Gm = W.model_rls(Y, K, D, 0.99)
    assert np.abs(out - om).max() <= 1e-9 * np.abs(om).max()
    assert np.abs(W.cov_full(Q, L) - Qm).max() <= 1e-9 * np.abs(Qm).max()
    assert np.abs(np.moveaxis(G, -1, -3) - Gm).max() <= 1e-9 * max(1.0, np.abs(Gm).max())


def test_a_cut_changes_no_bit_of_the_restatement():
    M, K, D, F, bins = 3, 2, 2, 9, 7
    Y = spectra((2,), M, F, bins).astype(np.complex64)
    io = W.power(Y)
    S = W.accumulate(Y, io, K, D)
    L = M * K
    out, Q, G = W.rls(Y, W.eye_cov((2,), M, K, bins), np.zeros((2, L, M, bins), np.complex64), K, D, 0.99)
    for cut in range(1, F):
        S2 = W.accumulate(Y, io, K, D, cut, F, state=W.accumulate(Y, io, K, D, 0, cut))
        assert np.array_equal(S.view(np.int32), S2.view(np.int32))
        o1, Q1, G1 = W.rls(Y, W.eye_cov((2,), M, K, bins), np.zeros((2, L, M, bins), np.complex64), K, D, 0.99, f1=cut)
        o2, Q2, G2 = W.rls(Y, Q1, G1, K, D, 0.99, f0=cut)
        assert np.array_equal(np.concatenate([o1, o2], axis=-2).view(np.float32).view(np.int32),
                              out.view(np.float32).view(np.int32))
        assert np.array_equal(Q2.view(np.int32), Q.view(np.int32))
        assert np.array_equal(G2.view(np.float32).view(np.int32), G.view(np.float32).view(np.int32))
    # pass-through: zero taps give the input back
    assert np.array_equal(W.filt(Y, np.zeros((2, L, M, bins), np.complex64), K, D), Y)


# ------------------------------------------------------------------ the scene
N, H, D = 512, 128, 3
_scene = {}


def scene_spectra(M):
    if M not in _scene:
        x, e = W.scene(M, early=D * H)
        w = W.hann(N)
        _scene[M] = (W.stft(x, N, H, w), W.stft(e, N, H, w))
    return _scene[M]


MEASURED = W.MEASURED


def rel(a, b):
    return float(np.abs(np.asarray(a, np.complex128) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("M,K", [(2, 10), (4, 8)])
def test_scene_offline(M, K):
    Y, E = scene_spectra(M)
    Ys = Y
    Zm = W.model_offline(Ys, K, D, 3)
    before, after = W.error_db(Ys, E), W.error_db(Zm, E)
    print(f"offline M={M} K={K}: before {before:.2f} dB, after {after:.2f} dB")
    assert after < before - 3.0
    Y32 = Ys.astype(np.complex64)
    S32 = W.accumulate(Y32, W.power(Y32), K, D)
    R, P = W.model_stats(Y32, Y32, K, D)
    L = M * K
    e_state = rel(W.cov_full(S32[..., :L * L, :], L), R)
    Z32 = W.dereverb_spec(Y32, K, D, 3)
    e_out = rel(Z32, W.model_offline(Y32, K, D, 3))
    print(f"  float32 restatement against the model: state {e_state:.2e}, output {e_out:.2e}")
    assert abs(W.error_db(Z32, E) - after) <= 1.0
    if (M, K) == (2, 10):  # the configuration the figures were taken at
        assert e_state <= 1.5 * MEASURED["offline_state"] and e_out <= 1.5 * MEASURED["offline_out"]


def test_scene_rls():
    M, K, alpha = 2, 10, 0.999
    Y, E = scene_spectra(M)
    F = Y.shape[-2]
    half = slice(F // 2, None)
    om, Qm, _ = W.model_rls(Y, K, D, alpha)
    before, after = W.error_db(Y, E, half), W.error_db(om, E, half)
    print(f"rls M={M} K={K}: before {before:.2f} dB, after {after:.2f} dB")
    assert after < before - 2.0
    Y32 = Y.astype(np.complex64)
    bins, L = Y.shape[-1], M * K
    o32, Q32, _ = W.rls(Y32, W.eye_cov((), M, K, bins), np.zeros((L, M, bins), np.complex64), K, D, alpha)
    o64, Q64, _ = W.model_rls(Y32, K, D, alpha)
    e_out, e_cov = rel(o32, o64), rel(W.cov_full(Q32, L), Q64)
    print(f"  float32 restatement against the model: output {e_out:.2e}, Q {e_cov:.2e}")
    assert abs(W.error_db(o32, E, half) - after) <= 1.0
    assert e_out <= 1.5 * MEASURED["rls_out"] and e_cov <= 1.5 * MEASURED["rls_cov"]
