"""CPU checks of the beamformer's numpy reference (tests/beamform_reference.py) on the
synthetic array of the contract's tests: a white target and a white interferer gated per
hop at random, integer delays (3m) mod 7 and (5m + 2) mod 11, sensor noise 0.05, periodic
Hann, 60 frames, an ideal-ratio mask at microphone 0, loading 1e-3.

The float32 restatement against the float64 model of the same algorithm on numpy's FFT, at
256/128, 512/128, 1024/256 with M = 2, 4, 8, both averaging modes and both solve modes
(condition numbers of A up to 6.7e3).  Measured, and the bars at 4 x the largest figure:
  planes, of a matrix's largest plane value        3.7e-7  -> 1.5e-6
  weights, of the largest weight                   1.75e-4 -> 7e-4
  |sum conj(w_m) d_m - 1| (STEERED, distortionless) 1.25e-6 -> 5e-6
The SINR at the output is 7.0 - 15.7 dB above microphone 0's in the float64 model, and the
float32 weights give the same figure to 0.01 dB; asserted: at least the model's own figure
minus 1 dB (and that the model improves on microphone 0 at all).  Delay-and-sum weights
pass the target through at the model's gain.  A run cut anywhere and carried equals the
uncut run bit for bit; groups in a batch and a shared mask equal each alone; the plane
order, the targets and the clamps; the float64 model against numpy's own solve."""
import numpy as np
import pytest

import beamform_reference as R

SHAPES = [(256, 128), (512, 128), (1024, 256)]
MICS = (2, 4, 8)
BAR_PLANES, BAR_WEIGHTS, BAR_DISTORTIONLESS = 1.5e-6, 7e-4, 5e-6

_scenes = {}


def scene(M, N, H):
    """(X, S, V, mask): float64 spectra (M, 60, bins) of the microphones, their target and
    interferer-plus-noise parts, and the ideal-ratio mask; computed once."""
    if (M, N, H) not in _scenes:
        x, s, v = R.scene(M, N, H)
        w = R.hann(N)
        X, S, V = (R.stft(a, N, H, w) for a in (x, s, v))
        out = (X, S, V, R.ideal_ratio_mask(S, V))
        for a in out:
            a.setflags(write=False)
        _scenes[(M, N, H)] = out
    return _scenes[(M, N, H)]


def c64(X):
    return X.astype(np.complex64)


def bits(a):
    a = np.asarray(a)
    if a.dtype.kind == "c":
        a = np.ascontiguousarray(a, np.complex64).view(np.float32)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("alpha", [0.0, 0.9])
@pytest.mark.parametrize("M", MICS)
@pytest.mark.parametrize("N,H", SHAPES)
def test_float32_restatement_against_float64(N, H, M, alpha):
    X, S, V, mask = scene(M, N, H)
    st64 = R.accumulate(X, mask, 0, alpha, np.float64)
    st32 = R.accumulate(c64(X), mask.astype(np.float32), 0, alpha)
    assert st32.dtype == np.float32 and st32.shape == (2, M * M, N // 2 + 1)
    planes = max(np.abs(st32[m].astype(np.float64) - st64[m]).max() / np.abs(st64[m]).max() for m in range(2))
    steer = R.steering_from_delays(R.target_delays(M) - R.target_delays(M)[0], N)
    print(f"{N}/{H} M={M} alpha={alpha}: planes {planes:.2e} of their maximum")
    assert planes <= BAR_PLANES
    for mode in (R.SOUDEN, R.STEERED):
        w64 = R.solve(st64, M, 0, mode, 1e-3, steer.astype(np.complex128), np.float64)
        w32 = R.solve(st32, M, 0, mode, 1e-3, steer)
        assert w32.dtype == np.complex64 and w32.shape == (M, N // 2 + 1)
        dw = np.abs(w32 - w64).max() / np.abs(w64).max()
        g64, g32 = R.sinr_gain_db(S, V, w64), R.sinr_gain_db(S, V, w32)
        print(f"  mode {mode}: weights {dw:.2e} of the largest, SINR gain {g64:.2f} dB (float64) {g32:.2f} dB (float32)")
        assert dw <= BAR_WEIGHTS
        assert g32 >= g64 - 1.0
        assert g64 > 0.0
        if mode == R.STEERED:
            dist = np.abs((np.conj(w32.astype(np.complex128)) * steer).sum(0) - 1).max()
            print(f"  distortionless within {dist:.2e}")
            assert dist <= BAR_DISTORTIONLESS


@pytest.mark.parametrize("M", MICS)
def test_delay_and_sum_passes_the_target_at_the_models_gain(M):
    N, H = 512, 128
    X, S, V, _ = scene(M, N, H)
    delays = R.target_delays(M) - R.target_delays(M)[0]
    w = R.delay_and_sum(delays, N)
    # the model: a target delayed by an integer number of samples, undone by the weights, is
    # microphone 0's target up to the frame's edge effect (the window sees a shifted signal)
    y64 = R.apply(S, w.astype(np.complex128), np.float64)
    y32 = R.apply(c64(S), w)
    gain64 = np.sqrt((np.abs(y64) ** 2).sum() / (np.abs(S[0]) ** 2).sum())
    gain32 = np.sqrt((np.abs(y32.astype(np.complex128)) ** 2).sum() / (np.abs(S[0]) ** 2).sum())
    print(f"M={M}: target gain {gain64:.4f} (float64) {gain32:.4f} (float32)")
    assert abs(gain64 - 1.0) <= 0.05  # six samples of misalignment at most under a 512-sample window
    # float32: the rounding of the inputs, M products and M sums per component, each within
    # 2^-23 of the magnitudes summed
    bound = (M + 4) * 2.0 ** -23 * (np.abs(w)[:, None, :] * np.abs(S)).sum(0).max()
    assert np.abs(y32 - y64).max() <= bound
    assert abs(gain32 - gain64) <= 1e-5


@pytest.mark.parametrize("alpha", [0.0, 0.9])
@pytest.mark.parametrize("target", [0, 1, 2])
def test_cut_and_carry_equals_the_uncut_run(alpha, target):
    X, _, _, mask = scene(4, 256, 128)
    X, mask = c64(X[:, :26]), mask[:26].astype(np.float32)
    st = R.accumulate(X, mask, target, alpha)
    for F1 in range(1, 26):
        sa = R.accumulate(X[:, :F1], mask[:F1], target, alpha)
        sb = R.accumulate(X[:, F1:], mask[F1:], target, alpha, state=sa)
        assert np.array_equal(bits(sb), bits(st)), F1


def test_groups_and_a_shared_mask_equal_each_alone():
    X, _, _, mask = scene(4, 256, 128)
    X, mask = c64(X[:, :12]), mask[:12].astype(np.float32)
    X3 = np.stack([X, X * np.float32(0.25), X[::-1].copy()])
    m3 = np.stack([mask, mask * np.float32(0.5), mask[::-1].copy()])
    s3 = R.accumulate(X3, m3, 0, 0.9)
    assert s3.shape == (3, 2, 16, 129)
    for g in range(3):
        assert np.array_equal(bits(s3[g]), bits(R.accumulate(X3[g], m3[g], 0, 0.9))), g
    shared = R.accumulate(X3, mask, 0, 0.9)
    assert np.array_equal(bits(shared), bits(R.accumulate(X3, np.stack([mask] * 3), 0, 0.9)))
    w3 = R.solve(s3, 4, 1)
    for g in range(3):
        assert np.array_equal(bits(w3[g]), bits(R.solve(s3[g], 4, 1))), g
    y3 = R.apply(X3, w3)
    for g in range(3):
        assert np.array_equal(bits(y3[g]), bits(R.apply(X3[g], w3[g]))), g


def test_plane_order_targets_and_factors():
    assert [R.re_plane(3, i, j) for i in range(3) for j in range(i + 1, 3)] == [3, 5, 7]
    assert R.re_plane(8, 6, 7) == 62 and R.planes(8) == 64
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((3, 5, 7)) + 1j * rng.standard_normal((3, 5, 7))).astype(np.complex64)
    mask = rng.random((5, 7)).astype(np.float32)
    both = R.accumulate(X, mask, 0)
    # Welch: the planes are plain sums in frame order of the weighted terms
    want = np.zeros(7, np.float32)
    for f in range(5):
        want = want + mask[f] * ((X[0, f].real * X[0, f].real) + (X[0, f].imag * X[0, f].imag))
    assert np.array_equal(both[0, 0], want)
    k = R.re_plane(3, 0, 2)
    P64 = (X[0].astype(np.complex128) * np.conj(X[2].astype(np.complex128)) * mask).sum(0)
    assert np.allclose(both[0, k], P64.real, rtol=1e-5, atol=1e-5) and np.allclose(both[0, k + 1], P64.imag, rtol=1e-5, atol=1e-5)
    assert np.array_equal(R.accumulate(X, mask, 1)[0], both[0]) and np.all(R.accumulate(X, mask, 1)[1] == 0)
    noise_only = R.accumulate(X, mask, 2)
    assert np.all(noise_only[0] == 0) and np.array_equal(noise_only[1], both[0])  # weight mu on the noise matrix
    assert np.array_equal(R.accumulate(X, np.float32(1) - mask, 2)[1], R.accumulate(X, np.float32(1) - mask, 1)[0])
    ones = R.accumulate(X, None, 2)
    assert np.array_equal(ones[1], R.accumulate(X, np.ones((5, 7), np.float32), 2)[1])
    with pytest.raises(ValueError):
        R.accumulate(X, None, 0)
    # the Hermitian matrix of the planes is the mask-weighted sum of outer products
    A = R.matrix(both[0], 3)
    Xd = X.astype(np.complex128)
    want = np.einsum("ifb,jfb,fb->bij", Xd, np.conj(Xd), mask.astype(np.float64))
    assert np.allclose(A, want, rtol=1e-4, atol=1e-4)


def test_zero_state_clamps_at_tiny_and_passthrough():
    st = np.zeros((2, 9, 5), np.float32)
    for mode in (R.SOUDEN, R.STEERED):
        w = R.solve(st, 3, 1, mode, 1e-3, np.ones((3, 5), np.complex64))
        assert np.all(np.isfinite(w.view(np.float32)))
    assert np.all(R.solve(st, 3, 1, R.SOUDEN) == 0)
    W = R.passthrough(3, 5, ref=2)
    X = (np.arange(3 * 4 * 5).reshape(3, 4, 5) + 1j).astype(np.complex64)
    assert np.array_equal(R.apply(X, W), X[2])


def test_solve_is_the_mvdr_solution_in_float64():
    """The float64 model against numpy's own solve: w = A^-1 Phi_s e_ref / tr(A^-1 Phi_s) and
    A^-1 d / (d^H A^-1 d)."""
    M, N, H = 4, 256, 128
    X, S, V, mask = scene(M, N, H)
    st = R.accumulate(X, mask, 0, 0.0, np.float64)
    Ps, Pn = R.matrix(st[0], M), R.matrix(st[1], M)
    A = Pn + 1e-3 * (np.trace(Pn, axis1=-2, axis2=-1).real / M)[:, None, None] * np.eye(M)
    G = np.linalg.solve(A, Ps)
    want = (G[:, :, 1] / np.trace(G, axis1=-2, axis2=-1)[:, None].real).T
    got = R.solve(st, M, 1, R.SOUDEN, 1e-3, None, np.float64)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    d = R.steering_from_delays(R.target_delays(M), N).astype(np.complex128)
    y = np.linalg.solve(A, d.T[:, :, None])[:, :, 0]
    want = (y / np.einsum("bm,bm->b", np.conj(d.T), y).real[:, None]).T
    got = R.solve(st, M, 0, R.STEERED, 1e-3, d, np.float64)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
