"""The frame-local spectral metric (tests/spec_reference.py) and the oracle's own
forward spectra under it, on the CPU.

Proves the inputs and bars of tests/test_gpu_spectral_accuracy.py fair before any
GPU sees them: at every shape of SPEC_SHAPES, in ZERO_PAD and DROP framing, the
oracle's spectra (kiss_fftr of the windowed frame, float32) are
  * within 4e-6 of the float64 DFT frame by frame, against the frame's OWN peak
    (measured <= 2.93e-7, worst 256/128; 1.12e-6 at 998/499, whose half size 499
    is prime and goes through kissfft's generic O(R^2) butterfly),
  * within 1e-6 of it in per-frame rel-L2 (measured <= 1.58e-7; 5.18e-7 at 998/499),
  * zero by value on every silent frame (-0 occurs), with zero DC and Nyquist
    imaginary parts,
and the inputs hold the lone silent frames (s2, 8), (gaps, 20), (gaps, 41) -- both
parities -- so the zero-frame assertions of the GPU test cannot pass vacuously.
"""
import numpy as np
import pytest

import spec_reference as R


@pytest.mark.parametrize("mode", [R.ZERO_PAD, R.DROP], ids=["zero_pad", "drop"])
@pytest.mark.parametrize("n,h", R.SPEC_SHAPES)
def test_oracle_spectra_meet_frame_local_bars(oracle, n, h, mode):
    x = R.make_spec_streams(n, h)
    assert x.shape[0] == R.SPEC_S and x.dtype == np.float32
    F = R.frame_count(x.shape[1], n, h, mode)
    assert F >= 45 and oracle.frame_count(x.shape[1], n, h, mode) == F
    worst_loc = worst_l2 = 0.0
    minus_zero = 0
    for s in range(R.SPEC_S):
        _, X = oracle.roundtrip_mask(x[s], n, h, mode=mode, want_spec=True)
        X64 = R.stft_f64(x[s], n, h, mode)
        assert X.shape == X64.shape == (F, n // 2 + 1), (s, X.shape)
        ps = R.spec_peak(X64)
        loc = R.spec_local_err(X, X64, ps)
        l2 = R.spec_frame_l2(X, X64)
        worst_loc, worst_l2 = max(worst_loc, loc), max(worst_l2, l2)
        assert loc <= R.SPEC_MAX_ABS, f"{n}/{h} mode {mode} stream {s}: spec_local_err(own) {loc:.3e}"
        assert l2 <= R.SPEC_REL_L2, f"{n}/{h} mode {mode} stream {s}: per-frame rel-L2 {l2:.3e}"
        assert R.silent_spec_is_zero(X, ps), f"{n}/{h} mode {mode} stream {s}: a silent frame is not zero"
        assert np.all(X[:, 0].imag == 0) and np.all(X[:, -1].imag == 0), s
        # the pair scales can only be larger: the oracle meets those bars a fortiori
        assert R.spec_local_err(X, X64, R.spec_pair_peak(ps)) <= loc
        assert R.spec_frame_l2(X, X64, pair=True) <= l2
        sil = X[R.silent_frames(ps)]
        minus_zero += int(np.count_nonzero(np.signbit(sil.real) | np.signbit(sil.imag)))
        lone = R.lone_silent_frames(ps)
        for ss, k in R.LONE_SILENT:
            if ss == s:
                assert k in lone, f"{n}/{h} mode {mode}: frame {k} of stream {s} is not a lone silent frame"
        if s == 5:   # exactly the two gaps: an even and an odd index
            assert R.silent_frames(ps).tolist() == [20, 41]
        if s in (0, 1, 3, 4):
            assert R.silent_frames(ps).size == 0
    print(f"{n}/{h} mode {mode}: spec_local_err(own) <= {worst_loc:.2e}, per-frame rel-L2 <= {worst_l2:.2e}, "
          f"-0 slots in silent frames {minus_zero}")


@pytest.mark.parametrize("n,h", R.SPEC_SHAPES)
def test_tail_streams_reach_no_frame(oracle, n, h):
    """DROP framing: the loud samples after the last frame's end change no frame (the
    float64 spectra are those of the streams cut at that end, and the oracle's keep the
    bars), every stream's tail is live, and stream 3's last frame -- odd count, no mate --
    is silent."""
    x = R.make_tail_streams(n, h)
    T = x.shape[1]
    F = R.frame_count(T, n, h, R.DROP)
    end = (F - 1) * h + n
    assert F % 2 == 1 and end < T and R.frame_count(end, n, h, R.DROP) == F
    for s in range(R.SPEC_S):
        assert np.max(np.abs(x[s, end:])) >= 0.1 * R.TAIL_GAIN * np.max(np.abs(x[s, (F - 2) * h:(F - 1) * h])), s
        X64 = R.stft_f64(x[s], n, h, R.DROP)
        assert np.array_equal(X64, R.stft_f64(x[s, :end], n, h, R.DROP))
        ps = R.spec_peak(X64)
        assert (ps[F - 1] == 0) == (s == R.TAIL_SILENT) and ps[F - 2] > 0
        _, X = oracle.roundtrip_mask(x[s], n, h, mode=R.DROP, want_spec=True)
        assert R.spec_local_err(X, X64, ps) <= R.SPEC_MAX_ABS and R.spec_frame_l2(X, X64) <= R.SPEC_REL_L2
        assert R.silent_spec_is_zero(X, ps)


def test_spec_streams_layout():
    """The two added streams are what the docstring says, at a shape with an odd T."""
    n, h = 882, 441
    x = R.make_spec_streams(n, h)
    T = x.shape[1]
    assert T == R.stream_len(n, h) and np.array_equal(x[:4], R.make_streams(n, h))
    X64 = R.stft_f64(x[4], n, h)
    k = 3                                              # a frame inside the on-bin segment
    assert int(np.argmax(np.abs(X64[k]))) == n // 8
    k = (3 * T // 4) // h + 2                          # inside the Nyquist segment
    assert int(np.argmax(np.abs(X64[k]))) == n // 2
    g = x[5]
    assert not g[20 * h:20 * h + n].any() and not g[41 * h:41 * h + n].any()
    assert g[20 * h - 1] != 0 and g[20 * h + n] != 0 and g[41 * h - 1] != 0 and g[41 * h + n] != 0


def test_spectral_metric_on_a_hand_made_case():
    X64 = np.zeros((5, 3), np.complex128)
    X64[0] = [4.0, 0.0, 3.0j]          # peak 4, norm 5
    X64[1] = 0.0                        # silent, mate 0 live: a lone silent frame
    X64[2] = [0.5, 0.0, 0.0]
    X64[3] = [0.0, 2.0, 0.0]
    X64[4] = [1.0, 0.0, 0.0]            # the last frame of an odd count: no mate
    ps = R.spec_peak(X64)
    assert ps.tolist() == [4.0, 0.0, 0.5, 2.0, 1.0]
    assert R.spec_pair_peak(ps).tolist() == [4.0, 4.0, 2.0, 2.0, 1.0]
    assert R.spec_pair_peak(ps[:4]).tolist() == [4.0, 4.0, 2.0, 2.0]
    assert R.silent_frames(ps).tolist() == [1] and R.lone_silent_frames(ps) == [1]
    assert R.lone_silent_frames(np.array([0.0, 0.0, 1.0, 0.0, 0.0])) == [3]   # 0, 1 both silent; 4 has no mate
    X = X64.copy()
    X[2, 1] += 0.25                     # frame 2: own scale 0.5, pair scale 2
    X[1, 2] = 9.0                       # a silent frame: not in spec_local_err under `own`
    assert R.spec_local_err(X, X64, ps) == 0.5
    assert R.spec_local_err(X, X64, R.spec_pair_peak(ps)) == 9.0 / 4.0
    X[1, 2] = 0.0
    assert R.spec_local_err(X, X64, R.spec_pair_peak(ps)) == 0.125
    assert R.spec_frame_l2(X, X64) == 0.5 and R.spec_frame_l2(X, X64, pair=True) == 0.125
    X[0, 1] = 0.5j                      # frame 0: norm 5
    assert R.spec_frame_l2(X, X64, pair=True) == 0.125 and R.spec_local_err(X, X64, ps) == 0.5
    X[0, 1] = 5.0
    assert R.spec_frame_l2(X, X64) == 1.0
    # silent frames: zero by value, either sign; anything else is a miss
    Z = X64.astype(np.complex64)
    assert R.silent_spec_is_zero(Z, ps)
    Z[1] = np.complex64(complex(-0.0, -0.0))
    assert R.silent_spec_is_zero(Z, ps)
    Z[1, 2] = np.complex64(1e-30j)
    assert not R.silent_spec_is_zero(Z, ps)
    Z[1, 2] = np.complex64(complex(np.nan, 0.0))
    assert not R.silent_spec_is_zero(Z, ps)


def test_bars_for_sizes_with_a_generic_butterfly():
    assert [R.largest_prime_factor(m) for m in (1, 2, 12, 441, 499, 960, 2205)] == [1, 2, 3, 7, 499, 5, 7]
    assert R.spec_bars(512, 1.0, 1.0) == (R.SPEC_MAX_ABS, R.SPEC_REL_L2)    # smooth: fixed, whatever the oracle does
    assert R.spec_bars(499, 1.12e-6, 5.18e-7) == (4 * 1.12e-6, 4 * 5.18e-7)
    assert R.spec_bars(499, 1e-7, 1e-7) == (R.SPEC_MAX_ABS, R.SPEC_REL_L2)  # never below the project's bars
    assert [n for n, _ in R.SPEC_SHAPES if R.generic_butterfly(n // 2)] == [998]
