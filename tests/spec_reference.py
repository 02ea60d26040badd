"""The frame-local spectral metric, and the streams the spectral tests share.

Test helper (a plain module, no fixtures), beside tests/f64_reference.py, whose
names it re-exports (`stft_f64`, `frame_count`, `SHAPES`, `make_streams`, the
block-local metric ...), so a test imports this module alone.

The spectral metric is the block-local idea one stage earlier: a forward spectrum
(`stft_f64`) is judged frame by frame.  `spec_peak` = max_b |X64[k, b]| is a frame's
own scale, `spec_pair_peak` the larger of it and the pair mate's when frame k ^ 1
exists; `spec_local_err(X, X64, scale)` and `spec_frame_l2` are the per-frame
peak-relative and rel-L2 errors, `silent_frames` / `silent_spec_is_zero` the frames
whose input is exact silence and the check that they are zero by value;
`spec_bars` gives the bars, which follow the oracle's own figure only where the
transform needs a generic butterfly (a prime factor > 7).

`make_spec_streams` / `make_tail_streams` build the inputs, so the CPU test
(tests/test_spec_reference.py) can prove them fair against the oracle before any
GPU test uses them.
"""
import numpy as np

from f64_reference import *  # noqa: F401,F403  (the float64 reference, the block-local metric, the shared inputs)
from f64_reference import DROP, SHAPES, O, frame_count, make_streams


# ------------------------------------------------------------------ the spectral metric
# The frequency-domain counterpart of the block-local metric: a forward spectrum is
# judged frame by frame against the frame's own scale ps[k] = max_b |X64[k, b]| (the
# reference transforms every frame alone), or with frame pairing on against the
# larger of its own and its pair mate's (frames k and k ^ 1 share one transform;
# pairs are aligned to even frame indices of the call, whatever the chunking).
SPEC_MAX_ABS = 4e-6   # the project's bars (tests/test_gpu_parity.py MAX_ABS, REL_L2)
SPEC_REL_L2 = 1e-6


def spec_peak(X64):
    """ps[k] = max_b |X64[k, b]|: the frame's own scale."""
    X64 = np.asarray(X64, np.complex128)
    return np.max(np.abs(X64), axis=1) if X64.shape[0] else np.zeros(0)


def _with_mate(v):
    v = np.asarray(v, np.float64)
    F = v.size
    mate = np.arange(F) ^ 1
    return np.maximum(v, np.where(mate < F, v[np.minimum(mate, F - 1)], 0.0)) if F else v


def spec_pair_peak(ps):
    """max(ps[k], ps[k ^ 1]) when k ^ 1 < F, otherwise ps[k]."""
    return _with_mate(ps)


def spec_frame_err(X, X64):
    """max_b |X[k, b] - X64[k, b]| per frame."""
    return np.max(np.abs(np.asarray(X, np.complex128) - np.asarray(X64, np.complex128)), axis=1)


def spec_local_err(X, X64, scale):
    """max over the frames with scale_k > 0 of max_b |X[k, b] - X64[k, b]| / scale_k."""
    scale = np.asarray(scale, np.float64)
    live = scale > 0
    return float(np.max(spec_frame_err(X, X64)[live] / scale[live])) if live.any() else 0.0


def spec_frame_l2(X, X64, pair=False):
    """max over the frames with L_k > 0 of ||X[k] - X64[k]||_2 / L_k; L_k = ||X64[k]||_2,
    with `pair` the larger of the frame's and its mate's."""
    X64 = np.asarray(X64, np.complex128)
    L = np.linalg.norm(X64, axis=1)
    if pair:
        L = _with_mate(L)
    d = np.linalg.norm(np.asarray(X, np.complex128) - X64, axis=1)
    live = L > 0
    return float(np.max(d[live] / L[live])) if live.any() else 0.0


def silent_frames(ps):
    """The frames whose float64 spectrum is all zero (every windowed sample is zero)."""
    return np.nonzero(np.asarray(ps) == 0)[0]


def silent_spec_is_zero(X, ps):
    """True when every re and im of every silent frame of X compares equal to 0 (the
    sign is free: the reference's kiss_fftr leaves -0 in some slots of a zero frame)."""
    rows = np.asarray(X)[silent_frames(ps)]
    return bool(np.all(rows.real == 0) and np.all(rows.imag == 0))


def lone_silent_frames(ps):
    """The silent frames whose pair mate k ^ 1 exists and is live."""
    ps = np.asarray(ps)
    return [int(k) for k in silent_frames(ps) if (k ^ 1) < ps.size and ps[k ^ 1] > 0]


def largest_prime_factor(m):
    p, best = 2, 1
    while p * p <= m:
        while m % p == 0:
            best, m = p, m // p
        p += 1
    return max(best, m) if m > 1 else best


def generic_butterfly(m):
    """True when a length-m complex transform needs a butterfly beyond radix 2/3/4/5/7
    (kissfft's generic O(R^2) one): its summation error grows with the factor R and its
    order of additions is the implementation's own, so no bar is fixed in advance."""
    return largest_prime_factor(m) > 7


def spec_bars(m, oracle_local=0.0, oracle_l2=0.0):
    """(peak-relative bar, rel-L2 bar) for a transform whose complex length is m (N / 2
    for a real transform of N): the project's bars; where m needs the generic
    butterfly, the larger of them and 4x the oracle's figure on the same input and metric."""
    if not generic_butterfly(m):
        return SPEC_MAX_ABS, SPEC_REL_L2
    return max(SPEC_MAX_ABS, 4.0 * oracle_local), max(SPEC_REL_L2, 4.0 * oracle_l2)


SPEC_SHAPES = SHAPES + [(256, 128), (1536, 384), (998, 499)]
SPEC_S = 6
LONE_SILENT = ((2, 8), (5, 20), (5, 41))   # (stream, frame): s2's onset, the two gaps


def make_spec_streams(n, h):
    """(6, T) float32: make_streams' four, then
    tones -- 0.5 cos(2 pi (n // 8) t / n) on [0, T/2) (exactly on a bin), 0.5 cos(2 pi
      (n / 8 + 0.37) t / n) + 0.25 on [T/2, 3T/4) (off-bin, plus DC), 0.4 (-1)^t on
      [3T/4, T) (the Nyquist bin); computed in float64, then rounded;
    gaps -- a plain stream with x[20h : 20h + n] = 0 and x[41h : 41h + n] = 0: exactly one
      silent frame with an even index (20, mate 21 live) and one with an odd index (41,
      mate 40 live).
    With s2's leading silence (frame 8 silent, 9 live) the lone silent frames LONE_SILENT
    exist at every shape and in both framings."""
    x4 = make_streams(n, h)
    T = x4.shape[1]
    t = np.arange(T, dtype=np.float64)
    a, b = T // 2, (3 * T) // 4
    tones = np.where(t < a, 0.5 * np.cos(2 * np.pi * (n // 8) * t / n),
                     np.where(t < b, 0.5 * np.cos(2 * np.pi * (n / 8 + 0.37) * t / n) + 0.25,
                              0.4 * (1.0 - 2.0 * (t % 2))))
    gaps = O.synth_streams(1, T, config_id=91)[0].copy()
    gaps[20 * h:20 * h + n] = 0.0
    gaps[41 * h:41 * h + n] = 0.0
    return np.concatenate([x4, tones.astype(np.float32)[None], gaps[None]]).astype(np.float32)


TAIL_GAIN = 2.0 ** 12
TAIL_SILENT = 3   # the stream whose last DROP frame is silenced


def make_tail_streams(n, h):
    """make_spec_streams for DROP framing, with the samples after the last frame's end --
    they belong to no frame -- 2^12 louder, and stream 3's last frame exact silence: the
    last frame of an odd frame count has no pair mate, so it keeps its own scale, and a
    silent one is zeros, whatever follows it."""
    x = make_spec_streams(n, h)
    T = x.shape[1]
    F = frame_count(T, n, h, DROP)
    end = (F - 1) * h + n
    assert F % 2 == 1 and end < T
    x[:, end:] *= np.float32(TAIL_GAIN)
    x[TAIL_SILENT, (F - 1) * h:end] = 0.0
    return x
