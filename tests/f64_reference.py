"""A float64 restatement of the masked round trip, and the block-local metric.

Test helper (a plain module, no fixtures).  `roundtrip_f64` restates
oracle/crlot_oracle.c:or_roundtrip_impl in numpy float64 for ZERO_PAD and DROP
framing and the symmetric Hann window:

    frame -> * w -> rfft -> * gain -> * mask[k] -> irfft -> * w -> add at k H

and block k (output samples [k H, (k + 1) H)) divided by
`oracle.norm_table(w32, n, h)[i mod ring_len]` widened to float64 and floored at
eps = 1e-8: the reference's sum-of-*window* table with its ring wrap, NOT the
sum of w^2.  The window is the oracle's float32 table widened, so the only
difference from the oracle is the float32 rounding of its arithmetic (and its
sanitize, |v| < 1e-30 -> 0, which none of the inputs below comes near).

The metric.  With nb = ceil(N / H), output block b is covered by the frames
C_b = [max(0, b - nb + 1), b].  `fs[k]` = max |irfft output of frame k| is the
scale of a frame;

    own_b  = max fs[C_b]
    pair_b = max fs[k] over k in C_b and their pair mates k ^ 1 < F

`local_err(y, y_ref, scale, h)` = max over blocks with scale_b > 0 of
max|y - y_ref| over the block / scale_b, and `silent_blocks(own)` = the blocks
with own_b == 0: every frame that reaches them is exactly zero, and the
reference chain returns +0 there.

The second half builds the inputs the block-local tests share (shapes, streams
with level steps and exact silence, gate masks), so the CPU test can prove them
fair against the oracle before any GPU test uses them.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle as O  # noqa: E402

ZERO_PAD, DROP = 0, 1
EPS = 1e-8


# ------------------------------------------------------------------ the reference
def window32(n):
    """The oracle's symmetric Hann table (float32)."""
    return O.window(O.HANN, n)


def frame_count(T, n, h, mode=ZERO_PAD):
    if T == 0:
        return 0
    if mode == ZERO_PAD:
        return -(-T // h)
    return 0 if T < n else (T - n) // h + 1


def frames_f64(x, n, h, mode=ZERO_PAD):
    """(F, n) float64 frames of x: frame k starts at k h; ZERO_PAD pads the tail."""
    x = np.asarray(x, np.float64)
    F = frame_count(x.size, n, h, mode)
    xp = np.concatenate([x, np.zeros(n)])
    idx = np.arange(F)[:, None] * h + np.arange(n)[None, :]
    return xp[idx]


def stft_f64(x, n, h, mode=ZERO_PAD):
    """(F, n/2+1) complex128: rfft(frame * w), the spectra before the step."""
    w = window32(n).astype(np.float64)
    return np.fft.rfft(frames_f64(x, n, h, mode) * w, axis=1)


def istft_ola_f64(spec, n, h):
    """Stepped spectra (F, n/2+1) -> (y_ref of length F h, fs): irfft (the imaginary
    parts of DC and Nyquist ignored, as kiss_fftri), synthesis window, overlap-add,
    the norm-table division."""
    spec = np.asarray(spec, np.complex128)
    F = spec.shape[0]
    w32 = window32(n)
    w = w32.astype(np.float64)
    t = np.fft.irfft(spec, n=n, axis=1)
    fs = np.max(np.abs(t), axis=1) if F else np.zeros(0)
    acc = np.zeros(F * h + n)
    tw = t * w
    for k in range(F):
        acc[k * h:k * h + n] += tw[k]
    norm = O.norm_table(w32, n, h).astype(np.float64)
    d = np.maximum(norm, EPS)
    y = acc[:F * h] / d[np.arange(F * h) % norm.size]
    return y, fs


def roundtrip_f64(x, n, h, gain=None, mask=None, mode=ZERO_PAD):
    """One stream x (T,), gain (n/2+1) or None, mask (F, n/2+1) or None ->
    (y_ref (F h,), fs (F,))."""
    spec = stft_f64(x, n, h, mode)
    if gain is not None:
        spec = spec * np.asarray(gain, np.float64)[None, :]
    if mask is not None:
        spec = spec * np.asarray(mask, np.float64)[:spec.shape[0]]
    return istft_ola_f64(spec, n, h)


# ------------------------------------------------------------------ the metric
def _cover_max(v, nb):
    """max of v over [max(0, b - nb + 1), b] for every b."""
    out = np.array(v, np.float64)
    for j in range(1, nb):
        out[j:] = np.maximum(out[j:], v[:len(v) - j])
    return out


def own_scale(fs, n, h):
    return _cover_max(np.asarray(fs, np.float64), -(-n // h))


def pair_scale(fs, n, h):
    fs = np.asarray(fs, np.float64)
    F = fs.size
    mate = np.arange(F) ^ 1
    withmate = np.maximum(fs, np.where(mate < F, fs[np.minimum(mate, F - 1)], 0.0))
    return _cover_max(withmate, -(-n // h))


def block_err(y, y_ref, h):
    d = np.abs(np.asarray(y, np.float64) - np.asarray(y_ref, np.float64))
    return d.reshape(-1, h).max(axis=1)


def local_err(y, y_ref, scale, h):
    """max_b (max|y - y_ref| over block b / scale_b) over the blocks with scale_b > 0."""
    e = block_err(y, y_ref, h)
    live = scale > 0
    return float(np.max(e[live] / scale[live])) if live.any() else 0.0


def silent_blocks(own):
    return np.nonzero(np.asarray(own) == 0)[0]


def silent_is_plus_zero(y, own, h):
    """True when every sample of every silent block of y has the bits of +0."""
    b = np.ascontiguousarray(y, np.float32).view(np.uint32).reshape(-1, h)
    return bool(np.all(b[silent_blocks(own)] == 0))


# ------------------------------------------------------------------ shared inputs
# one shape per walker family, smallest sizes
SHAPES = [(512, 128), (1024, 128), (1024, 256), (1024, 512), (2048, 512), (4096, 1024),
          (480, 120), (960, 240), (882, 441), (1764, 441), (1000, 250), (1920, 480)]
S = 4
GATE_VALUES = (0.0, 2.0 ** -12, 2.0 ** -24)
MASK_KINDS = ("shared", "per_stream")


def stream_len(n, h):
    return (12 if n // h >= 4 else 24) * n + h // 3


def make_streams(n, h):
    """(4, T) float32: s0 plain; s1 with level steps of 2^-24 and 2^12; s2 with exact
    leading silence whose onset is on the pair mate's last hop, and a silent gap; s3
    plain (the stream the gates apply to)."""
    T = stream_len(n, h)
    x = O.synth_streams(S, T, config_id=90).copy()
    x[1, 5 * n:6 * n] *= np.float32(2.0 ** -24)
    x[1, 8 * n:8 * n + 3 * h] *= np.float32(2.0 ** 12)
    x[2, :8 * h + n] = 0.0
    x[2, 30 * h + n:33 * h + n] = 0.0
    return x


def gate_rows(F, shift=0):
    rows = list(range(9, 20)) + [30] + list(range(41, 44))
    return np.array([r + shift for r in rows if 0 <= r + shift < F], np.int64)


def make_mask(n, F, v, kind):
    """Ones with the gate rows set to v.  "shared": (F, bins), every stream gated on
    rows [9, 20), {30}, [41, 44); "per_stream": (S, F, bins), s3 gated on those rows,
    s0 on the same rows shifted by one frame (the other parity of starts), s1 and s2
    left open."""
    bins = n // 2 + 1
    if kind == "shared":
        m = np.ones((F, bins), np.float32)
        m[gate_rows(F)] = v
        return m
    m = np.ones((S, F, bins), np.float32)
    m[3, gate_rows(F)] = v
    m[0, gate_rows(F, 1)] = v
    return m


def stream_mask(mask, s):
    return mask if mask.ndim == 2 else mask[s]


def make_gain(n):
    k = np.arange(n // 2 + 1)
    return (1.0 + 0.5 * np.cos(0.05 * k)).astype(np.float32)


def gated_spectra(x, n, h):
    """Hand-built spectra (S, F, bins) complex64: the float64 forward spectra rounded
    to float32, the gate rows (s3 as "shared", s0 shifted by one) exact zeros."""
    spec = np.stack([stft_f64(x[s], n, h) for s in range(x.shape[0])]).astype(np.complex64)
    F = spec.shape[1]
    spec[3, gate_rows(F)] = 0
    spec[0, gate_rows(F, 1)] = 0
    return spec
