"""Two independent restatements of the phase vocoder (include/crlot_dsp.h, "time
stretch") for the tests, numpy only:

reference(X, rate)   the torchaudio.functional.phase_vocoder recurrence in float64,
                     in its explicit form: the expected phase advance is subtracted,
                     the difference wrapped to [-pi, pi] and the advance added back,
                     then a float64 cumulative sum.  (So a test against it also shows
                     that advance and wrap cancel modulo 2 pi.)
emulate(X, rate)     the header's contract in float32 with a uint32 phase
                     accumulator, numpy's own atan2 / sqrt / sin / cos.
frame_count(F, rate) the number of t >= 0 with t * rate < F.

Spectra are (..., F, bins) complex arrays, time on the second-to-last axis.
Inputs are sanitized as the kernels sanitize them on load (NaN / Inf -> 0,
|v| < 1e-30 -> 0) in both.
"""
import numpy as np

RATES = (0.5, 0.75, 1.0, 1.3, 2.0, 3.7)


def frame_count(F, rate):
    F, rate = int(F), float(rate)
    if F <= 0:
        return 0
    n = int(np.ceil(F / rate))
    while n > 0 and float(n - 1) * rate >= F:
        n -= 1
    while float(n) * rate < F:
        n += 1
    return n


def steps(F, rate):
    """i_t (int64) and alpha_t (float32) of the F' output frames."""
    tau = np.arange(frame_count(F, rate), dtype=np.float64) * float(rate)
    i = np.floor(tau)
    return i.astype(np.int64), (tau - i).astype(np.float32)


def sanitize(X):
    X = np.asarray(X, np.complex64)
    re, im = X.real.copy(), X.imag.copy()
    for v in (re, im):
        with np.errstate(invalid="ignore"):
            v[~(np.isfinite(v) & (np.abs(v) >= np.float32(1e-30)))] = 0.0
    bins = X.shape[-1]
    im[..., 0] = 0.0  # bins 0 and N/2: the imaginary part is ignored
    im[..., bins - 1] = 0.0
    return re, im


def _padded(a, F):
    """(..., F, bins) -> (..., F + 1, bins): the frame with index F is all zeros."""
    pad = [(0, 0)] * a.ndim
    pad[-2] = (0, 1)
    return np.pad(a, pad)


def own_scale(X, rate):
    """max(|X[i_t]|, |X[i_t + 1]|) per output element, float64: the scale an
    element's error is measured against."""
    re, im = sanitize(X)
    mag = _padded(np.hypot(re.astype(np.float64), im.astype(np.float64)), X.shape[-2])
    i, _ = steps(X.shape[-2], rate)
    return np.maximum(np.take(mag, i, axis=-2), np.take(mag, i + 1, axis=-2))


def reference(X, rate, hop=None):
    re, im = sanitize(X)
    F, bins = X.shape[-2], X.shape[-1]
    Z = _padded(re.astype(np.float64) + 1j * im.astype(np.float64), F)
    i, _ = steps(F, rate)
    tau = np.arange(len(i), dtype=np.float64) * float(rate)
    al = (tau - np.floor(tau))[:, None]
    Z0, Z1 = np.take(Z, i, axis=-2), np.take(Z, i + 1, axis=-2)
    hop = (bins - 1) // 2 if hop is None else hop
    adv = np.linspace(0.0, np.pi * hop, bins)
    ph = np.angle(Z1) - np.angle(Z0) - adv
    ph = ph - 2.0 * np.pi * np.round(ph / (2.0 * np.pi))
    ph = ph + adv
    first = np.angle(np.take(Z, [0], axis=-2))
    ph = np.concatenate([first, np.delete(ph, -1, axis=-2)], axis=-2)
    acc = np.cumsum(ph, axis=-2)
    mag = al * np.abs(Z1) + (1.0 - al) * np.abs(Z0)
    return mag * np.exp(1j * acc)


K_TURN32 = np.float32(np.float32(1.0 / (2.0 * np.pi)) * np.float32(2.0 ** 32))  # (exact product)


def _q(re, im):
    a = np.arctan2(im, re).astype(np.float32)
    r = np.rint((a * K_TURN32).astype(np.float32)).astype(np.int64)  # |r| <= 2^31
    return (r & 0xFFFFFFFF).astype(np.uint32)


def _m(re, im):
    return np.sqrt(((re * re).astype(np.float32) + (im * im).astype(np.float32)).astype(np.float32)).astype(np.float32)


def emulate(X, rate):
    re, im = sanitize(X)
    F = X.shape[-2]
    q, m = _padded(_q(re, im), F), _padded(_m(re, im), F)
    i, al = steps(F, rate)
    al = al[:, None]
    q0, q1 = np.take(q, i, axis=-2), np.take(q, i + 1, axis=-2)
    m0, m1 = np.take(m, i, axis=-2), np.take(m, i + 1, axis=-2)
    inc = (q1 - q0).astype(np.uint32)  # wrapping
    first = np.take(q, [0], axis=-2)
    acc = np.cumsum(np.concatenate([first, np.delete(inc, -1, axis=-2)], axis=-2), axis=-2, dtype=np.uint32)
    mag = ((al * m1).astype(np.float32) + ((np.float32(1.0) - al).astype(np.float32) * m0).astype(np.float32))
    mag = mag.astype(np.float32)
    # phi = 2 pi acc / 2^32 through one float32 rounding of the signed phase
    x = (acc.view(np.int32).astype(np.float32) * np.float32(2.0 ** -31)).astype(np.float32)
    phi = (x.astype(np.float64) * np.pi)
    cs, sn = np.cos(phi).astype(np.float32), np.sin(phi).astype(np.float32)
    out_re = (mag * cs).astype(np.float32)
    out_im = (mag * sn).astype(np.float32)
    bins = X.shape[-1]
    out_im[..., 0] = 0.0
    out_im[..., bins - 1] = 0.0
    return (out_re + 1j * out_im).astype(np.complex64)


def own_scale_error(out, X, rate):
    """Per-element |out - reference| over the element's own scale, and the mask of
    the elements whose two sources are both zero (which must be exactly 0)."""
    ref = reference(X, rate)
    own = own_scale(X, rate)
    dead = own == 0
    err = np.abs(np.asarray(out, np.complex128) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(dead, 0.0, err / np.where(dead, 1.0, own))
    return rel, dead


def spectra(N, F, S=1, seed=5, special=True):
    """Synthetic float32 spectra (S, F, N/2+1): a chirp plus noise, framed at hop
    N/4 under a Hann window, through np.fft.rfft.  special: two silent frames in a
    row (so that some outputs have two zero sources), a bin column scaled by 1e-12
    and a frame scaled by 1e12."""
    rng = np.random.default_rng(seed + 1000 * N + F)
    H = N // 4
    T = (F - 1) * H + N
    n = np.arange(T)
    out = np.empty((S, F, N // 2 + 1), np.complex64)
    w = np.hanning(N)
    idx = np.arange(F)[:, None] * H + np.arange(N)[None, :]
    for s in range(S):
        x = np.sin(2 * np.pi * ((0.01 + 0.003 * s) * n + 2e-6 * n * n * 64.0 / N)) + 0.3 * rng.standard_normal(T)
        out[s] = np.fft.rfft((x[idx] * w).astype(np.float32).astype(np.float64), axis=1).astype(np.complex64)
    if special and F >= 8:
        out[:, F // 2:F // 2 + 2] = 0
        out[:, :, 5] *= np.float32(1e-12)
        out[:, 3] *= np.float32(1e12)
    return out
