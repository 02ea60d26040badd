"""Float64 reference of the resampler (include/crlot_dsp.h, "resample / pitch shift").

geometry(up, down, zeros, rolloff)        (U, D, W, K, base)
table(U, D, zeros, rolloff, window, beta) the (U, K) filter table in float64
output_length(T, U, D)                    ceil(T U / D)
sanitize(x)                               NaN / Inf -> 0, |v| < 1e-30 -> 0
resample(x, U, D, W, table)               y[m] = sum_i table[r][i] xs[c - W + 1 + i], the plain dot
                                          product over the K taps with zero padding, and
                                          sum_i |table[r][i] xs[.]| beside it (the error bound's scale)
fma_bound(K)                              gamma_K = K 2^-24 / (1 - K 2^-24)
"""
import math

import numpy as np


def geometry(up, down, zeros=16, rolloff=0.95):
    g = math.gcd(int(up), int(down))
    U, D = int(up) // g, int(down) // g
    base = min(U, D) * float(rolloff)
    W = int(math.ceil(zeros * D / base))
    return U, D, W, 2 * W, base


def table(up, down, zeros=16, rolloff=0.95, window="hann", beta=8.6):
    U, D, W, K, base = geometry(up, down, zeros, rolloff)
    j = np.arange(K, dtype=np.float64)[None, :] - W + 1
    r = np.arange(U, dtype=np.float64)[:, None]
    tau = (j - r / U) * base / D
    inside = np.abs(tau) < zeros
    t = np.where(inside, tau, 0.0)
    sinc = np.sinc(t)  # sin(pi t) / (pi t), 1 at 0
    if window == "hann":
        win = np.cos(np.pi * t / (2.0 * zeros)) ** 2
    elif window == "kaiser":
        win = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (t / zeros) ** 2))) / np.i0(beta)
    else:
        raise ValueError(window)
    return np.where(inside, (base / D) * sinc * win, 0.0), tau


def output_length(T, U, D):
    return (int(T) * U + D - 1) // D


def sanitize(x):
    x = np.asarray(x)
    a = np.abs(x)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(x) & (a >= np.float32(1e-30))
    return np.where(keep, x, 0).astype(x.dtype)


def resample(x, U, D, W, tab):
    """x: (..., T) -> (y, scale), both (..., L) float64; tab: (U, 2 W), any float dtype."""
    x = np.asarray(x)
    T = x.shape[-1]
    K = 2 * W
    L = output_length(T, U, D)
    xs = sanitize(x).astype(np.float64)
    pad = np.zeros(x.shape[:-1] + (W,), np.float64)
    xp = np.concatenate([pad, xs, pad, pad[..., :1]], axis=-1)  # xp[k + W] = xs[k]
    m = np.arange(L, dtype=np.int64)
    c, r = (m * D) // U, (m * D) % U
    idx = (c + 1)[:, None] + np.arange(K)[None, :]  # (c - W + 1 + i) + W
    h = np.asarray(tab, np.float64)[r]             # (L, K)
    terms = h * xp[..., idx]                         # (..., L, K)
    return terms.sum(-1), np.abs(terms).sum(-1)


def fma_bound(K):
    u = K * 2.0 ** -24
    return u / (1.0 - u)
