"""References for HPSS (include/crlot_dsp.h, "HPSS").

Test helper (a plain module, no fixtures).

`masks32` restates the contract with numpy float32 operations only: every step
is one correctly rounded float32 operation (numpy evaluates one ufunc at a time,
so there is no FMA), and a median is np.sort(window)[..., r], a selection, so the
device kernels equal it bit for bit however they find the median.

`softmask64` is librosa.util.softmask in float64 (with librosa's split_zeros rule)
for cross-checking the float32 mask formula on the same float32 medians.
"""
import numpy as np

HARD = -1                     # crlot_hpss_desc.power: CRLOT_HPSS_HARD
FLT_MIN = np.float32(1.17549435e-38)
U32 = 2.0 ** -24              # float32 unit roundoff


def sanit32(v):
    """IFftPlan's sanitize: NaN / Inf -> 0, |v| < 1e-30 -> 0 (float32)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(v)
        keep = (a >= np.float32(1e-30)) & (a <= np.float32(3.402823466e+38))
    return np.where(keep, v, np.float32(0.0)).astype(np.float32)


def magnitude32(Z):
    """m = sqrt(fl(fl(re re) + fl(im im))) of sanitized spectra (..., bins) complex64;
    bins 0 and N/2 take im as 0."""
    Z = np.asarray(Z, np.complex64)
    re = sanit32(Z.real)
    im = sanit32(Z.imag)
    im[..., 0] = 0
    im[..., -1] = 0
    with np.errstate(over="ignore", under="ignore"):
        a = re * re
        b = im * im
        return np.sqrt(a + b).astype(np.float32)


def ext(i, n):
    """The reflect extension (d c b a | a b c d | d c b a) of index array i into [0, n)."""
    j = np.mod(np.asarray(i, np.int64), 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def median_along(m, w, axis):
    """The running median of width w (odd) along `axis` with the reflect extension:
    np.sort of the gathered window, element r."""
    m = np.asarray(m)
    r = (w - 1) // 2
    n = m.shape[axis]
    idx = ext(np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :], n)   # (n, w)
    g = np.take(np.moveaxis(m, axis, -1), idx, axis=-1)                   # (..., n, w)
    med = np.sort(g, axis=-1)[..., r]
    return np.moveaxis(med, -1, axis)


def medians32(m, win_harm, win_perc):
    """(h, p): medians of m (..., F, bins) along time (axis -2) and frequency (axis -1)."""
    return median_along(m, win_harm, -2), median_along(m, win_perc, -1)


def softmask32(X, R, power, split):
    """The mask of X against R (R already multiplied by its margin), float32."""
    X = np.asarray(X, np.float32)
    R = np.asarray(R, np.float32)
    if power == HARD:
        return (X > R).astype(np.float32)
    Z = np.maximum(X, R)
    bad = Z < FLT_MIN
    Zs = np.where(bad, np.float32(1), Z)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        a = X / Zs
        b = R / Zs
        if power == 2:
            a = a * a
            b = b * b
        mask = a / (a + b)
    return np.where(bad, np.float32(0.5 if split else 0.0), mask).astype(np.float32)


def masks32(Z, win_harm=31, win_perc=31, power=2, margin_harm=1.0, margin_perc=1.0):
    """The contract: spectra (..., F, bins) complex64 -> (mask_h, mask_p) float32."""
    m = magnitude32(Z)
    h, p = medians32(m, win_harm, win_perc)
    mh, mp = np.float32(margin_harm), np.float32(margin_perc)
    split = bool(mh == 1 and mp == 1)
    with np.errstate(over="ignore", under="ignore"):
        return softmask32(h, p * mh, power, split), softmask32(p, h * mp, power, split)


def softmask64(X, X_ref, power, split_zeros):
    """librosa.util.softmask in float64 (power finite), librosa's code restated:
    Z = max(X, X_ref); mask = (X/Z)^p / ((X/Z)^p + (X_ref/Z)^p); where Z is below
    the smallest normal float32, 0.5 with split_zeros and else 0."""
    X = np.asarray(X, np.float64)
    R = np.asarray(X_ref, np.float64)
    Z = np.maximum(X, R)
    bad = Z < np.finfo(np.float32).tiny
    Zs = np.where(bad, 1.0, Z)
    a = (X / Zs) ** power
    b = (R / Zs) ** power
    with np.errstate(invalid="ignore"):
        mask = a / (a + b)
    return np.where(bad, 0.5 if split_zeros else 0.0, mask)


def make_spectrum(N, S, F, seed=0, nasty=False):
    """(S, F, bins) complex64: noise with a few sustained tones and clicks, so both
    medians and both masks take values across [0, 1]; nasty: zero rows and columns,
    NaN / Inf / tiny components and exact ties."""
    bins = N // 2 + 1
    rng = np.random.default_rng(1000 * N + 10 * F + S + seed)
    Z = (rng.standard_normal((S, F, bins)) + 1j * rng.standard_normal((S, F, bins))).astype(np.complex64)
    Z[:, :, 5::17] *= np.float32(8.0)          # tones: loud columns
    Z[:, 2::9, :] *= np.float32(6.0)           # clicks: loud rows
    Z *= rng.uniform(0.1, 10.0, (S, 1, 1)).astype(np.float32)
    if nasty:
        Z[0, F // 2, :] = 0                    # a zero row
        Z[0, :, 7] = 0                         # a zero column
        Z[0, :, 20:60] = 0                     # a zero band: h = p = 0 inside it
        Z[-1, 0, 3] = complex(np.nan, 1)
        Z[-1, 0, 4] = complex(1, np.inf)
        Z[-1, min(1, F - 1), 5] = complex(-np.inf, 2)
        Z[-1, min(1, F - 1), 6] = complex(1e-35, 1e-35)  # below the sanitize threshold
        Z[-1, :, 64:96] = np.complex64(3 + 4j)  # ties: a constant block, |z| = 5 exactly
        Z.imag[:, :, 0] = 0.5                  # bins 0 and N/2: imaginary parts are ignored
        Z.imag[:, :, -1] = -0.5
    return Z
