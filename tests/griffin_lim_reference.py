"""References for Griffin-Lim (include/crlot_dsp.h, "Griffin-Lim").

Test helper (a plain module, no fixtures).

`project32` restates the projection's contract with numpy float32 operations
only: every step is one correctly rounded float32 operation (numpy evaluates one
ufunc at a time, so there is no FMA), which is what both device kernels compute,
bit for bit.  `project64` is the same formula in float64.

`griffin_lim_f64` runs the recurrence in float64 on tests/f64_reference.py's
`stft_f64` / `istft_ola_f64`:

    y_0     = istft_ola(S_0)
    y_{i+1} = istft_ola(project(stft(y_i), tprev_i, mag)),   tprev_{i+1} = stft(y_i)

The norm table.  `istft_ola_f64` divides by the plan's default table, the
reference's sum of the *window* (f64_reference's docstring), so with an analysis
window istft_ola(stft(x)) = x sum(w^2) / sum(w), not x.  Griffin and Lim's theorem
(the spectral convergence never increases) is about the least-squares inverse,
which divides by sum(w^2).  `ls_norm32` is that table, periodic in the hop, in
float32 as a plan takes it (Plan.upload_tables(norm=...)); with `ls=True` the
functions here rescale every istft_ola_f64 output sample by
max(norm_w, eps) / max(norm_w2, eps), i.e. divide the same overlap-add sums by
the least-squares table instead.  The convergence tests, on the CPU and on the
device, run with that table; the default table's figures are printed beside them.
"""
import numpy as np

import f64_reference as R

U32 = 2.0 ** -24  # float32 unit roundoff
F_SIGNAL = 24     # frames of the test signal
SHAPES = [(256, 128), (512, 128), (1024, 256)]


# ------------------------------------------------------------------ the projection
def sanit32(v):
    """IFftPlan's sanitize: NaN / Inf -> 0, |v| < 1e-30 -> 0 (float32)."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(v)
        keep = (a >= np.float32(1e-30)) & (a <= np.float32(3.402823466e+38))
    return np.where(keep, v, np.float32(0.0)).astype(np.float32)


def alpha32(momentum):
    return np.float32(np.float64(momentum) / (1.0 + np.float64(momentum)))


def _parts(Z, dtype):
    """Sanitized (re, im) of spectra (..., bins); bins 0 and N/2 take im as 0."""
    Z = np.asarray(Z, np.complex64)
    re = sanit32(Z.real).astype(dtype)
    im = sanit32(Z.imag).astype(dtype)
    im[..., 0] = 0
    im[..., -1] = 0
    return re, im


def project32(X, mag, T=None, momentum=0.0):
    """The contract in float32: X, T (optional) complex64 (..., bins), mag float32
    (..., bins) -> complex64.  numpy float32 operations only."""
    f = np.float32
    xr, xi = _parts(X, f)
    m = sanit32(mag)
    if T is None:
        cr, ci = xr, xi
    else:
        a = alpha32(momentum)
        tr, ti = _parts(T, f)
        cr = xr - a * tr
        ci = xi - a * ti
    with np.errstate(all="ignore"):
        p = cr * cr + ci * ci
        d = np.sqrt(p) + f(1e-16)
        s = m / d
        out_r = cr * s
        out_i = ci * s
    assert out_r.dtype == f and out_i.dtype == f and s.dtype == f
    out_i[..., 0] = 0.0
    out_i[..., -1] = 0.0
    out = np.empty(out_r.shape, np.complex64)
    out.real = out_r
    out.imag = out_i
    return out


def project64(X, mag, T=None, momentum=0.0, sanitize=True):
    """The same formula in float64 (alpha in double).  sanitize=False: X, T and
    mag are used as they are (the float64 recurrence below)."""
    if sanitize:
        xr, xi = _parts(X, np.float64)
        m = sanit32(mag).astype(np.float64)
    else:
        X = np.asarray(X, np.complex128)
        xr, xi = X.real.copy(), X.imag.copy()
        xi[..., 0] = 0
        xi[..., -1] = 0
        m = np.asarray(mag, np.float64)
    cr, ci = xr, xi
    if T is not None:
        a = float(momentum) / (1.0 + float(momentum))
        if sanitize:
            tr, ti = _parts(T, np.float64)
        else:
            T = np.asarray(T, np.complex128)
            tr, ti = T.real.copy(), T.imag.copy()
            ti[..., 0] = 0
            ti[..., -1] = 0
        cr = xr - a * tr
        ci = xi - a * ti
    s = m / (np.sqrt(cr * cr + ci * ci) + 1e-16)
    out = (cr * s) + 1j * (ci * s)
    out.imag[..., 0] = 0
    out.imag[..., -1] = 0
    return out


def conditioning(X, T, momentum):
    """(|X| + alpha |T|) / |c|, the factor by which the subtraction c = X - alpha T
    amplifies the relative rounding errors of its operands (inf where c == 0)."""
    xr, xi = _parts(X, np.float64)
    if T is None:
        return np.ones(xr.shape)
    a = float(momentum) / (1.0 + float(momentum))
    tr, ti = _parts(T, np.float64)
    c = np.hypot(xr - a * tr, xi - a * ti)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.hypot(xr, xi) + a * np.hypot(tr, ti)) / c


# ------------------------------------------------------------------ the recurrence in float64
def ls_norm32(n, h):
    """The least-squares norm table of a plan: sum over the frames covering a
    sample of w^2, periodic in the hop, [ring_len] float32."""
    w = R.window32(n).astype(np.float64)
    ring = R.O.ring_len(n, h)
    i = np.arange(ring) % h
    tbl = np.zeros(ring)
    for j in range(0, n, h):
        ok = i + j < n
        tbl[ok] += w[(i + j)[ok]] ** 2
    return tbl.astype(np.float32)


def _rescale(n, h, L):
    """Per output sample max(norm_w, eps) / max(norm_w2, eps): turns istft_ola_f64's
    division by the default table into the division by ls_norm32."""
    w32 = R.window32(n)
    dw = np.maximum(R.O.norm_table(w32, n, h).astype(np.float64), R.EPS)
    d2 = np.maximum(ls_norm32(n, h).astype(np.float64), R.EPS)
    i = np.arange(L)
    return dw[i % dw.size] / d2[i % d2.size]


def istft_f64(spec, n, h, ls=False):
    y, _ = R.istft_ola_f64(spec, n, h)
    return y * _rescale(n, h, y.size) if ls else y


def griffin_lim_f64(mag, n, h, n_iter, momentum, init=None, ls=False, trace=False):
    """One stream: mag (F, bins) -> y_{n_iter} (F h,) in float64; trace=True: the
    list [y_0, ..., y_{n_iter}]."""
    mag = np.asarray(mag, np.float64)
    S0 = mag.astype(np.complex128) if init is None else project64(init, mag, sanitize=False)
    y = istft_f64(S0, n, h, ls)
    ys = [y]
    tprev = None
    for _ in range(n_iter):
        X = R.stft_f64(y, n, h)
        y = istft_f64(project64(X, mag, tprev if momentum > 0 else None, momentum, sanitize=False), n, h, ls)
        tprev = X
        ys.append(y)
    return ys if trace else y


def spectral_convergence(y, mag, n, h):
    """|| |stft_f64(y)| - mag ||_F / || mag ||_F"""
    mag = np.asarray(mag, np.float64)
    return float(np.linalg.norm(np.abs(R.stft_f64(np.asarray(y, np.float64), n, h)) - mag) / np.linalg.norm(mag))


# ------------------------------------------------------------------ shared inputs
def make_signal(n, h, seed=0, F=F_SIGNAL):
    """F h samples: a steady sine, a swept sine and 5 % noise (float32)."""
    T = F * h
    t = np.arange(T, dtype=np.float64)
    rng = np.random.default_rng(1000 + seed)
    f0 = 0.031 + 0.004 * seed
    sweep = 0.06 + (0.11 * t / T)
    x = 0.5 * np.sin(2 * np.pi * f0 * t) + 0.4 * np.sin(2 * np.pi * np.cumsum(sweep)) + \
        0.05 * rng.standard_normal(T)
    return x.astype(np.float32)


def target_mag(x, n, h):
    """|stft_f64(x)| rounded to float32: the magnitudes Griffin-Lim starts from."""
    return np.abs(R.stft_f64(x, n, h)).astype(np.float32)


def random_phase_init(shape, seed=0):
    """Unit-magnitude spectra with seeded uniform phases (complex64)."""
    ph = np.random.default_rng(2000 + seed).uniform(0.0, 2.0 * np.pi, shape)
    return np.exp(1j * ph).astype(np.complex64)
