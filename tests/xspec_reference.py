"""numpy reference of the cross-spectral estimator (include/crlot_dsp.h, "cross-spectral
estimation"): the contract in float64 (the model) and restated operation for operation in
float32 (what the kernels compute bit for bit) -- the four averaged planes, the derived
rows, the peak search -- plus the test signals (a delayed pair, a short FIR system) and a
float64 STFT.  Imported by the CPU and the GPU tests; needs numpy only."""
import numpy as np

f32 = np.float32
PLANES = ("Saa", "Sbb", "Sr", "Si")
NONE, PHAT = 0, 1


def factors(alpha, dt=f32):
    """(lambda, omega) as the kernels read them: (1, 1) for Welch sums (alpha 0), else
    dt(alpha) and dt(1 - alpha) formed in double."""
    a = float(alpha)
    return (dt(1), dt(1)) if a == 0.0 else (dt(a), dt(1.0 - a))


def _mx(a, b):
    return np.where(a > b, a, b)


def terms(A, B, dt=f32):
    """Step 1 on complex rows: Taa, Tbb, Tr, Ti, every operation rounded in dt (conj(A) B)."""
    ar, ai = np.asarray(A.real, dt), np.asarray(A.imag, dt)
    br, bi = np.asarray(B.real, dt), np.asarray(B.imag, dt)
    return ((ar * ar) + (ai * ai), (br * br) + (bi * bi), (ar * br) + (ai * bi), (ar * bi) - (ai * br))


def accumulate(A, B, alpha=0.0, dt=f32, state=None):
    """Steps 1 - 2 over A, B [..., F, bins] complex (frames along axis -2; A may lack the
    leading axes: a shared reference).  state: the four planes [..., 4, bins] to continue
    from (None: zeros).  Returns the planes after the last frame, [..., 4, bins] in dt."""
    lam, om = factors(alpha, dt)
    B = np.asarray(B)
    A = np.broadcast_to(np.asarray(A), B.shape)
    F = B.shape[-2]
    shape = B.shape[:-2] + (B.shape[-1],)
    S = [np.zeros(shape, dt) for _ in range(4)] if state is None else [np.array(state[..., j, :], dt) for j in range(4)]
    with np.errstate(all="ignore"):
        for f in range(F):
            T = terms(A[..., f, :], B[..., f, :], dt)
            S = [(lam * s) + (om * t) for s, t in zip(S, T)]
    return np.stack(S, axis=-2)


def derive(state, weighting=NONE, dt=f32):
    """Step 3 on a state block [..., 4, bins]: (C, H1, W), H1 and W complex."""
    Saa, Sbb, Sr, Si = (np.asarray(state[..., j, :], dt) for j in range(4))
    tiny = dt(1e-30)
    ct = np.complex64 if dt is f32 else np.complex128
    with np.errstate(all="ignore"):
        m2 = (Sr * Sr) + (Si * Si)
        C = m2 / _mx(Saa * Sbb, tiny)
        d = _mx(Saa, tiny)
        H1 = np.empty(Sr.shape, ct)
        H1.real, H1.imag = Sr / d, Si / d
        W = np.empty(Sr.shape, ct)
        if weighting == PHAT:
            e = _mx(np.sqrt(m2), tiny)
            W.real, W.imag = Sr / e, Si / e
        else:
            W.real, W.imag = Sr, Si
    return C, H1, W


def peak_row(cc, max_lag, dt=f32):
    """Step 4 on one row cc[N]: the serial scan and the parabolic refinement, {l, frac, y1} in dt."""
    cc = np.asarray(cc, dt)
    n = len(cc)
    assert 1 <= max_lag <= n // 2 - 1
    best, bv = 0, cc[(-max_lag) % n]
    for j in range(1, 2 * max_lag + 1):
        v = cc[(j - max_lag) % n]
        if v > bv:
            best, bv = j, v
    l = best - max_lag
    y0, y1, y2 = cc[(l - 1) % n], cc[l % n], cc[(l + 1) % n]
    with np.errstate(all="ignore"):
        den = (y0 - (dt(2) * y1)) + y2
        frac = dt(0) if den == 0 else (dt(0.5) * (y0 - y2)) / den
    return np.array([dt(l), frac, y1], dt)


def peak(cc, max_lag, dt=f32):
    """peak_row over the rows of cc [P, N]."""
    return np.stack([peak_row(r, max_lag, dt) for r in np.asarray(cc)])


def runner_up(cc, max_lag, lag):
    """The largest value of a row within the search at any lag but `lag`."""
    n = len(cc)
    return max(float(cc[l % n]) for l in range(-max_lag, max_lag + 1) if l != lag)


def delay(state, n, weighting=PHAT, max_lag=None, dt=f32):
    """derive(W) -> irfft -> peak in numpy (the inverse transform is numpy's, in float64,
    rounded to dt: the model of crlot_xspec_delay, not its bits).  Returns (rows, cc)."""
    W = derive(state, weighting, dt)[2]
    cc = np.fft.irfft(W.astype(np.complex128), n, axis=-1).astype(dt)
    m = n // 2 - 1 if max_lag is None else max_lag
    return peak(cc.reshape(-1, n), m, dt).reshape(cc.shape[:-1] + (3,)), cc


# ----------------------------------------------------------------- signals and transforms
def hann(n):
    """The periodic Hann window."""
    return np.hanning(n + 1)[:n]


def stft(x, N, H, w):
    """Frames k H .. k H + N of x [..., T] under w, float64 rfft: [..., F, N/2+1]."""
    x = np.asarray(x, np.float64)
    F = (x.shape[-1] - N) // H + 1
    return np.stack([np.fft.rfft(x[..., k * H:k * H + N] * w) for k in range(F)], axis=-2)


def length(N, H, F):
    return N + (F - 1) * H


def delayed_pair(T, D, seed=11, noise=0.1):
    """a white noise, b[n] = a[n - D] + noise * white (D may be negative: b leads).  float32
    values in float64 arrays, so every consumer transforms the same samples."""
    rng = np.random.default_rng(seed)
    pad = abs(D) + 1
    g = rng.standard_normal(T + 2 * pad)
    a = g[pad:pad + T]
    b = g[pad - D:pad - D + T] + noise * rng.standard_normal(T)
    return a.astype(f32).astype(np.float64), b.astype(f32).astype(np.float64)


FIR = np.array([1.0, 0.0, 0.0, 0.3, 0.0, -0.2, 0.0, 0.1])


def fir_pair(T, seed=13, noise=0.01, h=FIR):
    """a white noise, b = a (*) h + noise * white, the filter run in from before the first sample."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(T + len(h) - 1)
    b = np.convolve(g, h)[len(h) - 1:len(h) - 1 + T] + noise * rng.standard_normal(T)
    return g[len(h) - 1:].astype(f32).astype(np.float64), b.astype(f32).astype(np.float64)
