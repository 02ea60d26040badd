"""numpy reference of the beamformer (include/crlot_dsp.h, "beamformer"): the contract in
float64 (the model) and restated operation for operation in float32 (what the kernels
compute bit for bit) -- the two spatial covariance matrices per bin, the Cholesky solve for
the weights in both modes, the weighted sum -- plus the test scene (a gated target and a
gated interferer on an array with integer delays), its ideal-ratio mask, the SINR figure
and a float64 STFT.  Vectorised over bins (and any leading axes), scalar loops over the M
microphones.  Imported by the CPU and the GPU tests; needs numpy only."""
import numpy as np

from xspec_reference import factors, hann, length, stft  # noqa: F401  (the same averaging factors and transform)

f32 = np.float32
SOUDEN, STEERED = 0, 1


def _mx(a, b):
    return np.where(a > b, a, b)


def _ct(dt):
    return np.complex64 if dt is f32 else np.complex128


def planes(M):
    return M * M


def re_plane(M, i, j):
    """The plane of Re Phi_ij, i < j (Im is the next one): the M diagonals come first."""
    return M + 2 * (i * M - i * (i + 1) // 2 + (j - i - 1))


def _parts(X, dt):
    return np.asarray(X.real, dt), np.asarray(X.imag, dt)


def _mulc(ar, ai, br, bi):  # a conj(b)
    return (ar * br) + (ai * bi), (ai * br) - (ar * bi)


def _cmul(ar, ai, br, bi):  # conj(a) b
    return (ar * br) + (ai * bi), (ar * bi) - (ai * br)


def _mul(ar, ai, br, bi):  # a b
    return (ar * br) - (ai * bi), (ar * bi) + (ai * br)


def accumulate(X, mask=None, target=0, alpha=0.0, dt=f32, state=None):
    """Steps 1 - 2.  X [..., M, F, bins] complex; mask [..., F, bins] (broadcast over the
    leading axes: a shared mask) or None (1).  state [..., 2, M M, bins] to continue from
    (None: zeros).  Returns the block after the last frame; a matrix the target does not
    update keeps its input (zeros without one)."""
    lam, om = factors(alpha, dt)
    X = np.asarray(X)
    M, F, bins = X.shape[-3:]
    lead = X.shape[:-3]
    if target == 0 and mask is None:
        raise ValueError("target 0 needs a mask")
    S = np.zeros(lead + (2, M * M, bins), dt) if state is None else np.array(state, dt)
    mu = None if mask is None else np.broadcast_to(np.asarray(mask, dt), lead + (F, bins))
    mats = {0: (0, 1), 1: (0,), 2: (1,)}[target]
    with np.errstate(all="ignore"):
        for f in range(F):
            xr, xi = _parts(X[..., f, :], dt)  # [..., M, bins]
            m = np.ones(lead + (bins,), dt) if mu is None else mu[..., f, :]
            for mat in mats:
                wgt = (dt(1) - m) if (target == 0 and mat == 1) else m
                P = S[..., mat, :, :]
                for i in range(M):
                    t = (xr[..., i, :] * xr[..., i, :]) + (xi[..., i, :] * xi[..., i, :])
                    P[..., i, :] = (lam * P[..., i, :]) + (om * (wgt * t))
                    for j in range(i + 1, M):
                        tr, ti = _mulc(xr[..., i, :], xi[..., i, :], xr[..., j, :], xi[..., j, :])
                        k = re_plane(M, i, j)
                        P[..., k, :] = (lam * P[..., k, :]) + (om * (wgt * tr))
                        P[..., k + 1, :] = (lam * P[..., k + 1, :]) + (om * (wgt * ti))
    return S


def _cholesky(Pn, M, loading, dt):
    """The factor of Phi_n + ld I from its planes [..., M M, bins]: d[j], and L[(i, j)] = (re, im), i > j."""
    tiny = dt(1e-30)
    tr = Pn[..., 0, :]
    for i in range(1, M):
        tr = tr + Pn[..., i, :]
    ld = _mx(dt(loading) * (tr / dt(M)), tiny)
    A = [Pn[..., i, :] + ld for i in range(M)]
    d, L = [None] * M, {}
    for j in range(M):
        s = A[j]
        for k in range(j):
            lr, li = L[(j, k)]
            s = s - ((lr * lr) + (li * li))
        d[j] = np.sqrt(_mx(s, tiny))
        for i in range(j + 1, M):
            p = re_plane(M, j, i)
            cr, ci = Pn[..., p, :], -Pn[..., p + 1, :]  # A_ij = conj(A_ji)
            for k in range(j):
                pr, pi = _mulc(*L[(i, k)], *L[(j, k)])
                cr, ci = cr - pr, ci - pi
            L[(i, j)] = (cr / d[j], ci / d[j])
    return d, L


def _chol_solve(d, L, r, M):
    """y = A^-1 r: r a list of M (re, im)."""
    z = [None] * M
    for i in range(M):
        tr, ti = r[i]
        for k in range(i):
            pr, pi = _mul(*L[(i, k)], *z[k])
            tr, ti = tr - pr, ti - pi
        z[i] = (tr / d[i], ti / d[i])
    y = [None] * M
    for i in range(M - 1, -1, -1):
        tr, ti = z[i]
        for k in range(i + 1, M):
            pr, pi = _cmul(*L[(k, i)], *y[k])
            tr, ti = tr - pr, ti - pi
        y[i] = (tr / d[i], ti / d[i])
    return y


def solve(state, M, ref=0, mode=SOUDEN, loading=1e-3, steer=None, dt=f32):
    """Step 3 on a block [..., 2, M M, bins]: the weights [..., M, bins] complex.  loading is
    rounded to dt once (the object's float).  steer [..., M, bins] complex for STEERED."""
    state = np.asarray(state, dt)
    Ps, Pn = state[..., 0, :, :], state[..., 1, :, :]
    tiny = dt(1e-30)
    zero = np.zeros(Ps[..., 0, :].shape, dt)
    with np.errstate(all="ignore"):
        d, L = _cholesky(Pn, M, dt(loading), dt)
        if mode == STEERED:
            sr, si = _parts(np.asarray(steer), dt)
            r = [(np.broadcast_to(sr[..., m, :], zero.shape), np.broadcast_to(si[..., m, :], zero.shape)) for m in range(M)]
            y = _chol_solve(d, L, r, M)
            q = (r[0][0] * y[0][0]) + (r[0][1] * y[0][1])
            for m in range(1, M):
                q = q + ((r[m][0] * y[m][0]) + (r[m][1] * y[m][1]))
            den = _mx(q, tiny)
        else:
            trace, y = None, None
            for c in range(M):
                r = []
                for i in range(M):
                    if i == c:
                        r.append((Ps[..., i, :], zero))
                    elif i < c:
                        p = re_plane(M, i, c)
                        r.append((Ps[..., p, :], Ps[..., p + 1, :]))
                    else:
                        p = re_plane(M, c, i)
                        r.append((Ps[..., p, :], -Ps[..., p + 1, :]))
                yc = _chol_solve(d, L, r, M)
                trace = yc[c][0] if c == 0 else trace + yc[c][0]
                if c == ref:
                    y = yc
            den = _mx(trace, tiny)
        W = np.empty(zero.shape[:-1] + (M, zero.shape[-1]), _ct(dt))
        for m in range(M):
            W[..., m, :].real = y[m][0] / den
            W[..., m, :].imag = y[m][1] / den
    return W


def apply(X, W, dt=f32):
    """Step 4: X [..., M, F, bins], W [..., M, bins] -> Y [..., F, bins]."""
    X = np.asarray(X)
    M = X.shape[-3]
    yr = np.zeros(X.shape[:-3] + X.shape[-2:], dt)
    yi = np.zeros_like(yr)
    with np.errstate(all="ignore"):
        for m in range(M):
            xr, xi = _parts(X[..., m, :, :], dt)
            wr, wi = _parts(np.asarray(W)[..., m, None, :], dt)
            pr, pi = _cmul(wr, wi, xr, xi)
            yr, yi = yr + pr, yi + pi
    Y = np.empty(yr.shape, _ct(dt))
    Y.real, Y.imag = yr, yi
    return Y


def passthrough(M, bins, ref=0, lead=(), dt=f32):
    """The weights after create / reset."""
    W = np.zeros(tuple(lead) + (M, bins), _ct(dt))
    W[..., ref, :] = 1
    return W


def steering_from_delays(delays, nfft):
    """exp(-2 pi i b tau / N) per microphone and bin, float64 rounded once to complex64:
    delays [..., M] in samples against the reference microphone -> [..., M, N/2+1]."""
    tau = np.asarray(delays, np.float64)[..., None]
    b = np.arange(nfft // 2 + 1, dtype=np.float64)
    return np.exp(-2j * np.pi * b * tau / nfft).astype(np.complex64)


def delay_and_sum(delays, nfft):
    """Delay-and-sum weights d / M from delays [..., M]."""
    d = steering_from_delays(delays, nfft).astype(np.complex128)
    return (d / d.shape[-2]).astype(np.complex64)


def matrix(P, M):
    """The Hermitian matrices [..., bins, M, M] complex128 of planes [..., M M, bins] (the condition number's input)."""
    P = np.asarray(P, np.float64)
    A = np.zeros(P.shape[:-2] + (P.shape[-1], M, M), np.complex128)
    for i in range(M):
        A[..., i, i] = P[..., i, :]
        for j in range(i + 1, M):
            k = re_plane(M, i, j)
            A[..., i, j] = P[..., k, :] + 1j * P[..., k + 1, :]
            A[..., j, i] = P[..., k, :] - 1j * P[..., k + 1, :]
    return A


# ----------------------------------------------------------------- the scene
def target_delays(M):
    return np.array([(3 * m) % 7 for m in range(M)])


def interferer_delays(M):
    return np.array([(5 * m + 2) % 11 for m in range(M)])


def scene(M, N, H, F=60, seed=5, noise=0.05):
    """A white target and a white interferer, each gated on and off per hop at random, on M
    microphones with integer delays (3m) mod 7 and (5m + 2) mod 11, sensor noise at `noise`.
    Returns (x, s, v): the microphone signals [M, T] and their target and interferer-plus-
    noise parts, x = s + v, float32 values in float64 arrays."""
    rng = np.random.default_rng(seed)
    T = length(N, H, F)
    hops = T // H + 2
    pad = 16

    def gated():
        g = rng.standard_normal(T + pad)
        on = np.repeat(rng.integers(0, 2, hops).astype(np.float64), H)[:T + pad]
        return g * on

    src, itf = gated(), gated()
    s = np.stack([src[pad - d:pad - d + T] for d in target_delays(M)])
    v = np.stack([itf[pad - d:pad - d + T] for d in interferer_delays(M)]) + noise * rng.standard_normal((M, T))
    s = s.astype(f32).astype(np.float64)
    v = v.astype(f32).astype(np.float64)
    return (s + v).astype(f32).astype(np.float64), s, v


def ideal_ratio_mask(S, V):
    """|S0|^2 / (|S0|^2 + |V0|^2) at microphone 0 from spectra [M, F, bins] (0 where both vanish)."""
    ps, pv = np.abs(S[0]) ** 2, np.abs(V[0]) ** 2
    return np.where(ps + pv > 0, ps / np.maximum(ps + pv, 1e-300), 0.0)


def sinr_db(Ys, Yv):
    """10 log10 of the power ratio of two spectra sets."""
    return 10.0 * np.log10((np.abs(Ys) ** 2).sum() / (np.abs(Yv) ** 2).sum())


def sinr_gain_db(S, V, W):
    """The SINR after the weights W [M, bins] minus microphone 0's, in dB, float64."""
    W = np.asarray(W, np.complex128)
    out = sinr_db(apply(S, W, np.float64), apply(V, W, np.float64))
    return out - sinr_db(S[0], V[0])
