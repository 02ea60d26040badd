"""numpy reference of the WPE dereverberator (include/crlot_dsp.h, "dereverberation"): the
contract restated operation for operation in float32 (what the kernels compute bit for
bit; dt=np.float64 runs the same statements in double) and a float64 model in the textbook
form (einsum, linalg.solve), plus the test scene (a gated white source under exponentially
decaying white impulse responses), the early-signal error figure and a float64 STFT.
The restatement is vectorised over bins, leading axes and -- where the contract fixes no
order between them -- matrix entries; every order the contract does fix (the frames, the
microphones of the power, the Cholesky and the substitutions, the filter's l, the RLS
step's j and i) is an explicit loop.  Imported by the CPU and the GPU tests; needs numpy
only."""
import numpy as np

from beamform_reference import _chol_solve, _cholesky, _cmul, _mul, _mulc, _mx, _parts, re_plane
from xspec_reference import hann, length, stft  # noqa: F401  (the same transform)

f32 = np.float32
TINY = 1e-30

# what the float32 restatement shows against the float64 model on the scene, relative to the
# largest magnitude (measured: state 4.97e-07, output 5.70e-04, RLS output 5.36e-06, Q 1.37e-05;
# DESIGN 3s tables them).  tests/test_wpe_reference.py measures them again and holds them with a
# half again for another BLAS or numpy; the GPU tests hold the device to 4 x these.
MEASURED = dict(offline_state=5.0e-7, offline_out=5.7e-4, rls_out=5.4e-6, rls_cov=1.4e-5)


def _ct(dt):
    return np.complex64 if dt is f32 else np.complex128


def state_planes(M, K):
    L = M * K
    return L * L + 2 * L * M


def p_plane(L, M, l, m):
    return L * L + 2 * (l * M + m)


def stacked(Y, K, D):
    """Y [..., M, F, bins] -> [..., L, F, bins]: entry l = tau M + m of frame t is Y_m(t - D -
    tau), zeros before the start."""
    Y = np.asarray(Y)
    M, F, bins = Y.shape[-3:]
    out = np.zeros(Y.shape[:-3] + (M * K, F, bins), Y.dtype)
    for tau in range(K):
        sh = D + tau
        if sh < F:
            out[..., tau * M:(tau + 1) * M, sh:, :] = Y[..., :, :F - sh, :]
    return out


def power(Z, floor=1e-10, dt=f32):
    """Step 1: iota [..., F, bins] of Z [..., M, F, bins]."""
    with np.errstate(all="ignore"):
        return (dt(1) / _lam(Z, floor, dt)).astype(dt)


def _lam(Z, floor, dt):
    """lambda [..., F, bins]: the mean power over the microphones, summed in m order, floored."""
    zr, zi = _parts(np.asarray(Z), dt)
    M = zr.shape[-3]
    with np.errstate(all="ignore"):
        p = (zr[..., 0, :, :] * zr[..., 0, :, :]) + (zi[..., 0, :, :] * zi[..., 0, :, :])
        for m in range(1, M):
            p = p + ((zr[..., m, :, :] * zr[..., m, :, :]) + (zi[..., m, :, :] * zi[..., m, :, :]))
        return _mx(p / dt(M), dt(floor)).astype(dt)


def _unpack(S, M, K, dt):
    """State planes [..., L L + 2 L M, bins] -> (Rr, Ri [..., L, L, bins] upper part, Pr, Pi [..., L, M, bins])."""
    L = M * K
    lead, bins = S.shape[:-2], S.shape[-1]
    Rr, Ri = np.zeros(lead + (L, L, bins), dt), np.zeros(lead + (L, L, bins), dt)
    for i in range(L):
        Rr[..., i, i, :] = S[..., i, :]
        for j in range(i + 1, L):
            Rr[..., i, j, :] = S[..., re_plane(L, i, j), :]
            Ri[..., i, j, :] = S[..., re_plane(L, i, j) + 1, :]
    P = S[..., L * L:, :].reshape(lead + (L, M, 2, bins))
    return Rr, Ri, np.array(P[..., 0, :]), np.array(P[..., 1, :])


def _pack(Rr, Ri, Pr, Pi, M, K, dt):
    L = M * K
    lead, bins = Rr.shape[:-3], Rr.shape[-1]
    S = np.zeros(lead + (state_planes(M, K), bins), dt)
    for i in range(L):
        S[..., i, :] = Rr[..., i, i, :]
        for j in range(i + 1, L):
            S[..., re_plane(L, i, j), :] = Rr[..., i, j, :]
            S[..., re_plane(L, i, j) + 1, :] = Ri[..., i, j, :]
    S[..., L * L:, :] = np.stack([Pr, Pi], axis=-2).reshape(lead + (2 * L * M, bins))
    return S


def accumulate(Y, iota, K, D, f0=0, f1=None, state=None, dt=f32):
    """Step 2 over the frames [f0, f1) of Y [..., M, F, bins] with iota [..., F, bins]; state
    [..., L L + 2 L M, bins] to continue from (None: zeros).  The entries are independent, so
    they are formed together; the frames are walked in order."""
    Y = np.asarray(Y)
    M, F, bins = Y.shape[-3:]
    f1 = F if f1 is None else f1
    L = M * K
    lead = Y.shape[:-3]
    S = np.zeros(lead + (state_planes(M, K), bins), dt) if state is None else np.asarray(state, dt)
    Rr, Ri, Pr, Pi = _unpack(S, M, K, dt)
    yr, yi = _parts(Y, dt)
    sr, si = _parts(stacked(Y, K, D), dt)
    io = np.asarray(iota, dt)
    with np.errstate(all="ignore"):
        for t in range(f0, f1):
            ar, ai = sr[..., :, None, t, :], si[..., :, None, t, :]
            w = io[..., None, None, t, :]
            tr, ti = _mulc(ar, ai, sr[..., None, :, t, :], si[..., None, :, t, :])
            Rr, Ri = Rr + (w * tr), Ri + (w * ti)
            tr, ti = _mulc(ar, ai, yr[..., None, :, t, :], yi[..., None, :, t, :])
            Pr, Pi = Pr + (w * tr), Pi + (w * ti)
    return _pack(Rr.astype(dt), Ri.astype(dt), Pr.astype(dt), Pi.astype(dt), M, K, dt)


def solve(S, M, K, loading=1e-3, dt=f32):
    """Step 3: the taps [..., L, M, bins] complex of a state block."""
    S = np.asarray(S, dt)
    L = M * K
    with np.errstate(all="ignore"):
        d, Lf = _cholesky(S[..., :L * L, :], L, loading, dt)
        G = np.zeros(S.shape[:-2] + (L, M, S.shape[-1]), _ct(dt))
        for m in range(M):
            r = [(S[..., p_plane(L, M, l, m), :], S[..., p_plane(L, M, l, m) + 1, :]) for l in range(L)]
            y = _chol_solve(d, Lf, r, L)
            for l in range(L):
                G[..., l, m, :] = y[l][0] + 1j * y[l][1].astype(_ct(dt))
    return G


def _join(re, im, dt):
    out = np.empty(re.shape, _ct(dt))
    out.real, out.imag = re, im
    return out


def filt(Y, G, K, D, dt=f32):
    """Step 4: X [..., M, F, bins] from Y and the taps G [..., L, M, bins]."""
    Y = np.asarray(Y)
    M = Y.shape[-3]
    yr, yi = _parts(Y, dt)
    sr, si = _parts(stacked(Y, K, D), dt)
    gr, gi = _parts(np.asarray(G), dt)
    ar, ai = np.zeros(yr.shape, dt), np.zeros(yr.shape, dt)
    with np.errstate(all="ignore"):
        for l in range(M * K):
            pr, pi = _cmul(gr[..., l, :, None, :], gi[..., l, :, None, :], sr[..., l, None, :, :], si[..., l, None, :, :])
            ar, ai = ar + pr, ai + pi
        return _join(yr - ar, yi - ai, dt)


def eye_cov(lead, M, K, bins, dt=f32):
    L = M * K
    Q = np.zeros(tuple(lead) + (L * L, bins), dt)
    Q[..., :L, :] = 1
    return Q


def rls(Y, Q, G, K, D, alpha=0.9999, floor=1e-10, f0=0, f1=None, dt=f32):
    """Step 5 over the frames [f0, f1): Y [..., M, F, bins], Q [..., L L, bins] planes, G [...,
    L, M, bins] complex.  Returns (out [..., M, f1 - f0, bins], Q, G)."""
    Y = np.asarray(Y)
    M, F, bins = Y.shape[-3:]
    f1 = F if f1 is None else f1
    L = M * K
    lead = Y.shape[:-3]
    S = np.zeros(lead + (state_planes(M, K), bins), dt)
    S[..., :L * L, :] = np.asarray(Q, dt)
    Ur, Ui, _, _ = _unpack(S, M, K, dt)  # the diagonal in Ur[i, i], the upper part in (Ur, Ui)[i, j], i < j
    gr, gi = (np.array(a) for a in _parts(np.asarray(G), dt))
    yr, yi = _parts(Y, dt)
    sr, si = _parts(stacked(Y, K, D), dt)
    lam = _lam(Y, floor, dt)
    a = dt(alpha)
    idx = np.arange(L)
    shape1 = (L,) + (1,)
    out = np.zeros(lead + (M, f1 - f0, bins), _ct(dt))
    with np.errstate(all="ignore"):
        for t in range(f0, f1):
            cr, ci = sr[..., t, :], si[..., t, :]  # [..., L, bins]
            # pred with the old taps
            ar, ai = np.zeros(lead + (M, bins), dt), np.zeros(lead + (M, bins), dt)
            for l in range(L):
                pr, pi = _cmul(gr[..., l, :, :], gi[..., l, :, :], cr[..., l, None, :], ci[..., l, None, :])
                ar, ai = ar + pr, ai + pi
            er, ei = yr[..., t, :] - ar, yi[..., t, :] - ai  # [..., M, bins]
            out[..., t - f0, :] = _join(er, ei, dt)
            # v_i, j ascending from j = 0's term
            vr = vi = None
            for j in range(L):
                up = (idx < j).reshape(shape1)
                dg = (idx == j).reshape(shape1)
                qr = np.where(up, Ur[..., :, j, :], Ur[..., j, :, :])
                qi = np.where(up, Ui[..., :, j, :], Ui[..., j, :, :])
                bjr, bji = cr[..., j, None, :], ci[..., j, None, :]
                m_r, m_i = _mul(qr, qi, bjr, bji)
                c_r, c_i = _cmul(qr, qi, bjr, bji)
                d_r, d_i = qr * bjr, qr * bji
                tr = np.where(dg, d_r, np.where(up, m_r, c_r))
                ti = np.where(dg, d_i, np.where(up, m_i, c_i))
                vr, vi = (tr, ti) if j == 0 else (vr + tr, vi + ti)
            s = None
            for i in range(L):
                term = (cr[..., i, :] * vr[..., i, :]) + (ci[..., i, :] * vi[..., i, :])
                s = term if i == 0 else s + term
            den = _mx((a * lam[..., t, :]) + s, dt(TINY))[..., None, :]
            kr, ki = vr / den, vi / den
            # Q: the upper part and the diagonal
            pr, pi = _mulc(kr[..., :, None, :], ki[..., :, None, :], vr[..., None, :, :], vi[..., None, :, :])
            nr, ni = (Ur - pr) / a, (Ui - pi) / a
            dd = (Ur[..., idx, idx, :] - ((kr * vr) + (ki * vi))) / a
            keep = (idx[:, None] < idx[None, :])[..., None]
            Ur, Ui = np.where(keep, nr, Ur), np.where(keep, ni, Ui)
            Ur[..., idx, idx, :] = dd
            # taps
            pr, pi = _mulc(kr[..., :, None, :], ki[..., :, None, :], er[..., None, :, :], ei[..., None, :, :])
            gr, gi = gr + pr, gi + pi
    Z = np.zeros(lead + (L, M, bins), dt)
    Qn = _pack(Ur.astype(dt), Ui.astype(dt), Z, Z, M, K, dt)[..., :L * L, :]
    return out, Qn, _join(gr.astype(dt), gi.astype(dt), dt)


def dereverb_spec(Y, K, D, iterations=3, loading=1e-3, floor=1e-10, dt=f32):
    """crlot_wpe between its two transforms: `iterations` rounds of steps 1 - 4."""
    Z = np.asarray(Y)
    M = Z.shape[-3]
    for _ in range(iterations):
        S = accumulate(Y, power(Z, floor, dt), K, D, dt=dt)
        Z = filt(Y, solve(S, M, K, loading, dt), K, D, dt)
    return Z


# ------------------------------------------------------------------ the float64 model
def cov_full(Qp, L):
    """Hermitian planes [..., L L, bins] -> [..., bins, L, L] complex128."""
    Qp = np.asarray(Qp, np.float64)
    A = np.zeros(Qp.shape[:-2] + (Qp.shape[-1], L, L), np.complex128)
    for i in range(L):
        A[..., i, i] = Qp[..., i, :]
        for j in range(i + 1, L):
            v = Qp[..., re_plane(L, i, j), :] + 1j * Qp[..., re_plane(L, i, j) + 1, :]
            A[..., i, j], A[..., j, i] = v, np.conj(v)
    return A


def model_stats(Y, Z, K, D, floor=1e-10):
    """R [..., bins, L, L], P [..., bins, L, M] (steps 1 - 2) in complex128."""
    Y = np.asarray(Y, np.complex128)
    Z = np.asarray(Z, np.complex128)
    lam = np.maximum(np.mean(np.abs(Z) ** 2, axis=-3), floor)
    St = stacked(Y, K, D)
    R = np.einsum("...lfb,...fb,...kfb->...blk", St, 1.0 / lam, np.conj(St))
    P = np.einsum("...lfb,...fb,...mfb->...blm", St, 1.0 / lam, np.conj(Y))
    return R, P


def model_taps(R, P, loading=1e-3):
    L = R.shape[-1]
    ld = np.maximum(loading * np.real(np.trace(R, axis1=-2, axis2=-1)) / L, TINY)
    return np.linalg.solve(R + ld[..., None, None] * np.eye(L), P)  # [..., bins, L, M]


def model_filter(Y, G, K, D):
    Y = np.asarray(Y, np.complex128)
    return Y - np.einsum("...blm,...lfb->...mfb", np.conj(G), stacked(Y, K, D))


def model_offline(Y, K, D, iterations=3, loading=1e-3, floor=1e-10):
    Z = np.asarray(Y, np.complex128)
    for _ in range(iterations):
        R, P = model_stats(Y, Z, K, D, floor)
        Z = model_filter(Y, model_taps(R, P, loading), K, D)
    return Z


def model_rls(Y, K, D, alpha=0.9999, floor=1e-10, Q=None, G=None):
    """Step 5 in complex128 over every frame: (out [..., M, F, bins], Q [..., bins, L, L], G [..., bins, L, M])."""
    Y = np.asarray(Y, np.complex128)
    M, F, bins = Y.shape[-3:]
    L = M * K
    lead = Y.shape[:-3]
    Q = np.broadcast_to(np.eye(L, dtype=np.complex128), lead + (bins, L, L)).copy() if Q is None else np.array(Q)
    G = np.zeros(lead + (bins, L, M), np.complex128) if G is None else np.array(G)
    St = stacked(Y, K, D)
    lam = np.maximum(np.mean(np.abs(Y) ** 2, axis=-3), floor)
    out = np.zeros(Y.shape, np.complex128)
    for t in range(F):
        y = np.moveaxis(St[..., t, :], -1, -2)      # [..., bins, L]
        x = np.moveaxis(Y[..., t, :], -1, -2)       # [..., bins, M]
        pred = x - np.einsum("...lm,...l->...m", np.conj(G), y)
        v = np.einsum("...ij,...j->...i", Q, y)
        den = np.maximum(alpha * lam[..., t, :] + np.real(np.einsum("...i,...i->...", np.conj(y), v)), TINY)
        k = v / den[..., None]
        Q = (Q - k[..., :, None] * np.conj(v)[..., None, :]) / alpha
        G = G + k[..., :, None] * np.conj(pred)[..., None, :]
        out[..., t, :] = np.moveaxis(pred, -1, -2)
    return out, Q, G


# ------------------------------------------------------------------ the scene
def scene(M, seconds=3.0, rate=16000, t60=0.25, ir_taps=2048, early=384, seed=0):
    """A white source gated on and off in 50 ms blocks under, per microphone, an impulse
    response of white noise under a 10^(-3 t / T60) envelope with h[0] = 1.  Returns (x, e):
    the microphone signals and the early signals (the first `early` taps alone), [M, T] float64."""
    rng = np.random.default_rng(seed)
    T = int(seconds * rate)
    blk = int(0.05 * rate)
    gate = (np.arange(T) // blk) % 2 == 0
    src = rng.standard_normal(T) * gate
    env = 10.0 ** (-3.0 * np.arange(ir_taps) / (t60 * rate))
    x, e = np.zeros((M, T)), np.zeros((M, T))
    for m in range(M):
        h = rng.standard_normal(ir_taps) * env
        h[0] = 1.0
        x[m] = np.convolve(src, h)[:T]
        e[m] = np.convolve(src, h[:early])[:T]
    return x, e


def error_db(X, E, frames=slice(None)):
    """10 log10 of sum |X - E|^2 / sum |E|^2 over all channels, the frames given and all bins."""
    X, E = np.asarray(X, np.complex128)[..., frames, :], np.asarray(E, np.complex128)[..., frames, :]
    return 10.0 * np.log10(np.sum(np.abs(X - E) ** 2) / np.sum(np.abs(E) ** 2))
