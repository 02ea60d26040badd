"""numpy reference of the noise suppressor (include/crlot_dsp.h, "noise suppressor"): the
contract's recurrence in float64 (the model) and restated operation for operation in
float32 (what the kernels compute bit for bit), the test signal (harmonic bursts plus
white noise), a float64 STFT / overlap-add, and the two behaviour figures.  Imported by
the CPU and the GPU tests; needs numpy only."""
import numpy as np

f32 = np.float32
DEFAULTS = dict(alpha_s=0.8, alpha_p=0.2, alpha_d=0.95, delta=5.0, window=64, alpha_dd=0.98, g_min=0.1)
PLANES = ("S", "Smin", "Stmp", "p", "lam", "A2")


def constants(dt, **params):
    """The descriptor as the kernels read it: each factor rounded to dt, its complement
    dt(1 - factor) formed in double."""
    v = {**DEFAULTS, **params}
    c = {"window": int(v["window"]), "delta": dt(v["delta"]), "g_min": dt(v["g_min"])}
    for name in ("s", "p", "d", "dd"):
        a = float(v["alpha_" + name])
        c["alpha_" + name] = dt(a)
        c["omega_" + name] = dt(1.0 - a)
    return c


def _mx(a, b):
    return np.where(a > b, a, b)


def _mn(a, b):
    return np.where(a < b, a, b)


def power(X, dt=f32):
    """Step 1 on complex rows: (Xr Xr) + (Xi Xi), each operation rounded in dt."""
    re, im = X.real.astype(dt), X.imag.astype(dt)
    return (re * re) + (im * im)


def gains(P, dt=f32, state=None, k0=0, **params):
    """Steps 2 - 5 over P[..., F, bins] (frames along axis -2), every operation rounded in
    dt on its own.  state: the six planes [..., 6, bins] after frame k0 - 1 (None: fresh,
    k0 must be 0).  Returns (G like P, the state after the last frame)."""
    c = constants(dt, **params)
    P = np.asarray(P, dt)
    F = P.shape[-2]
    one, zero, tiny = dt(1), dt(0), dt(1e-30)
    if state is None:
        assert k0 == 0
        S = Smin = Stmp = pp = lam = A2 = None
    else:
        S, Smin, Stmp, pp, lam, A2 = (np.array(state[..., j, :], dt) for j in range(6))
    G = np.empty(P.shape, dt)
    with np.errstate(all="ignore"):
        for f in range(F):
            k, p_ = k0 + f, P[..., f, :]
            if k == 0:
                S, Smin, Stmp, lam = p_.copy(), p_.copy(), p_.copy(), p_.copy()
                pp, A2 = np.zeros_like(p_), np.zeros_like(p_)
            else:
                S = (c["alpha_s"] * S) + (c["omega_s"] * p_)
                if k % c["window"] == 0:
                    Smin = _mn(Stmp, S)
                    Stmp = S.copy()
                else:
                    Smin = _mn(Smin, S)
                    Stmp = _mn(Stmp, S)
                present = S > (c["delta"] * Smin)
                pp = (c["alpha_p"] * pp) + np.where(present, c["omega_p"], zero)
                ad = c["alpha_d"] + (c["omega_d"] * pp)
                lam = (ad * lam) + ((one - ad) * p_)
            lc = _mx(lam, tiny)
            gamma = p_ / lc
            xi = (c["alpha_dd"] * (A2 / lc)) + (c["omega_dd"] * _mx(gamma - one, zero))
            g = _mx(xi / (one + xi), c["g_min"])
            A2 = (g * g) * p_
            G[..., f, :] = g
    st = np.stack([np.asarray(v, dt) for v in (S, Smin, Stmp, pp, lam, A2)], axis=-2) if F or state is not None else None
    return G, st


# ----------------------------------------------------------------- signal and transforms
def sqrt_hann(n):
    return np.sqrt(np.hanning(n + 1)[:n])


def bursts(N, H, F, seed=7, fs=16000.0, snr_db=5.0):
    """Harmonic bursts at unit power (on and off every 10 frames up to 40 frames, every
    0.3 s beyond) plus white noise at snr_db.  Returns (s, v, on): clean, noise, burst flag."""
    rng = np.random.default_rng(seed)
    T = N + (F - 1) * H
    n = np.arange(T)
    t = n / fs
    on = ((n // H // 10) % 2 == 1) if F <= 40 else ((t // 0.3) % 2 == 1)
    s = sum(np.sin(2 * np.pi * 150 * h * t + h) / h for h in range(1, 11)) * on
    s = s / np.sqrt(np.mean(s[on] ** 2))
    v = rng.standard_normal(T) * 10 ** (-snr_db / 20)
    return s, v, on


def stft(x, N, H, w):
    F = (len(x) - N) // H + 1
    return np.stack([np.fft.rfft(x[k * H:k * H + N] * w) for k in range(F)])


def istft(X, N, H, w, T):
    y, d = np.zeros(T), np.zeros(T)
    for k in range(X.shape[0]):
        y[k * H:k * H + N] += np.fft.irfft(X[k], N) * w
        d[k * H:k * H + N] += w * w
    return y / np.maximum(d, 1e-9)


def behaviour(G, s, v, on, N, H, w, y=None):
    """The two figures over the second half of the run, the last frame's tail excluded:
    the noise removed in the gaps (dB; y: the suppressor's output, default the float64
    chain under G) and the SNR gain inside the bursts, the clean and the noise part run
    through the same gains G apart (dB)."""
    T = len(s)
    G = np.asarray(G, np.float64)
    if y is None:
        y = istft(stft(s + v, N, H, w) * G, N, H, w, T)
    ys = istft(stft(s, N, H, w) * G, N, H, w, T)
    yv = istft(stft(v, N, H, w) * G, N, H, w, T)
    m = slice(T // 2, T - N)
    off, onm = (~on)[m], on[m]
    nr_gap = 10 * np.log10(np.mean(v[m][off] ** 2) / np.mean(np.asarray(y, np.float64)[m][off] ** 2))
    snr_in = 10 * np.log10(np.mean(s[m][onm] ** 2) / np.mean(v[m][onm] ** 2))
    snr_out = 10 * np.log10(np.mean(ys[m][onm] ** 2) / np.mean(yv[m][onm] ** 2))
    return float(nr_gap), float(snr_out - snr_in)
