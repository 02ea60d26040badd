"""Reference of the adaptive filter (include/crlot_dsp.h, "adaptive filter"), numpy only.
Two models of the contract's steps 1 - 8, both per hop and per channel:

F64Model(B, K, channels, ...)   float64 throughout on numpy's FFT: what the algorithm computes.
F32Model(B, K, channels, ...)   float32: steps 3, 6 and 7 bit-exactly as the contract orders them
                                (stream_convolve_reference's exactly rounded fmaf; every product,
                                sum and quotient of step 6 rounded on its own), the transforms
                                pluggable: numpy's float64 FFT rounded to float32 (default) or the
                                oracle's kiss_fftr pair (stream_convolve_reference.KissPair).

The float32 steps are also plain functions on arrays of bins, for a caller that has the
spectra (the GPU tests apply them to the device's own state):
chain(W, ring, k)               step 3: Y of hop k from the weight rows and the ring, with + 0.0f
power(pw, X, k, cst)            step 6: the power estimate after hop k
gradient(pw, E, cst)            step 6: G
update(W, ring, G, k)           step 7: the new W; rows p > k are returned untouched
constants(mu, lam, delta, P)    (mu_P, lambda, omega, delta) as crlot_fdaf_set_step stores them

Spectra are complex64 / complex128 arrays of B + 1 bins; W and ring are (..., P, B + 1).
misalignment_db(h_hat, h) is 10 log10(|h_hat - h|^2 / |h|^2); make_case(B, P, hops, seed)
the identification problem of the convergence tests.
"""
import numpy as np

import convolve_reference as CR
import stream_convolve_reference as SR

F32 = np.float32


def constants(mu, lam, delta, P):
    return F32(float(mu) / float(P)), F32(lam), F32(1.0 - float(lam)), F32(delta)


def chain(W, ring, k):
    P = W.shape[-2]
    re = np.zeros(W.shape[:-2] + W.shape[-1:], F32)
    im = np.zeros_like(re)
    for j in range(max(0, k - P + 1), k + 1):
        re, im = SR.mac(re, im, W[..., k - j, :], ring[..., j % P, :])
    return ((re + F32(0.0)) + 1j * (im + F32(0.0))).astype(np.complex64)


def power(pw, X, k, cst):
    _, lam, omega, _ = cst
    xr, xi = F32(X.real), F32(X.imag)
    m = (xr * xr) + (xi * xi)
    return m if k == 0 else (lam * np.asarray(pw, F32)) + (omega * m)


def gradient(pw, E, cst):
    mu_p, _, _, delta = cst
    g = mu_p / (np.asarray(pw, F32) + delta)
    return ((g * F32(E.real)) + 1j * (g * F32(E.imag))).astype(np.complex64)


def update(W, ring, G, k):
    P = W.shape[-2]
    out = np.array(W, np.complex64)
    gr, gi = F32(G.real), F32(G.imag)
    for p in range(min(k + 1, P)):
        X = ring[..., (k - p) % P, :]
        xr, xi = F32(X.real), F32(X.imag)
        re = SR.fmaf(xr, gr, F32(W[..., p, :].real))
        re = SR.fmaf(xi, gi, re)
        im = SR.fmaf(xr, gi, F32(W[..., p, :].imag))
        im = SR.fmaf(-xi, gr, im)
        out[..., p, :] = re + 1j * im
    return out


def _f64_fwd(frame):
    return np.fft.rfft(np.asarray(frame, np.float64))


def _f64_inv(spec):
    return np.fft.irfft(np.asarray(spec, np.complex128), n=2 * (len(spec) - 1))


class _Model:
    """The state machine both models share; a subclass supplies the arithmetic."""

    def __init__(self, B, K, channels, mu=0.5, lam=0.9, delta=1e-3, mode=1, adapt=True):
        self.B, self.K, self.C, self.P = B, K, channels, -(-K // B)
        self.mu, self.lam, self.delta, self.mode, self.adapt = mu, lam, delta, mode, adapt
        self.reset()

    def reset(self):
        B, C, P = self.B, self.C, self.P
        self.ring = np.zeros((C, P, B + 1), self.ctype)
        self.W = np.zeros((C, P, B + 1), self.ctype)
        self.pw = np.zeros((C, B + 1), self.rtype)
        self.E = np.zeros((C, B + 1), self.ctype)
        self.G = np.zeros((C, B + 1), self.ctype)
        self.prev = np.zeros((C, B), self.rtype)
        self.k = 0

    def set_taps(self, h):
        h = np.asarray(h, self.rtype)
        h = h[None] if h.ndim == 1 else h
        for c in range(self.C):
            row = np.zeros(self.P * self.B, self.rtype)
            row[:self.K] = h[c % len(h)]
            for p in range(self.P):
                frame = np.zeros(2 * self.B, self.rtype)
                frame[:self.B] = row[p * self.B:(p + 1) * self.B]
                self.W[c, p] = self.fwd(frame)

    def taps(self):
        out = np.zeros((self.C, self.P * self.B), self.rtype)
        for c in range(self.C):
            for p in range(self.P):
                out[c, p * self.B:(p + 1) * self.B] = self.inv(self.W[c, p])[:self.B]
        return out[:, :self.K]

    def constrain(self, p=-1):
        for c in range(self.C):
            for q in (range(self.P) if p < 0 else (p,)):
                w = np.array(self.inv(self.W[c, q]))
                w[self.B:] = 0
                self.W[c, q] = self.fwd(w)

    def push(self, x, d):
        """x: (C, B) or None for a block of zeros; d: (C, B).  Returns (e, y), each (C, B)."""
        B, C, P, k = self.B, self.C, self.P, self.k
        e = np.zeros((C, B), self.rtype)
        y = np.zeros((C, B), self.rtype)
        for c in range(C):
            xb = np.zeros(B, self.rtype) if x is None else CR.sanitize(np.asarray(x[c], F32)).astype(self.rtype)
            db = CR.sanitize(np.asarray(d[c], F32)).astype(self.rtype)
            self.ring[c, k % P] = self.fwd(np.concatenate([self.prev[c], xb]))
            self.prev[c] = xb
            y[c] = self.filter_output(c, k)
            e[c] = db - y[c]
            if self.adapt:
                self.E[c] = self.fwd(np.concatenate([np.zeros(B, self.rtype), self.clean(e[c])]))
        self.step_6_7(k)
        if self.adapt and self.mode == 1:
            self.constrain(k % P)
        elif self.adapt and self.mode == 2:
            self.constrain(-1)
        self.k += 1
        return e, y


class F64Model(_Model):
    ctype, rtype = np.complex128, np.float64
    fwd, inv = staticmethod(_f64_fwd), staticmethod(_f64_inv)

    @staticmethod
    def clean(v):
        return v

    def filter_output(self, c, k):
        Y = np.zeros(self.B + 1, np.complex128)
        for j in range(max(0, k - self.P + 1), k + 1):
            Y += self.W[c, k - j] * self.ring[c, j % self.P]
        return self.inv(Y)[self.B:]

    def step_6_7(self, k):
        P = self.P
        m = np.abs(self.ring[:, k % P]) ** 2
        self.pw = m if k == 0 else self.lam * self.pw + (1.0 - self.lam) * m
        if not self.adapt:
            return
        self.G = (self.mu / P) / (self.pw + self.delta) * self.E
        for p in range(min(k + 1, P)):
            self.W[:, p] += np.conj(self.ring[:, (k - p) % P]) * self.G


class F32Model(_Model):
    ctype, rtype = np.complex64, F32

    def __init__(self, B, K, channels, mu=0.5, lam=0.9, delta=1e-3, mode=1, adapt=True, fwd=SR.np_fwd, inv=SR.np_inv):
        self.fwd, self.inv = fwd, inv
        super().__init__(B, K, channels, mu, lam, delta, mode, adapt)
        self.cst = constants(mu, lam, delta, self.P)

    @staticmethod
    def clean(v):
        return CR.sanitize(v)

    def filter_output(self, c, k):
        return CR.sanitize(self.inv(chain(self.W[c], self.ring[c], k)))[self.B:]

    def step_6_7(self, k):
        self.pw = power(self.pw, self.ring[:, k % self.P], k, self.cst)
        if not self.adapt:
            return
        self.G = gradient(self.pw, self.E, self.cst)
        self.W = update(self.W, self.ring, self.G, k)


def misalignment_db(h_hat, h):
    h_hat, h = np.asarray(h_hat, np.float64), np.asarray(h, np.float64)
    num = float(np.sum((h_hat - h) ** 2))
    return 10.0 * np.log10(max(num, 1e-300) / float(np.sum(h ** 2)))


def make_case(B, P, hops, seed, channels=1):
    """x: (channels, hops B) seeded standard normal; h: (channels, K), K = P B - 5, normal times
    exp(-n / (K / 4)) scaled to unit norm; d: the float64 convolution truncated to x's length."""
    K = P * B - 5
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((channels, hops * B)).astype(F32)
    h = rng.standard_normal((channels, K)) * np.exp(-np.arange(K) / (K / 4.0))
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    d = np.array([np.convolve(x[c].astype(np.float64), h[c])[:hops * B] for c in range(channels)])
    return x, h, d


def run(model, x, d):
    """Push x and d (C, hops B) block by block; returns (e, y), each (C, hops B)."""
    B = model.B
    out = [model.push(None if x is None else x[:, j * B:(j + 1) * B], d[:, j * B:(j + 1) * B])
           for j in range(d.shape[1] // B)]
    return np.concatenate([o[0] for o in out], axis=1), np.concatenate([o[1] for o in out], axis=1)
