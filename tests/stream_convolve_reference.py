"""Reference of the streaming convolver (include/crlot_dsp.h, "streaming convolution"),
on top of tests/convolve_reference.py.  numpy only.  One float32 model -- the same
transform pair, the same exactly rounded fmaf, the same overlap-add -- run two ways:

whole_signal(x, h, B, F_out)   crlot_convolve's chain over the whole signal: X_j for j < F_in =
                               ceil(T / B), frame f's chain over j = max(0, f-P+1) .. min(f, F_in-1)
                               (rows j >= F_in are not loaded), every block f < F_out
HopMachine(h, B, channels)     the per-hop state machine: a ring of P spectrum rows, the partial
                               chain `pre` (split=True: formed after each hop for the next frame,
                               the hop adds the last term; split=False: the hop runs the whole
                               chain over the ring), the carry; push(None) is a block of zeros

fmaf(a, b, c)                  float32 fused multiply-add, exactly rounded: the product is exact in
                               float64, the sum is rounded to odd there (two-sum), then once to float32
transforms                     fwd(frame 2B float32) -> B + 1 complex64, inv(B + 1 complex64) -> 2B
                               float32 already times 1/N.  Default: numpy's float64 FFT rounded to
                               float32; KissPair(oracle, B) is the oracle's kiss_fftr pair
"""
import numpy as np

import convolve_reference as CR

F32 = np.float32


def fmaf(a, b, c):
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)   # exact: 48-bit product, exponents in range
        c64 = c.astype(np.float64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)                  # two-sum: p + c = s + err exactly
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)      # round to odd
        return s.astype(F32)


def mac(re, im, H, X):
    """One term of the chain on arrays of bins: the four fmaf in the contract's order."""
    Hr, Hi, Xr, Xi = F32(H.real), F32(H.imag), F32(X.real), F32(X.imag)
    re = fmaf(Hr, Xr, re)
    re = fmaf(-Hi, Xi, re)
    im = fmaf(Hr, Xi, im)
    im = fmaf(Hi, Xr, im)
    return re, im


def np_fwd(frame):
    return np.fft.rfft(np.asarray(frame, np.float64)).astype(np.complex64)


def np_inv(spec):
    return np.fft.irfft(np.asarray(spec, np.complex128), n=2 * (len(spec) - 1)).astype(F32)


class KissPair:
    """The oracle's kiss_fftr / kiss_fftri at N = 2B (its inverse is already scaled by 1/N)."""

    def __init__(self, oracle, B):
        self.plan = oracle.KissR(2 * B)

    def fwd(self, frame):
        return np.asarray(self.plan.forward(np.ascontiguousarray(frame, F32)), np.complex64)

    def inv(self, spec):
        return np.asarray(self.plan.inverse(np.ascontiguousarray(spec, np.complex64)), F32)


def filter_spectra(h, B, fwd=np_fwd):
    hb = CR._blocks(CR._rows(np.asarray(h, F32)), B)
    return np.array([[fwd(hb[q, p]) for p in range(hb.shape[1])] for q in range(hb.shape[0])])


def analyse(block, B, fwd):
    frame = np.zeros(2 * B, F32)
    frame[:B] = CR.sanitize(np.asarray(block, F32))
    return fwd(frame)


def synthesise(re, im, carry, inv):
    """(block, new carry): inverse, sanitize, fma(fma(o, 1, 0), 1, acc), the division by 1."""
    spec = (re + F32(0.0)) + 1j * (im + F32(0.0))
    o = CR.sanitize(inv(spec.astype(np.complex64)))
    B = len(carry)
    one, zero = F32(1.0), F32(0.0)
    block = fmaf(fmaf(o[:B], one, zero), one, carry) / one
    return block, fmaf(fmaf(o[B:], one, zero), one, np.zeros(B, F32))


def whole_signal(x, h, B, F_out, fwd=np_fwd, inv=np_inv):
    x = np.asarray(x, F32)
    x = x[None] if x.ndim == 1 else x
    C, T = x.shape
    H = filter_spectra(h, B, fwd)
    nf, P = H.shape[:2]
    F_in = -(-T // B)
    xp = np.zeros((C, F_in * B), F32)
    xp[:, :T] = x
    y = np.zeros((C, F_out * B), F32)
    for c in range(C):
        X = [analyse(xp[c, j * B:(j + 1) * B], B, fwd) for j in range(F_in)]
        carry = np.zeros(B, F32)
        for f in range(F_out):
            re, im = np.zeros(B + 1, F32), np.zeros(B + 1, F32)
            for j in range(max(0, f - P + 1), min(f, F_in - 1) + 1):
                re, im = mac(re, im, H[c % nf, f - j], X[j])
            y[c, f * B:(f + 1) * B], carry = synthesise(re, im, carry, inv)
    return y


class HopMachine:
    def __init__(self, h, B, channels, split=True, fwd=np_fwd, inv=np_inv):
        self.B, self.C, self.split, self.fwd, self.inv = B, channels, split, fwd, inv
        self.H = filter_spectra(h, B, fwd)
        self.nf, self.P = self.H.shape[:2]
        self.reset()

    def reset(self):
        B, C, P = self.B, self.C, self.P
        self.ring = np.zeros((C, P, B + 1), np.complex64)   # zero rows: hops that have not happened
        self.pre = np.zeros((C, 2, B + 1), F32)
        self.carry = np.zeros((C, B), F32)
        self.k = 0

    def _terms(self, c, f, re, im, upto):
        """Frame f's terms j = f-P+1 .. upto ascending from the ring; a negative j is a zero row."""
        for j in range(f - self.P + 1, upto + 1):
            X = self.ring[c, j % self.P] if j >= 0 else np.zeros(self.B + 1, np.complex64)
            re, im = mac(re, im, self.H[c % self.nf, f - j], X)
        return re, im

    def push(self, block):
        B, C, P, k = self.B, self.C, self.P, self.k
        out = np.zeros((C, B), F32)
        for c in range(C):
            x = np.zeros(B, F32) if block is None else block[c]
            self.ring[c, k % P] = analyse(x, B, self.fwd)
            if self.split:   # the head: the last term on top of the partial chain
                re, im = mac(self.pre[c, 0], self.pre[c, 1], self.H[c % self.nf, 0], self.ring[c, k % P])
            else:
                re, im = self._terms(c, k, np.zeros(B + 1, F32), np.zeros(B + 1, F32), upto=k)
            out[c], self.carry[c] = synthesise(re, im, self.carry[c], self.inv)
            if self.split:   # the tail: frame k + 1's partial chain, raw, from +0
                pr, pi = self._terms(c, k + 1, np.zeros(B + 1, F32), np.zeros(B + 1, F32), upto=k)
                self.pre[c, 0], self.pre[c, 1] = pr, pi
        self.k += 1
        return out


def run_hops(machine, x, F_total):
    """Push x (C, T) block by block, the last block zero-padded by the caller, then None
    blocks up to F_total hops.  Returns (C, F_total B)."""
    x = np.asarray(x, F32)
    C, T = x.shape
    B = machine.B
    F_in = -(-T // B)
    xp = np.zeros((C, F_in * B), F32)
    xp[:, :T] = x
    blocks = [machine.push(xp[:, j * B:(j + 1) * B] if j < F_in else None) for j in range(F_total)]
    return np.concatenate(blocks, axis=1)
