"""References of partitioned FFT convolution (include/crlot_dsp.h, "partitioned FFT
convolution").  numpy only.

sanitize(x)                          NaN / Inf -> 0, |v| < 1e-30 -> 0 (the forward's rule)
partition_f64(h, B)                  H (n_filters, P, B + 1) complex128: the DFT of every block of B
                                     taps zero-padded to 2B
chain_terms(F_in, P, F_out)          terms of each output frame's chain
fdl_mac_f64(X, H, F_out)             (Y, scale_re, scale_im): the plain sum over j of H[f - j] X[j] in
                                     complex128 and, beside it, sum(|Hr Xr| + |Hi Xi|) and
                                     sum(|Hr Xi| + |Hi Xr|), the error bound's scales
overlap_add_f64(Y, B, L)             irfft of every frame, overlap-added at hop B, cropped to L
convolve_f64(x, h)                   np.convolve in float64 of the sanitized x, filter s mod n_filters
convolve_oracle_f32(oracle, x, h, B) the same partitioned algorithm in float32 on the CPU: the
                                     oracle's kiss_fftr per block, the contract's chain with each
                                     product and sum rounded to float32, the oracle's inverse, a
                                     float32 overlap-add
fma_bound(n)                         gamma_n = n 2^-24 / (1 - n 2^-24)
error_figures(y, y64)                per stream (rel-L2, max-abs / max|y64|)
bars(oracle_l2, oracle_peak)         the larger of the project's 1e-6 / 4e-6 and 4x the oracle's figure
make_streams(S, T, B, seed)          the GPU tests' input: white noise, a silent block-aligned
                                     stretch, a 2^12 level step
make_filter(n_filters, K, seed)      decaying noise, a room-like tail
"""
import numpy as np

REL_L2 = 1e-6   # the project's bars (tests/spec_reference.py SPEC_REL_L2, SPEC_MAX_ABS)
MAX_ABS = 4e-6

# crlot_convolve's accuracy cases, shared by the CPU record of the oracle's own
# error and the GPU test: (B, T, K, S, n_filters)
ACCURACY_CASES = [(128, 70 * 128 - 5, 37 * 128 - 9, 3, 2), (512, 9 * 512 + 3, 3 * 512 + 7, 5, 5),
                  (256, 6 * 256 + 1, 256 + 1, 1, 1)]


def sanitize(x):
    x = np.asarray(x)
    a = np.abs(x)
    with np.errstate(invalid="ignore"):
        keep = np.isfinite(x) & (a >= np.float32(1e-30))
    return np.where(keep, x, 0).astype(x.dtype)


def _rows(h):
    h = np.asarray(h)
    return h[None] if h.ndim == 1 else h


def _blocks(h, B):
    """(n_filters, K) -> (n_filters, P, 2B): block p of every filter zero-padded to 2B."""
    h = _rows(h)
    nf, K = h.shape
    P = -(-K // B)
    out = np.zeros((nf, P, 2 * B), h.dtype)
    for p in range(P):
        seg = h[:, p * B:min(K, (p + 1) * B)]
        out[:, p, :seg.shape[1]] = seg
    return out


def partition_f64(h, B):
    return np.fft.rfft(_blocks(np.asarray(h, np.float64), B), axis=-1)


def chain_terms(F_in, P, F_out):
    f = np.arange(F_out)
    return np.maximum(0, np.minimum(f, F_in - 1) - np.maximum(0, f - P + 1) + 1)


def fdl_mac_f64(X, H, F_out):
    """X: (S, F_in, bins) complex, H: (n_filters, P, bins) complex -> (Y, scale_re,
    scale_im), (S, F_out, bins) complex128 / float64 / float64."""
    X = np.asarray(X, np.complex128)
    H = np.asarray(H, np.complex128)
    S, F_in, bins = X.shape
    nf, P, _ = H.shape
    Y = np.zeros((S, F_out, bins), np.complex128)
    sr = np.zeros((S, F_out, bins))
    si = np.zeros((S, F_out, bins))
    for s in range(S):
        Hq = H[s % nf]
        for p in range(P):
            lo, hi = p, min(F_out, F_in + p)   # output frames f with j = f - p in [0, F_in)
            if hi <= lo:
                continue
            x = X[s, lo - p:hi - p]
            hp = Hq[p][None]
            Y[s, lo:hi] += hp * x
            sr[s, lo:hi] += np.abs(hp.real * x.real) + np.abs(hp.imag * x.imag)
            si[s, lo:hi] += np.abs(hp.real * x.imag) + np.abs(hp.imag * x.real)
    return Y, sr, si


def overlap_add_f64(Y, B, L):
    S, F, _ = Y.shape
    fr = np.fft.irfft(Y, n=2 * B, axis=-1)
    y = np.zeros((S, (F + 1) * B))
    for f in range(F):
        y[:, f * B:f * B + 2 * B] += fr[:, f]
    return y[:, :L]


def convolve_f64(x, h):
    x = sanitize(np.asarray(x, np.float32)).astype(np.float64)
    x = x[None] if x.ndim == 1 else x
    h = _rows(np.asarray(h, np.float64))
    return np.stack([np.convolve(x[s], h[s % h.shape[0]]) for s in range(x.shape[0])])


def _f32(v):
    return np.asarray(v, np.float32)


def convolve_oracle_f32(oracle, x, h, B):
    """(S, T + K - 1) float32: the partitioned algorithm as a float32 CPU program."""
    x = np.asarray(x, np.float32)
    x = x[None] if x.ndim == 1 else x
    h = _rows(np.asarray(h, np.float32))
    S, T = x.shape
    nf, K = h.shape
    N, P = 2 * B, -(-K // B)
    F_in, L = -(-T // B), T + K - 1
    F_out = -(-L // B)
    plan = oracle.KissR(N)
    hb = _blocks(h, B)
    H = np.array([[plan.forward(hb[q, p]) for p in range(P)] for q in range(nf)])
    y = np.zeros((S, (F_out + 1) * B), np.float32)
    xp = np.zeros(F_in * B, np.float32)
    for s in range(S):
        xp[:] = 0
        xp[:T] = x[s]
        X = np.array([plan.forward(np.concatenate([xp[j * B:(j + 1) * B], np.zeros(B, np.float32)]))
                      for j in range(F_in)])
        Hq = H[s % nf]
        Hr, Hi, Xr, Xi = _f32(Hq.real), _f32(Hq.imag), _f32(X.real), _f32(X.imag)
        for f in range(F_out):
            re = np.zeros(B + 1, np.float32)
            im = np.zeros(B + 1, np.float32)
            for j in range(max(0, f - P + 1), min(f, F_in - 1) + 1):
                p = f - j
                re = _f32(re + _f32(Hr[p] * Xr[j]))
                re = _f32(re - _f32(Hi[p] * Xi[j]))
                im = _f32(im + _f32(Hr[p] * Xi[j]))
                im = _f32(im + _f32(Hi[p] * Xr[j]))
            fr = plan.inverse((re + 1j * im).astype(np.complex64))
            y[s, f * B:f * B + N] = _f32(y[s, f * B:f * B + N] + fr)
    return y[:, :L]


def fma_bound(n):
    u = n * 2.0 ** -24
    return u / (1.0 - u)


def error_figures(y, y64):
    """Per stream: (rel-L2, max-abs over max|y64|); a silent reference stream gives (0, 0)
    when y is silent too, else (inf, inf)."""
    y = np.asarray(y, np.float64)
    y64 = np.asarray(y64, np.float64)
    out = []
    for a, b in zip(y, y64):
        d = a - b
        nb, pk = np.sqrt(np.sum(b * b)), np.max(np.abs(b))
        if pk == 0.0:
            out.append((0.0, 0.0) if not np.any(d) else (np.inf, np.inf))
        else:
            out.append((float(np.sqrt(np.sum(d * d)) / nb), float(np.max(np.abs(d)) / pk)))
    return out


def bars(oracle_l2=0.0, oracle_peak=0.0):
    return max(REL_L2, 4.0 * oracle_l2), max(MAX_ABS, 4.0 * oracle_peak)


def make_streams(S, T, B, seed=0):
    """(S, T) float32 white noise in [-0.5, 0.5) scaled by 2^-6; stream s is silent over
    block s + 1 (block-aligned, where T reaches it) and 2^12 louder from sample 2 T / 3."""
    rng = np.random.default_rng(1000 + seed)
    x = (rng.random((S, T), np.float32) - np.float32(0.5)) * np.float32(2.0 ** -6)
    for s in range(S):
        x[s, (s + 1) * B:(s + 2) * B] = 0.0
        x[s, (2 * T) // 3:] *= np.float32(2.0 ** 12)
    return x


def make_filter(n_filters, K, seed=0):
    rng = np.random.default_rng(2000 + seed)
    k = np.arange(K, dtype=np.float64)
    h = rng.standard_normal((n_filters, K)) * np.exp(-4.0 * k / max(K, 1))[None]
    return (h / np.sqrt(max(K, 1) / 8.0 + 1.0)).astype(np.float32)
