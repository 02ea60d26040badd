"""GPU tests of partitioned FFT convolution (include/crlot_dsp.h, "partitioned FFT
convolution"): crlot_fdl_mac against the float64 sum within the derived fmaf-chain
bound; its bits independent of chunking, batch and leading dimensions, and memory
containment; crlot_convolve equal to stft -> fdl_mac -> istft_ola through the borrowed
plan, bit for bit, with pairing on and off and in two slices; its accuracy against
np.convolve in float64 under the bar the float32 CPU oracle sets; exact zeros, the
identity filter, untouched tails; the launch records; errors and empties.

Inputs (tests/convolve_reference.py make_streams): white noise, a silent block-aligned
stretch per stream and a 2^12 level step.
"""
import functools

import numpy as np
import pytest

import convolve_reference as CR

pytestmark = pytest.mark.gpu

F_IN = 70


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_convs = {}


def conv_for(pkg, B, K, nf=1, seed=0):
    key = (B, K, nf, seed)
    if key not in _convs:
        h = CR.make_filter(nf, K, seed)
        _convs[key] = (pkg.Convolver(h, block=B), h)
    return _convs[key]


@functools.lru_cache(maxsize=None)
def streams(S, T, B, seed=0):
    x = CR.make_streams(S, T, B, seed)
    x.setflags(write=False)
    return x


def spectra_of(torch, conv, x):
    """The engine plan's spectra of x, on the device and as float32 pairs on the host."""
    X = conv.plan.stft(torch.from_numpy(np.array(x)).cuda())
    torch.cuda.synchronize()
    return X, X.cpu().numpy()


# ------------------------------------------------------------------ 1. the delay line against float64
# (B, P, S, n_filters): P = 1 and 2 (the tiles of one and two frames), 4 (tile 4), 37
# (tile 8: edge and interior blocks), 512-point blocks (9 bin blocks, the last one lane);
# every S and n_filters in {1, 2, S}
FDL_CASES = [(128, 1, 1, 1), (128, 2, 3, 2), (128, 4, 5, 5), (128, 37, 3, 1), (128, 37, 5, 2), (512, 3, 3, 3)]


@pytest.mark.parametrize("B,P,S,nf", FDL_CASES)
def test_fdl_mac_within_the_fma_chain_bound(pkg, torch_cuda, B, P, S, nf):
    """Every output within gamma_n * scale + 2^-149 of the float64 sum over the same float32
    X and H, n = twice the terms of its chain (two fmaf per term and component), for
    F_out = F_in + P - 1 and for F_out < F_in.  Derived: a chain of n fmaf, each
    exactly rounded, is off by at most gamma_n times the sum of the |products|; 2^-149
    covers a last rounding into the subnormals."""
    torch = torch_cuda
    K = (P - 1) * B + 7 if P > 1 else B - 3
    conv, h = conv_for(pkg, B, K, nf, seed=P)
    assert conv.partitions == P
    X, Xh = spectra_of(torch, conv, streams(S, F_IN * B - 5, B, seed=B + P))
    assert Xh.shape == (S, F_IN, B + 1)
    H = conv.spectra()
    H64 = CR.partition_f64(h, B)
    assert H.shape == H64.shape == (nf, P, B + 1)
    assert np.max(np.abs(H - H64)) <= 4e-6 * np.max(np.abs(H64))
    for F_out in (F_IN + P - 1, 50):
        got = conv.fdl_mac(X, F_out=F_out)
        torch.cuda.synchronize()
        rec = conv.last_launch()
        assert rec["name"] == "k_fdl_mac" and rec["tile"] == (1 if P == 1 else 2 if P <= 3 else 4 if P < 12 else 8)
        got = got.cpu().numpy()
        want, sr, si = CR.fdl_mac_f64(Xh, H, F_out)
        n = 2 * CR.chain_terms(F_IN, P, F_out)
        bound = np.array([CR.fma_bound(int(v)) for v in n])[None, :, None]
        tiny = 2.0 ** -149
        er = np.abs(got.real.astype(np.float64) - want.real)
        ei = np.abs(got.imag.astype(np.float64) - want.imag)
        assert np.all(er <= bound * sr + tiny), float(np.max(er / (bound * sr + tiny)))
        assert np.all(ei <= bound * si + tiny), float(np.max(ei / (bound * si + tiny)))
        assert np.any(got.real != 0)


def test_fdl_mac_empty_ranges_store_plus_zero(pkg, torch_cuda):
    """F_out beyond F_in + P - 1: the frames no input reaches are +0, bit for bit; F_in = 0 too."""
    torch = torch_cuda
    B, P = 128, 4
    conv, _ = conv_for(pkg, B, (P - 1) * B + 7, 1, seed=P)
    X, _ = spectra_of(torch, conv, streams(2, 6 * B, B))
    out = torch.full((2, 6 + P + 4, B + 1), complex(7.0, -7.0), dtype=torch.complex64, device="cuda")
    conv.fdl_mac(X, out=out, F_out=6 + P + 4)
    torch.cuda.synchronize()
    tail = torch.view_as_real(out[:, 6 + P - 1:]).contiguous().view(torch.int32)
    assert int(tail.abs().max()) == 0
    assert bool(torch.any(out[:, 6 + P - 2] != 0))
    none = torch.zeros((2, 0, B + 1), dtype=torch.complex64, device="cuda")
    z = conv.fdl_mac(none, F_out=3)
    torch.cuda.synchronize()
    assert z.shape == (2, 3, B + 1) and int(torch.view_as_real(z).contiguous().view(torch.int32).abs().max()) == 0


# ------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("B,P", [(128, 37), (128, 2), (512, 3)])
def test_fdl_mac_bits_do_not_depend_on_chunks_batch_or_layout(pkg, torch_cuda, B, P):
    torch = torch_cuda
    S, bins = 3, B + 1
    K = (P - 1) * B + 7
    conv, _ = conv_for(pkg, B, K, 1, seed=P)
    X, _ = spectra_of(torch, conv, streams(S, F_IN * B - 5, B, seed=B + P))
    F_out = F_IN + P - 1
    conv.set_chunks(0)
    base = conv.fdl_mac(X)
    torch.cuda.synchronize()
    try:
        for n in (1, 2, 3, 5):
            conv.set_chunks(n)
            got = conv.fdl_mac(X)
            torch.cuda.synchronize()
            assert conv.last_launch()["n_chunks"] == n
            assert same_bits(torch, torch.view_as_real(got), torch.view_as_real(base)), n
    finally:
        conv.set_chunks(0)
    # each stream alone
    for s in range(S):
        one = conv.fdl_mac(X[s:s + 1].contiguous())
        torch.cuda.synchronize()
        assert same_bits(torch, torch.view_as_real(one[0]), torch.view_as_real(base[s])), s
    # padded leading dimensions on both sides; sentinels beyond the bins, between the
    # streams and after the last row
    big_in = torch.zeros((S, F_IN + 2, bins + 5), dtype=torch.complex64, device="cuda")
    big_in[:, :F_IN, :bins] = X
    sent = complex(-3.5, 9.25)
    big_out = torch.full((S + 1, F_out + 3, bins + 3), sent, dtype=torch.complex64, device="cuda")
    out = big_out[:S, :F_out, :bins]
    conv.fdl_mac(big_in[:, :F_IN, :bins], out=out)
    torch.cuda.synchronize()
    assert same_bits(torch, torch.view_as_real(out), torch.view_as_real(base))
    assert bool(torch.all(big_out[:S, :F_out, bins:] == sent)) and bool(torch.all(big_out[:S, F_out:] == sent))
    assert bool(torch.all(big_out[S] == sent))


def test_filter_follows_the_stream_index(pkg, torch_cuda):
    """Stream s uses filter s mod n_filters: a batch of 5 against two filters equals each
    stream run alone through a single-filter convolver of its filter."""
    torch = torch_cuda
    B, P, S = 128, 4, 5
    K = (P - 1) * B + 7
    conv, h = conv_for(pkg, B, K, 2, seed=9)
    X, _ = spectra_of(torch, conv, streams(S, 20 * B, B, seed=3))
    got = conv.fdl_mac(X)
    for q in range(2):
        single = pkg.Convolver(h[q], block=B)
        for s in range(q, S, 2):
            one = single.fdl_mac(X[s])
            torch.cuda.synchronize()
            assert same_bits(torch, torch.view_as_real(one), torch.view_as_real(got[s])), (q, s)
        single.close()


# ------------------------------------------------------------------ 3. convolve against the hand composition
def compose(conv, x):
    plan = conv.plan
    T = x.shape[1]
    L = conv.output_length(T)
    F_out = -(-L // conv.block)
    Y = conv.fdl_mac(plan.stft(x), F_out=F_out)
    return plan.istft_ola(Y)[:, :L]


@pytest.mark.parametrize("pairing", [0, 1])
@pytest.mark.parametrize("B", [128, 256, 512])
def test_convolve_equals_the_hand_composition(pkg, torch_cuda, B, pairing):
    """N = 256 has no pair kernel, N = 512 and 1024 have one.  T and K at every block edge."""
    torch = torch_cuda
    S = 3
    for K in (1, B + 1, 3 * B + 7):
        conv, _ = conv_for(pkg, B, K, 2, seed=K)
        plan = conv.plan
        plan.set_frame_pairing(bool(pairing))
        try:
            for T in (1, B - 1, B + 1, 5 * B + 3):
                x = torch.from_numpy(np.array(streams(S, T, B, seed=T))).cuda()
                want = compose(conv, x)
                got = conv.convolve(x)
                torch.cuda.synchronize()
                assert got.shape == (S, T + K - 1)
                assert same_bits(torch, got, want), (K, T)
                assert "k_fdl_mac" in plan.last_launch()["kernels"]
        finally:
            plan.set_frame_pairing(True)


def test_convolve_chunk_knobs_keep_the_bits(pkg, torch_cuda):
    torch = torch_cuda
    B, K, S, T = 512, 3 * 512 + 7, 3, 40 * 512 + 3
    conv, _ = conv_for(pkg, B, K, 2, seed=K)
    x = torch.from_numpy(np.array(streams(S, T, B))).cuda()
    base = conv.convolve(x)
    torch.cuda.synchronize()
    try:
        for n in (1, 3):
            conv.plan.set_chunks(n)
            conv.set_chunks(n + 1)
            want = compose(conv, x)
            got = conv.convolve(x)
            torch.cuda.synchronize()
            assert same_bits(torch, got, want) and same_bits(torch, got, base), n
    finally:
        conv.plan.set_chunks(0)
        conv.set_chunks(0)


def test_convolve_in_two_slices(pkg, torch_cuda):
    """B = 2048, S = 64, T = 128 B, K = B + 2: F_in = 128, F_out = 130 rows of 4098 floats per
    stream plus the 130 B floats of the uncropped output are 5 294 096 bytes (more where a
    half is staged); 2^28 // 5 294 096 = 50, so at most 50 streams per slice.  Three filters:
    the second slice starts at a stream whose filter is not filter 0."""
    torch = torch_cuda
    B, S = 2048, 64
    T, K = 128 * B, B + 2
    conv, _ = conv_for(pkg, B, K, 3, seed=1)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn((S, T), device="cuda", generator=g) * 0.01
    x[:, 2 * T // 3:] *= 4096.0
    x[:, 3 * B:4 * B] = 0.0
    assert (1 << 28) // (((128 + 130) * (2 * B + 2) + 130 * B) * 4) == 50
    want = compose(conv, x)
    got = conv.convolve(x)
    torch.cuda.synchronize()
    assert same_bits(torch, got, want)
    rec = conv.last_launch()
    nbw = (B + 1 + 63) // 64
    # the last slice's delay line: n_s streams x 33 bin blocks x chunks waves, four per workgroup
    n_s = rec["grid"] * 4 // (nbw * rec["n_chunks"])
    assert 1 <= n_s <= 50 and n_s < S, rec


# ------------------------------------------------------------------ 4. accuracy
@pytest.mark.parametrize("pairing", [0, 1])
@pytest.mark.parametrize("case", CR.ACCURACY_CASES, ids=lambda c: "B%d_T%d_K%d_S%d_nf%d" % c)
def test_convolve_accuracy_against_float64(pkg, oracle, torch_cuda, case, pairing, capsys):
    """Per stream rel-L2 and max-abs over max|y64| against np.convolve in float64; the bar
    per metric is the larger of the project's 1e-6 / 4e-6 and 4x what the float32 CPU
    oracle reaches on the same input and metric.
    Observed on MI355X, ranges over the streams and both pairing settings (device |
    oracle): B = 128, P = 37: rel-L2 1.96e-7 - 2.08e-7 | 1.98e-7 - 2.00e-7, peak 2.17e-7 -
    2.42e-7 | 1.83e-7 - 2.46e-7; B = 512, P = 4: rel-L2 1.82e-7 - 2.00e-7 | 2.00e-7 - 2.12e-7,
    peak 1.65e-7 - 2.38e-7 | 1.74e-7 - 2.49e-7; B = 256, P = 2: rel-L2 1.91e-7 - 1.97e-7 |
    2.05e-7, peak 1.43e-7 - 1.94e-7 | 1.85e-7.  The bars come out as 1e-6 / 4e-6."""
    torch = torch_cuda
    B, T, K, S, nf = case
    x = streams(S, T, B)
    conv, h = conv_for(pkg, B, K, nf)
    y64 = CR.convolve_f64(x, h)
    ofig = CR.error_figures(CR.convolve_oracle_f32(oracle, x, h, B), y64)
    conv.plan.set_frame_pairing(bool(pairing))
    try:
        y = conv.convolve(torch.from_numpy(np.array(x)).cuda())
        torch.cuda.synchronize()
    finally:
        conv.plan.set_frame_pairing(True)
    dfig = CR.error_figures(y.cpu().numpy(), y64)
    with capsys.disabled():
        print("\nconvolve accuracy", case, "pairing", pairing, "device",
              " ".join("(%.2e, %.2e)" % f for f in dfig), "oracle", " ".join("(%.2e, %.2e)" % f for f in ofig))
    for (l2, peak), (ol2, opeak) in zip(dfig, ofig):
        bar_l2, bar_peak = CR.bars(ol2, opeak)
        assert l2 <= bar_l2 and peak <= bar_peak, (l2, peak, bar_l2, bar_peak)


# ------------------------------------------------------------------ 5. exactness and containment
def test_zero_stream_identity_filter_and_untouched_tail(pkg, torch_cuda):
    torch = torch_cuda
    B, S = 256, 3
    T, K = 6 * B + 1, 2 * B + 9
    conv, _ = conv_for(pkg, B, K, 1, seed=4)
    x = np.array(streams(S, T, B, seed=2))
    x[1] = 0.0
    L = T + K - 1
    F_out = -(-L // B)
    assert L < F_out * B
    # rows shorter than F_out * B, a sentinel in and behind them
    y = torch.full((S + 1, L + 5), 123.0, device="cuda")
    conv.convolve(torch.from_numpy(x).cuda(), y=y[:S])
    torch.cuda.synchronize()
    assert int(y[1, :L].view(torch.int32).abs().max()) == 0            # +0, bit for bit
    assert bool(torch.all(y[:S, L:] == 123.0)) and bool(torch.all(y[S] == 123.0))
    assert bool(torch.any(y[0, :L] != 0)) and bool(torch.any(y[2, :L] != 0))
    dense = conv.convolve(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert same_bits(torch, dense, y[:S, :L])
    # h = [1]: y is x within the accuracy bar (x holds no NaN, Inf or tiny value)
    ident = pkg.Convolver(np.ones(1, np.float32), block=B)
    xi = np.array(streams(S, T, B, seed=6))
    yi = ident.convolve(torch.from_numpy(xi).cuda())
    torch.cuda.synchronize()
    assert yi.shape == (S, T)
    bar_l2, bar_peak = CR.bars()
    for l2, peak in CR.error_figures(yi.cpu().numpy(), CR.convolve_f64(xi, [1.0])):
        assert l2 <= bar_l2 and peak <= bar_peak, (l2, peak)
    # 1-d in, 1-d out
    y1 = ident.convolve(torch.from_numpy(xi[0]).cuda())
    torch.cuda.synchronize()
    assert same_bits(torch, y1, yi[0])
    ident.close()


def test_nan_and_inf_samples_are_zeros(pkg, torch_cuda):
    """crlot_stft's forward maps NaN / Inf to 0; the delay line adds no sanitizing."""
    torch = torch_cuda
    B, T, K = 128, 5 * 128 + 3, 128 + 1
    conv, h = conv_for(pkg, B, K, 1, seed=8)
    x = np.array(streams(1, T, B, seed=8))
    x[0, 5], x[0, 300], x[0, 301] = np.nan, np.inf, -np.inf
    y = conv.convolve(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    (l2, peak), = CR.error_figures(y.cpu().numpy(), CR.convolve_f64(x, h))
    assert l2 <= CR.REL_L2 and peak <= CR.MAX_ABS, (l2, peak)


# ------------------------------------------------------------------ 6. errors and empties
def test_errors_and_empties(pkg, torch_cuda):
    torch = torch_cuda
    L_ = pkg.lib()
    B, K = 128, 300
    conv, _ = conv_for(pkg, B, K, 1, seed=7)
    conv.prepare()
    bins, row = B + 1, 2 * B + 2
    buf = torch.zeros(8 * row + 4096, device="cuda")
    p = buf.data_ptr()
    # the output spectra overlap the input spectra
    assert L_.crlot_fdl_mac(conv._h, p, p + 4 * row, 1, 2, 4, 2 * row, row, 4 * row, row, None) == pkg.EINVAL
    assert "overlap" in L_.crlot_last_error().decode()
    assert L_.crlot_fdl_mac(conv._h, p + 4, p + 4 * 4 * row, 1, 2, 4, 2 * row, row, 4 * row, row, None) == pkg.EINVAL
    assert "aligned" in L_.crlot_last_error().decode()
    # x and y overlap; rows of y too short
    assert L_.crlot_convolve(conv._h, p, p + 4 * 100, 1, 500, 500, 0, None) == pkg.EINVAL
    assert "overlap" in L_.crlot_last_error().decode()
    assert L_.crlot_convolve(conv._h, p, p + 4 * 4096, 2, 500, 500, 798, None) == pkg.EINVAL
    assert L_.crlot_convolve(conv._h, p, p + 4 * 4096, 2, 500, 499, 799, None) == pkg.EINVAL
    spec = torch.zeros((2, 4, bins), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):
        conv.fdl_mac(spec, out=spec, F_out=4)
    x = torch.zeros((2, 500), device="cuda")
    with pytest.raises(ValueError):
        conv.convolve(x, y=torch.zeros((2, 798), device="cuda"))
    with pytest.raises(ValueError):
        conv.convolve(x.double())
    # empties: nothing written
    assert conv.convolve(torch.zeros((0, 500), device="cuda")).shape == (0, 799)
    assert conv.convolve(torch.zeros((2, 0), device="cuda")).shape == (2, 0)
    assert conv.fdl_mac(torch.zeros((0, 4, bins), dtype=torch.complex64, device="cuda")).shape == (0, 6, bins)
    # the borrowed plan outlives a close of its view, and the convolver still works
    plan = conv.plan
    assert (plan.frame_size, plan.hop_size, plan.frame_count(3 * B + 1)) == (2 * B, B, 4)
    plan.close()
    conv._plan = None
    y = conv.convolve(torch.ones((1, 10), device="cuda"))
    torch.cuda.synchronize()
    assert y.shape == (1, 10 + K - 1) and bool(torch.isfinite(y).all())
