"""GPU tests of the adaptive filter (include/crlot_dsp.h, "adaptive filter"): after every
hop the downloaded state equals the contract step by step, bit for bit (the reference
spectrum and the error spectrum against the offline entries, the output against the
chain and the offline inverse, the power estimate, the gradient and every weight row
against the float32 model applied to the device's own previous state); the gradient
constraint zeroes the upper half of every partition within the bar a float32
kiss_fftr round trip sets and modes 1 and 2 equal explicit constraint calls; the filter
identifies a system to -100 dB with the constraint and not without; e tracks the
float64 model under the bar the float32 CPU model sets; a frozen filter is the
convolution; the bits do not depend on the channel count, a channel's position, the
layout, reset, or a NULL reference block; sentinels and launch records.

Shapes: every E instantiation (B = 128, 256, 512, 1024), P = 1, 2, 3, 5; channels 1, 3, 5, 9
(a partial workgroup, a second and a third one).
"""
import numpy as np
import pytest

import convolve_reference as CR
import fdaf_reference as FR
import stream_convolve_reference as SR

pytestmark = pytest.mark.gpu

SHAPES = [(128, 1), (128, 2), (128, 3), (128, 5), (256, 4), (512, 3), (1024, 2)]
CONV_SHAPES = [(128, 3), (128, 5), (256, 4), (512, 3)]


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def np_bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def cplx(t):
    """A state view (.., 2 bins) of (re, im) floats -> complex64 on the host."""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.complex64)


def cbits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.int32)


_plans = {}


def plan_for(pkg, B):
    """The offline plan of step 2: frame 2B, hop B, a window of ones, frame pairing off."""
    if B not in _plans:
        _plans[B] = pkg.Plan(frame_size=2 * B, hop_size=B, window_type=pkg.RECT, window_norm=pkg.NORM_NONE,
                             boundary_mode=pkg.ZERO_PAD, analysis_window=True, apply_window_inside=False,
                             frame_pairing=False)
    return _plans[B]


def blocks_of(torch, a, B):
    """(C, hops B) host array -> a list of contiguous (C, B) device blocks."""
    t = torch.from_numpy(np.array(a, np.float32)).cuda()
    C = t.shape[0]
    return list(t.view(C, -1, B).permute(1, 0, 2).contiguous())


def run_device(torch, af, x, d, want_y=False):
    """Push x (or None) and d, (C, hops B) host arrays; returns e (and y) as host arrays (C, hops B)."""
    B = af.block
    db = blocks_of(torch, d, B)
    xb = blocks_of(torch, x, B) if x is not None else [None] * len(db)
    es, ys = [], []
    for xj, dj in zip(xb, db):
        if af.interleaved:
            xj, dj = (None if xj is None else xj.t().contiguous()), dj.t().contiguous()
        y = torch.empty_like(dj) if want_y else None
        e = af.push(xj, dj, y=y)
        es.append(e.t() if af.interleaved else e)
        if want_y:
            ys.append(y.t() if af.interleaved else y)
    torch.cuda.synchronize()
    e = torch.cat(es, dim=1).cpu().numpy()
    return (e, torch.cat(ys, dim=1).cpu().numpy()) if want_y else e


_cases = {}


def case(B, P, hops, channels, seed):
    key = (B, P, hops, channels, seed)
    if key not in _cases:
        x, h, d = FR.make_case(B, P, hops, seed, channels)
        for a in (x, h, d):
            a.setflags(write=False)
        _cases[key] = (x, h, d)
    return _cases[key]


# ------------------------------------------------------------------ 1. every step, bit for bit
@pytest.mark.parametrize("B,P", SHAPES)
def test_every_hop_equals_the_contract_bit_for_bit(pkg, torch_cuda, B, P):
    """2P + 3 hops (the ring wraps twice), mode 0, the weights started from noise so that
    every row is its own sentinel.  One case carries a NaN, an Inf and a 1e-38 sample."""
    torch = torch_cuda
    plan = plan_for(pkg, B)
    hops, K = 2 * P + 3, P * B - 5
    cst = FR.constants(1.0, 0.9, 1e-3, P)
    for C in (1, 3, 5, 9):
        x, _, d = (np.array(a) for a in case(B, P, hops, C, seed=B + P))
        d = d.astype(np.float32)
        if C == 3:
            x[0, 5], x[1, B + 2], x[2, 3 * B + 9] = np.nan, np.inf, np.float32(1e-38)
            d[2, 7], d[0, 2 * B + 1] = np.inf, np.nan
        af = pkg.AdaptiveFilter(B, K, C)
        af.set_step(1.0, 0.9, 1e-3)
        af.set_constraint(0)
        assert af.state_bytes == 4 * C * (2 * P * (2 * B + 2) + 2 * (2 * B + 2) + B + B + 1)
        st = af.state()
        rng = np.random.default_rng(C)
        st["W"].copy_(torch.from_numpy((rng.standard_normal(tuple(st["W"].shape)) * 0.05).astype(np.float32)))
        # step 2 offline: crlot_stft with pairing off over the reference prefixed by B zeros
        xpad = torch.zeros((C, (hops + 1) * B), device="cuda")
        xpad[:, B:] = torch.from_numpy(x).cuda()
        S = plan.stft(xpad)
        torch.cuda.synchronize()
        xb, db = blocks_of(torch, x, B), blocks_of(torch, d, B)
        for k in range(hops):
            W_prev, pw_prev = cplx(st["W"]), st["pw"].cpu().numpy()
            y = torch.empty_like(db[k])
            e = af.push(xb[k], db[k], y=y)
            torch.cuda.synchronize()
            ring, W, E, G = cplx(st["ring"]), cplx(st["W"]), cplx(st["E"]), cplx(st["G"])
            pw = st["pw"].cpu().numpy()
            where = (C, k)
            # 2: the ring row is the offline spectrum; prev is the sanitized block
            assert same_bits(torch, torch.view_as_real(S[:, k]).reshape(C, -1), st["ring"][:, k % P]), where
            assert np.array_equal(np_bits(st["prev"].cpu().numpy()), np_bits(CR.sanitize(x[:, k * B:(k + 1) * B]))), where
            # 3, 4: y is the offline inverse of the chain over the previous weights; e = d - y
            Y = torch.from_numpy(FR.chain(W_prev, ring, k)).cuda()
            o = plan.irfft(Y)
            assert same_bits(torch, o[:, B:], y), where
            dbk = CR.sanitize(d[:, k * B:(k + 1) * B])
            assert np.array_equal(np_bits(e.cpu().numpy()), np_bits(dbk - y.cpu().numpy())), where
            # 5: E is the offline spectrum of [+0, e]
            fr = torch.zeros((C, 2 * B), device="cuda")
            fr[:, B:] = e
            assert same_bits(torch, torch.view_as_real(plan.rfft(fr)).reshape(C, -1), st["E"]), where
            # 6: pw and G from the device's own X_k, E and previous pw
            pw_want = FR.power(pw_prev, ring[:, k % P], k, cst)
            assert np.array_equal(np_bits(pw), np_bits(pw_want)), where
            assert np.array_equal(cbits(G), cbits(FR.gradient(pw, E, cst))), where
            # 7: every W row from the previous W, the ring and G; rows p > k untouched
            assert np.array_equal(cbits(W), cbits(FR.update(W_prev, ring, G, k))), where
            if k < P - 1:
                assert np.array_equal(cbits(W[:, k + 1:]), cbits(W_prev[:, k + 1:])), where
        rec = af.last_launch()
        assert rec["kernels"] == [49, 50] and rec["names"] == ["k_fdaf_hop", "k_fdaf_update"], rec
        assert rec["hop_grid"] == -(-C // 4) and rec["update_grid"] == C * -(-(B + 1) // 64) and rec["constrain_grid"] == 0
        assert af.hops == hops
        af.close()


# ------------------------------------------------------------------ 2. the gradient constraint
def _halves(W, w_ref=None):
    """Float64 inverse of rows (.., bins): (max |upper half|, max |lower half - reference's|) over
    max |w| of the reference rows, and the inverses."""
    w = np.fft.irfft(W.astype(np.complex128), axis=-1)
    B = w.shape[-1] // 2
    ref = w if w_ref is None else w_ref
    scale = np.max(np.abs(ref))
    return np.max(np.abs(w[..., B:])) / scale, np.max(np.abs(w[..., :B] - ref[..., :B])) / scale, w


@pytest.mark.parametrize("B,P", CONV_SHAPES + [(1024, 2)])
def test_constraint_zeroes_the_upper_halves(pkg, oracle, torch_cuda, B, P, capsys):
    """P + 2 unconstrained adapting hops leave wrap-around in the upper halves; constrain(-1)
    removes it.  The bar is 4x what the oracle's float32 kiss_fftr inverse -> zero ->
    forward reaches on the same rows, per metric."""
    torch = torch_cuda
    C, hops = 3, P + 2
    x, _, d = case(B, P, hops, C, seed=7 * B + P)
    af = pkg.AdaptiveFilter(B, P * B - 5, C)
    af.set_step(1.0, 0.9, 1e-3)
    af.set_constraint(0)
    run_device(torch, af, x, d)
    st = af.state()
    W0 = cplx(st["W"])
    up0, _, w0 = _halves(W0)
    # the CPU round trip of the same rows
    pair = SR.KissPair(oracle, B)
    W_cpu = np.zeros_like(W0)
    for c in range(C):
        for p in range(P):
            w = np.array(pair.inv(W0[c, p]))
            w[B:] = 0
            W_cpu[c, p] = pair.fwd(w)
    up_cpu, lo_cpu, _ = _halves(W_cpu, w0)
    af.constrain(-1)
    torch.cuda.synchronize()
    up, lo, _ = _halves(cplx(st["W"]), w0)
    with capsys.disabled():
        print(f"\nfdaf constraint B {B} P {P}: upper before {up0:.2e}; after: device {up:.2e} oracle {up_cpu:.2e};"
              f" lower change: device {lo:.2e} oracle {lo_cpu:.2e}")
    assert up0 > 1e3 * max(4 * up_cpu, 1e-7), up0   # the test has teeth
    assert up <= 4 * up_cpu, (up, up_cpu)
    assert lo <= 4 * lo_cpu, (lo, lo_cpu)
    af.close()


@pytest.mark.parametrize("B,P", [(128, 1), (128, 3), (128, 5), (256, 4), (512, 3), (1024, 2)])
def test_modes_equal_explicit_constraint_calls(pkg, torch_cuda, B, P):
    torch = torch_cuda
    C, hops = 5, 2 * P + 3
    x, _, d = case(B, P, hops, C, seed=11 * B + P)
    xb, db = blocks_of(torch, x, B), blocks_of(torch, d, B)
    for mode in (1, 2):
        a, b = pkg.AdaptiveFilter(B, P * B - 5, C), pkg.AdaptiveFilter(B, P * B - 5, C)
        for af, m in ((a, mode), (b, 0)):
            af.set_step(1.0, 0.9, 1e-3)
            af.set_constraint(m)
        for k in range(hops):
            ea = a.push(xb[k], db[k])
            eb = b.push(xb[k], db[k])
            b.constrain(k % P if mode == 1 else -1)
            assert same_bits(torch, ea, eb), (mode, k)
        torch.cuda.synchronize()
        assert same_bits(torch, a.state()["W"], b.state()["W"]), mode
        rec = a.last_launch()
        assert rec["kernels"] == [49, 50, 51] and rec["names"][2] == "k_fdaf_constrain"
        assert rec["constrain_grid"] == -(-(C * (1 if mode == 1 else P)) // 4)
        a.close()
        b.close()


# ------------------------------------------------------------------ 3. convergence
@pytest.mark.parametrize("B,P", CONV_SHAPES)
def test_identifies_the_system(pkg, torch_cuda, B, P, capsys):
    """The reference test's inputs, 200 hops, 3 channels with different h, mu = 1: -100 dB in
    modes 1 and 2 (the float32 CPU model reaches -130 dB); at (128, 3) mode 1 ends at
    least 60 dB below mode 0."""
    torch = torch_cuda
    C = 3
    x, h, d = case(B, P, 200, C, seed=1000 * B + P)
    got = {}
    for mode in (1, 2, 0) if (B, P) == (128, 3) else (1, 2):
        af = pkg.AdaptiveFilter(B, P * B - 5, C)
        af.set_step(1.0, 0.9, 1e-3)
        af.set_constraint(mode)
        run_device(torch, af, x, d)
        taps = af.taps()
        got[mode] = [FR.misalignment_db(taps[c], h[c]) for c in range(C)]
        af.close()
    with capsys.disabled():
        print(f"\nfdaf misalignment B {B} P {P}:", {m: [round(v, 1) for v in vs] for m, vs in got.items()})
    for mode in (1, 2):
        assert max(got[mode]) <= -100.0, (mode, got[mode])
    if 0 in got:
        assert max(got[1]) <= min(got[0]) - 60.0, got


# ------------------------------------------------------------------ 4. tracking, 5. the frozen filter
def _bars(device, cpu):
    """Per metric: the larger of the project's bar and 4x the float32 CPU model's figure."""
    return [(max(CR.REL_L2, 4 * c[0]), max(CR.MAX_ABS, 4 * c[1])) for c in cpu]


def _figures(a, ref, scale):
    """Per channel (rel-L2 against ref, peak error over max |scale|)."""
    a, ref, scale = (np.asarray(v, np.float64) for v in (a, ref, scale))
    return [(float(np.linalg.norm(a[c] - ref[c]) / np.linalg.norm(ref[c])),
             float(np.max(np.abs(a[c] - ref[c])) / np.max(np.abs(scale[c])))) for c in range(len(a))]


@pytest.mark.parametrize("B,P", [(128, 3), (256, 4), (512, 3)])
@pytest.mark.parametrize("mode", [0, 1])
def test_error_tracks_the_float64_model(pkg, oracle, torch_cuda, B, P, mode, capsys):
    """60 hops, d plus noise of sigma 0.01: e against the float64 model, per channel."""
    torch = torch_cuda
    C, hops = 3, 60
    x, _, d = case(B, P, hops, C, seed=13 * B + P)
    d = (d + 0.01 * np.random.default_rng(B + P).standard_normal(d.shape)).astype(np.float32)
    m64 = FR.F64Model(B, P * B - 5, C, mu=1.0, lam=0.9, delta=1e-3, mode=mode)
    e64, _ = FR.run(m64, x, d)
    pair = SR.KissPair(oracle, B)
    m32 = FR.F32Model(B, P * B - 5, C, mu=1.0, lam=0.9, delta=1e-3, mode=mode, fwd=pair.fwd, inv=pair.inv)
    e32, _ = FR.run(m32, x, d)
    af = pkg.AdaptiveFilter(B, P * B - 5, C)
    af.set_step(1.0, 0.9, 1e-3)
    af.set_constraint(mode)
    e = run_device(torch, af, x, d)
    af.close()
    dev, cpu = _figures(e, e64, d), _figures(e32, e64, d)
    with capsys.disabled():
        print(f"\nfdaf tracking B {B} P {P} mode {mode}: device", " ".join("(%.2e, %.2e)" % f for f in dev),
              "float32 model", " ".join("(%.2e, %.2e)" % f for f in cpu))
    for (l2, peak), (bar_l2, bar_peak) in zip(dev, _bars(dev, cpu)):
        assert l2 <= bar_l2 and peak <= bar_peak, (dev, cpu)


@pytest.mark.parametrize("B,P", [(128, 1), (128, 5), (256, 4), (512, 3)])
def test_frozen_filter_is_the_convolution(pkg, oracle, torch_cuda, B, P, capsys):
    torch = torch_cuda
    C, hops = 3, 2 * P + 3
    x, h, d = case(B, P, hops, C, seed=17 * B + P)
    h32 = h.astype(np.float32)
    y64 = CR.convolve_f64(x, h32)[:, :hops * B]
    pair = SR.KissPair(oracle, B)
    m32 = FR.F32Model(B, P * B - 5, C, adapt=False, fwd=pair.fwd, inv=pair.inv)
    m32.set_taps(h32)
    _, y32 = FR.run(m32, x, d)
    af = pkg.AdaptiveFilter(B, P * B - 5, C)
    af.set_adapt(False)
    af.set_taps(h32)
    W0 = af.state()["W"].clone()
    # taps -> spectra -> taps: one float32 transform pair, under the project's peak bar
    assert np.max(np.abs(af.taps().astype(np.float64) - h32)) <= CR.MAX_ABS * np.max(np.abs(h32))
    e, y = run_device(torch, af, x, d, want_y=True)
    assert same_bits(torch, W0, af.state()["W"])
    assert af.last_launch()["kernels"] == [49]
    assert np.array_equal(np_bits(e), np_bits(CR.sanitize(d.astype(np.float32)) - y))
    dev, cpu = _figures(y, y64, y64), _figures(y32, y64, y64)
    with capsys.disabled():
        print(f"\nfdaf frozen B {B} P {P}: device", " ".join("(%.2e, %.2e)" % f for f in dev),
              "float32 model", " ".join("(%.2e, %.2e)" % f for f in cpu))
    for (l2, peak), (bar_l2, bar_peak) in zip(dev, _bars(dev, cpu)):
        assert l2 <= bar_l2 and peak <= bar_peak, (dev, cpu)
    af.close()


# ------------------------------------------------------------------ 6. invariance, bit for bit
@pytest.mark.parametrize("B,P", [(128, 3), (512, 3)])
def test_bits_do_not_depend_on_batch_layout_reset_or_null_blocks(pkg, torch_cuda, B, P):
    torch = torch_cuda
    C, hops, K = 5, 2 * P + 3, P * B - 5
    x, h, d = (np.array(a) for a in case(B, P, hops, C, seed=19 * B + P))
    x[:, 2 * B:3 * B] = 0.0     # hop 2 is pushed as a NULL block below

    def make(channels, interleaved=False, mode=1):
        af = pkg.AdaptiveFilter(B, K, channels, interleaved=interleaved)
        af.set_step(1.0, 0.9, 1e-3)
        af.set_constraint(mode)
        return af

    af = make(C)
    e, y = run_device(torch, af, x, d, want_y=True)
    W = af.state()["W"].clone()
    assert np.any(y != 0) and np.any(W.cpu().numpy() != 0)
    # reset, then the same run
    af.reset()
    assert af.hops == 0 and not bool(torch.any(af.state()["W"] != 0))
    e2, y2 = run_device(torch, af, x, d, want_y=True)
    assert np.array_equal(np_bits(e), np_bits(e2)) and np.array_equal(np_bits(y), np_bits(y2))
    assert same_bits(torch, W, af.state()["W"])
    af.close()
    # each channel alone (another grid for every kernel), in modes 1 and 2
    for mode in (1, 2):
        full = make(C, mode=mode)
        ef = run_device(torch, full, x, d)
        for c in (0, C - 1) if mode == 2 else range(C):
            one = make(1, mode=mode)
            ec = run_device(torch, one, x[c:c + 1], d[c:c + 1])
            assert np.array_equal(np_bits(ec), np_bits(ef[c:c + 1])), (mode, c)
            assert same_bits(torch, one.state()["W"], full.state()["W"][c:c + 1]), (mode, c)
            one.close()
        full.close()
    # the interleaved layout
    il = make(C, interleaved=True)
    ei, yi = run_device(torch, il, x, d, want_y=True)
    assert np.array_equal(np_bits(e), np_bits(ei)) and np.array_equal(np_bits(y), np_bits(yi))
    assert same_bits(torch, W, il.state()["W"])
    il.close()
    # a NULL reference block is a block of zeros
    nb = make(C)
    db = blocks_of(torch, d, B)
    xb = blocks_of(torch, x, B)
    en = torch.cat([nb.push(None if k == 2 else xb[k], db[k]) for k in range(hops)], dim=1)
    torch.cuda.synchronize()
    assert np.array_equal(np_bits(e), np_bits(en.cpu().numpy()))
    assert same_bits(torch, W, nb.state()["W"])
    nb.close()
    # one row of taps for every channel equals replicated rows
    a, b = make(C), make(C)
    for f in (a, b):
        f.set_adapt(False)
    a.set_taps(h[0].astype(np.float32))
    b.set_taps(np.repeat(h[0:1].astype(np.float32), C, axis=0))
    assert same_bits(torch, a.state()["W"], b.state()["W"])
    assert np.array_equal(np_bits(run_device(torch, a, x, d)), np_bits(run_device(torch, b, x, d)))
    a.close()
    b.close()


def test_outputs_stay_inside_their_blocks(pkg, torch_cuda):
    """Sentinels around e and y, both layouts, a partial and a second workgroup."""
    torch = torch_cuda
    B, P, C = 128, 2, 5
    x, _, d = case(B, P, 3, C, seed=23)
    for interleaved in (False, True):
        af = pkg.AdaptiveFilter(B, P * B - 5, C, interleaved=interleaved)
        n = C * B
        pad = 4 * B
        bufs = {name: torch.full((n + 2 * pad,), 777.0, device="cuda") for name in ("e", "y")}
        shape = (B, C) if interleaved else (C, B)
        views = {name: t[pad:pad + n].view(shape) for name, t in bufs.items()}
        xb, db = blocks_of(torch, x, B), blocks_of(torch, d, B)
        for k in range(3):
            xk, dk = (xb[k].t().contiguous(), db[k].t().contiguous()) if interleaved else (xb[k], db[k])
            af.push(xk, dk, e=views["e"], y=views["y"])
        torch.cuda.synchronize()
        for name, t in bufs.items():
            assert bool(torch.all(t[:pad] == 777.0)) and bool(torch.all(t[pad + n:] == 777.0)), (name, interleaved)
            assert not bool(torch.any(t[pad:pad + n] == 777.0)), (name, interleaved)
        rec = af.last_launch()
        assert rec["kernels"] == [49, 50, 51] and rec["hop_grid"] == 2 and rec["update_grid"] == C * 3
        assert rec["constrain_grid"] == 2
        af.set_adapt(False)
        af.push(xb[0].t().contiguous() if interleaved else xb[0], db[0].t().contiguous() if interleaved else db[0])
        assert af.last_launch()["kernels"] == [49]
        af.close()
