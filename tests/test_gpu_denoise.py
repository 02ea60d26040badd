"""GPU tests of the noise suppressor (include/crlot_dsp.h, "noise suppressor").

Bit for bit: crlot_denoise_gains on the device's own crlot_stft rows equals the float32
numpy restatement of the contract (tests/denoise_reference.py) in gains and final state;
a run cut at every frame and carried equals the uncut run; crlot_denoise equals the hand
composition with frame pairing on and off; the streaming hops concatenated equal
crlot_denoise (pairing off, DROP) on the fused and the staged route, the two routes
agree, and after every hop the object's state equals the model's; the bits do not depend
on the batch, the PCM layout, a reset or a plan gain, and g_min = 1 is push_hop.
Accuracy: the gains against the float64 model on numpy's FFT (a threshold compare may
flip on a rounding difference in X: at most 1e-3 of the (frame, bin) pairs may differ by
more than 1e-3), y against the float64 chain.  Behaviour: the noise removed in the gaps
and the SNR gain in the bursts within 0.5 dB of the float64 model's.

Shapes: 256/128 (E = 2), 512/128 (E = 4), 512/256 (S = 2), 1024/256 (E = 8), 2048/512
(staged), 960/240 (mixed radix, staged); channels 1, 3, 5, 9; L = 8 and 3 L + 2 frames.
One channel carries a NaN, an Inf and a 1e-38 sample, one is all zeros.
"""
import ctypes

import numpy as np
import pytest

import denoise_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(256, 128), (512, 128), (512, 256), (1024, 256), (2048, 512), (960, 240)]
FUSED = {(256, 128), (512, 128), (512, 256), (1024, 256)}
L = 8
F = 3 * L + 2
CHANNELS = (1, 3, 5, 9)
K_GAINS, K_HOP, K_STFT, K_ISTFT = 53, 54, 55, 56


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_inputs, _plans = {}, {}


def signal(N, H, C, frames=F):
    """(C, T) float32: bursts plus noise per channel (its own seed); with three channels or
    more channel 1 carries a NaN, an Inf and a 1e-38 sample and channel 2 is all zeros."""
    key = (N, H, C, frames)
    if key not in _inputs:
        rows = []
        for c in range(C):
            s, v, _ = R.bursts(N, H, frames, seed=7 + c)
            rows.append((s + v).astype(np.float32))
        x = np.stack(rows)
        if C >= 3:
            x[1, 5], x[1, N + 3], x[1, 2 * N + 1] = np.nan, np.inf, np.float32(1e-38)
            x[2] = 0.0
        x.setflags(write=False)
        _inputs[key] = x
    return _inputs[key]


def plan_of(pkg, N, H):
    if (N, H) not in _plans:
        _plans[(N, H)] = pkg.Plan(frame_size=N, hop_size=H, boundary_mode=pkg.DROP, frame_pairing=False)
    p = _plans[(N, H)]
    p.set_frame_pairing(False)
    return p


def device_spectra(torch, plan, x):
    S = plan.stft(torch.from_numpy(np.array(x)).cuda())
    torch.cuda.synchronize()
    return S


def model(S, **params):
    """The float32 restatement on device spectra (C, F, bins) complex64 -> gains, state."""
    return R.gains(R.power(S.cpu().numpy(), np.float32), np.float32, window=L, **params)


def run_stream(pkg, torch, plan, dn, x, interleaved=False, after_hop=None):
    """Push x (C, T) hop by hop through Stream.denoise_hop; returns y (C, F H)."""
    C, T = x.shape
    H = plan.hop_size
    st = pkg.Stream(plan, C, interleaved=interleaved)
    xd = torch.from_numpy(np.array(x)).cuda()
    outs = []
    for q in range(T // H):
        hop = xd[:, q * H:(q + 1) * H]
        hop = hop.t().contiguous() if interleaved else hop.contiguous()
        out, em = st.denoise_hop(dn, hop)
        assert em == (H if q >= plan.frame_size // H - 1 else 0), q
        if em:
            outs.append(out.t() if interleaved else out)
        if after_hop:
            after_hop(q, em)
    torch.cuda.synchronize()
    st.close()
    return torch.cat(outs, dim=1).cpu().numpy()


# ------------------------------------------------------------------ 1. the offline gains
@pytest.mark.parametrize("N,H", SHAPES)
def test_gains_equal_the_float32_restatement(pkg, torch_cuda, N, H):
    """Gains and final state, every channel count, padded mask rows with sentinels."""
    torch = torch_cuda
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    for C in CHANNELS:
        S = device_spectra(torch, plan, signal(N, H, C))
        assert S.shape == (C, F, bins)
        G, st = model(S)
        if C >= 3:
            assert np.all(G[2] == np.float32(0.1)) and np.isfinite(G).all()
        dn = pkg.Denoiser(plan, C, window=L)
        buf = torch.full((C, F + 1, bins + 3), -7.0, device="cuda")
        mask = buf[:, :F, :bins]
        dn.gains(S, mask=mask, carry=True)
        torch.cuda.synchronize()
        assert same(mask.cpu().numpy(), G), C
        assert torch.all(buf[:, F:] == -7.0) and torch.all(buf[:, :, bins:] == -7.0)
        assert same(dn.state().cpu().numpy(), st), C
        assert dn.frames == F
        rec = dn.last_launch()
        assert rec["kernels"] == [K_GAINS] and rec["grids"] == [C * ((bins + 63) // 64)] and rec["route"] == 0
        # carry = 0 leaves the object alone and takes any stream count
        dn2 = pkg.Denoiser(plan, C + 1, window=L)
        assert same(dn2.gains(S).cpu().numpy(), G) and dn2.frames == 0
        assert torch.all(dn2.state() == 0)
        with pytest.raises(ValueError):
            dn2.gains(S, carry=True)
        dn.close(), dn2.close()


@pytest.mark.parametrize("N,H", [(256, 128), (960, 240)])
def test_gains_cut_and_carried_equal_the_uncut_run(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, C = plan_of(pkg, N, H), 3
    S = device_spectra(torch, plan, signal(N, H, C))
    dn = pkg.Denoiser(plan, C, window=L)
    whole = dn.gains(S, carry=True).cpu().numpy()
    state = dn.state().cpu().numpy()
    assert same(whole, model(S)[0])
    for F1 in range(1, F):
        dn.reset()
        a = dn.gains(S[:, :F1], carry=True)
        assert dn.frames == F1
        b = dn.gains(S[:, F1:], carry=True)
        torch.cuda.synchronize()
        assert same(torch.cat([a, b], dim=1).cpu().numpy(), whole), F1
        assert same(dn.state().cpu().numpy(), state), F1
    dn.close()


# ------------------------------------------------------------------ 2. the offline composite
@pytest.mark.parametrize("N,H", SHAPES)
@pytest.mark.parametrize("pairing", [False, True])
def test_denoise_equals_the_hand_composition(pkg, torch_cuda, N, H, pairing):
    torch = torch_cuda
    plan, C = plan_of(pkg, N, H), 5
    plan.set_frame_pairing(pairing)
    x = torch.from_numpy(np.array(signal(N, H, C))).cuda()
    dn = pkg.Denoiser(plan, C, window=L)
    S = plan.stft(x)
    G = dn.gains(S)
    plan.set_spectral_mask(G)
    want = plan.istft_ola(S)
    plan.set_spectral_mask(None)
    buf = torch.full((C + 1, F * H + 5), -7.0, device="cuda")
    y = dn.denoise(x, y=buf[:C, :F * H])
    torch.cuda.synchronize()
    assert same(y.cpu().numpy(), want.cpu().numpy())
    assert torch.all(buf[C:] == -7.0) and torch.all(buf[:, F * H:] == -7.0)
    assert dn.frames == 0 and "k_denoise_gains" in plan.last_launch()["kernels"]
    plan.set_spectral_mask(G)
    with pytest.raises(ValueError):
        dn.denoise(x)
    plan.set_spectral_mask(None)
    plan.set_frame_pairing(False)
    dn.close()


# ------------------------------------------------------------------ 3. the hops
@pytest.mark.parametrize("N,H", SHAPES)
def test_hops_equal_denoise_on_both_routes_and_the_state_follows_the_model(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins, NB = plan_of(pkg, N, H), N // 2 + 1, -(-N // H)
    fused = (N, H) in FUSED
    for C in CHANNELS:
        x = signal(N, H, C)
        dn = pkg.Denoiser(plan, C, window=L)
        assert dn.fused_ok == fused
        want = dn.denoise(torch.from_numpy(np.array(x)).cuda()).cpu().numpy()
        S = device_spectra(torch, plan, x)
        P = R.power(S.cpu().numpy(), np.float32)
        got = {}
        for route in ((1, 2) if fused else (2,)):
            dn.reset()
            dn.set_route(route)
            track = {"state": None}

            def after_hop(q, em, track=track, route=route):
                rec = dn.last_launch()
                k = q - (NB - 1)
                if route == 1:
                    assert rec == {"route": 1, "kernels": [K_HOP], "names": ["k_stream_denoise"],
                                   "grids": [(C + 3) // 4]}, rec
                else:
                    assert rec["route"] == 2 and rec["kernels"] == ([K_STFT, K_GAINS, K_ISTFT] if em else [K_STFT])
                    if em:
                        assert rec["grids"][1] == C * ((bins + 63) // 64)
                        if fused or N == 2048:
                            assert rec["grids"][0] == rec["grids"][2] == (C + 3) // 4
                if not em:
                    assert dn.frames == 0 and torch.all(dn.state() == 0), q
                    return
                _, track["state"] = R.gains(P[:, k:k + 1], np.float32, state=track["state"], k0=k, window=L)
                assert dn.frames == k + 1
                assert same(dn.state().cpu().numpy(), track["state"]), (C, route, k)

            got[route] = run_stream(pkg, torch, plan, dn, x, after_hop=after_hop)
            assert same(got[route], want), (C, route)
        if fused:
            assert same(got[1], got[2]), C
        else:
            with pytest.raises(NotImplementedError):
                dn.set_route(1)
        dn.set_route(0)
        dn.reset()
        run_stream(pkg, torch, plan, dn, x[:, :N])
        assert dn.last_launch()["route"] == (1 if fused else 2)
        dn.close()


@pytest.mark.parametrize("N,H", [(512, 128), (1024, 256), (2048, 512), (960, 240)])
def test_hop_invariances(pkg, torch_cuda, N, H):
    """Each channel alone, the interleaved layout, reset then the same run, a plan gain, and
    g_min = 1 against push_hop."""
    torch = torch_cuda
    plan, C = plan_of(pkg, N, H), 5
    x = signal(N, H, C)
    dn = pkg.Denoiser(plan, C, window=L)
    base = run_stream(pkg, torch, plan, dn, x)
    state = dn.state().cpu().numpy()
    # reset, then the same run, through sentinel-framed hop buffers
    dn.reset()
    assert torch.all(dn.state() == 0) and dn.frames == 0
    st = pkg.Stream(plan, C)
    xd = torch.from_numpy(np.array(x)).cuda()
    buf = torch.full((C + 2, H), -7.0, device="cuda")
    outs = []
    for q in range(x.shape[1] // H):
        _, em = st.denoise_hop(dn, xd[:, q * H:(q + 1) * H].contiguous(), out=buf[1:C + 1])
        if em:
            outs.append(buf[1:C + 1].clone())
        assert torch.all(buf[0] == -7.0) and torch.all(buf[C + 1] == -7.0)
    torch.cuda.synchronize()
    assert same(torch.cat(outs, dim=1).cpu().numpy(), base) and same(dn.state().cpu().numpy(), state)
    st.close()
    # the interleaved PCM layout
    dn.reset()
    assert same(run_stream(pkg, torch, plan, dn, x, interleaved=True), base)
    assert same(dn.state().cpu().numpy(), state)
    dn.close()
    # each channel alone
    for c in range(C):
        d1 = pkg.Denoiser(plan, 1, window=L)
        assert same(run_stream(pkg, torch, plan, d1, x[c:c + 1]), base[c:c + 1]), c
        assert same(d1.state().cpu().numpy(), state[c:c + 1]), c
        d1.close()
    # g_min = 1: G = 1 everywhere, the plain hop's bits
    d1 = pkg.Denoiser(plan, C, window=L, g_min=1.0)
    got = run_stream(pkg, torch, plan, d1, x)
    st = pkg.Stream(plan, C)
    outs = []
    for q in range(x.shape[1] // H):
        out, em = st.push_hop(xd[:, q * H:(q + 1) * H].contiguous())
        if em:
            outs.append(out)
    torch.cuda.synchronize()
    assert same(got, torch.cat(outs, dim=1).cpu().numpy())
    st.close(), d1.close()
    # a plan gain: the gains come from X before it, the step is (X gain) G
    gain = (0.5 + np.arange(N // 2 + 1) / N).astype(np.float32)
    plan.set_spectral_gain(gain)
    try:
        d1 = pkg.Denoiser(plan, C, window=L)
        want = d1.denoise(xd).cpu().numpy()
        routes = (1, 2) if (N, H) in FUSED else (2,)
        for route in routes:
            d1.reset()
            d1.set_route(route)
            assert same(run_stream(pkg, torch, plan, d1, x), want), route
            assert same(d1.state().cpu().numpy(), state), route
        assert not same(want, base)
        d1.close()
    finally:
        plan.set_spectral_gain(None)
        torch.cuda.synchronize()


def test_hop_argument_checks(pkg, torch_cuda):
    torch = torch_cuda
    plan, other = plan_of(pkg, 256, 128), plan_of(pkg, 512, 128)
    H = 128
    dn, st = pkg.Denoiser(plan, 2, window=L), pkg.Stream(plan, 2)
    hop = torch.zeros((2, H), device="cuda")
    with pytest.raises(ValueError):
        st.denoise_hop(pkg.Denoiser(other, 2), hop)
    with pytest.raises(ValueError):
        st.denoise_hop(pkg.Denoiser(plan, 3), hop)
    lib, em = pkg.lib(), ctypes.c_int32()
    d_other, d3 = pkg.Denoiser(other, 2), pkg.Denoiser(plan, 3)
    for bad in (d_other, d3):  # the C entry's own checks
        assert lib.crlot_stream_denoise_hop(st._h, bad._h, hop.data_ptr(), hop.data_ptr(), em, None) == pkg.EINVAL
    # counters: two hops complete frame 0; a suppressor that has not seen it is refused from then on
    st.denoise_hop(dn, hop)
    st.denoise_hop(dn, hop)
    assert dn.frames == 1
    fresh = pkg.Denoiser(plan, 2, window=L)
    with pytest.raises(RuntimeError):
        st.denoise_hop(fresh, hop)
    st.push_hop(hop)  # the stream moves on without the suppressor
    with pytest.raises(RuntimeError):
        st.denoise_hop(dn, hop)
    st.reset()
    with pytest.raises(RuntimeError):
        st.denoise_hop(dn, hop)
    dn.reset()
    assert st.denoise_hop(dn, hop)[1] == 0
    # a split-mode stream refuses the whole-mode call
    st2 = pkg.Stream(plan, 2)
    st2.stft_hop(hop)
    with pytest.raises(RuntimeError):
        st2.denoise_hop(fresh, hop)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 4. accuracy against float64
def chain64(x, G, N, H, w, den):
    """The float64 chain as the plan runs it: w twice, the periodic divisor table."""
    X = R.stft(x.astype(np.float64), N, H, w)
    acc = np.zeros(len(x))
    for k in range(X.shape[0]):
        acc[k * H:k * H + N] += np.fft.irfft(X[k] * G[k], N) * w
    n = X.shape[0] * H
    return acc[:n] / den[np.arange(n) % len(den)]


@pytest.mark.parametrize("N,H", SHAPES)
def test_gains_and_output_against_the_float64_model(pkg, torch_cuda, oracle, N, H):
    torch = torch_cuda
    plan, C = plan_of(pkg, N, H), 2
    x = signal(N, H, C)
    w32 = pkg.window_table(pkg.HANN, N)
    w, den = w32.astype(np.float64), pkg.norm_table(w32, N, H).astype(np.float64)
    dn = pkg.Denoiser(plan, C, window=L)
    xd = torch.from_numpy(np.array(x)).cuda()
    G = dn.gains(plan.stft(xd)).cpu().numpy()
    y = dn.denoise(xd).cpu().numpy()
    for c in range(C):
        X64 = R.stft(x[c].astype(np.float64), N, H, w)
        G64, _ = R.gains(R.power(X64, np.float64), np.float64, window=L)
        d = np.abs(G[c].astype(np.float64) - G64)
        share = float(np.mean(d > 1e-3))
        y64 = chain64(x[c], G64, N, H, w, den)
        # the bar the float32 restatement sets on the oracle's kiss_fftr, same input
        _, So = oracle.roundtrip_mask(x[c], N, H, mode=oracle.DROP, want_spec=True)
        Go, _ = R.gains(R.power(So, np.float32), np.float32, window=L)
        yo = oracle.roundtrip_mask(x[c], N, H, mask=Go, mode=oracle.DROP)
        peak = np.max(np.abs(y64))

        def err(a):
            e = a.astype(np.float64) - y64
            return np.linalg.norm(e) / np.linalg.norm(y64), np.max(np.abs(e)) / peak

        rel, mx = err(y[c])
        rel_o, mx_o = err(yo)
        print(f"{N}/{H} ch{c}: max|dG| {d.max():.2e} share>1e-3 {share:.2e}; y rel-L2 {rel:.2e} peak {mx:.2e}; "
              f"oracle f32 rel-L2 {rel_o:.2e} peak {mx_o:.2e}")
        assert share <= 1e-3
        assert rel <= max(1e-6, 4 * rel_o) and mx <= max(4e-6, 4 * mx_o)
    dn.close()


# ------------------------------------------------------------------ 5. behaviour
def test_suppression_matches_the_float64_model(pkg, torch_cuda):
    """512/128, sqrt-Hann windows, L = 62, 500 frames, two channels through the hops: the
    noise removed in the gaps and the SNR gain in the bursts, second half of the run."""
    torch = torch_cuda
    N, H, frames, win = 512, 128, 500, 62
    w = R.sqrt_hann(N)
    w32 = w.astype(np.float32)
    plan = pkg.Plan(frame_size=N, hop_size=H, boundary_mode=pkg.DROP, frame_pairing=False)
    # the window runs twice (analysis, synthesis): the divisor is the overlap-added w^2
    norm = np.tile((w32.astype(np.float64) ** 2).reshape(N // H, H).sum(0), plan.ring_len // H).astype(np.float32)
    plan.upload_tables(window=w32, norm=norm)
    torch.cuda.synchronize()
    for seed in (7, 8):
        s, v, on = R.bursts(N, H, frames, seed=seed)
        x = (s + v).astype(np.float32)
        G64, _ = R.gains(R.power(R.stft(x.astype(np.float64), N, H, w), np.float64), np.float64, window=win)
        nr_m, gain_m = R.behaviour(G64, s, v, on, N, H, w)
        dn = pkg.Denoiser(plan, 1, window=win)
        y = run_stream(pkg, torch, plan, dn, x[None, :])[0]
        dn.reset()
        G = dn.gains(plan.stft(torch.from_numpy(x).cuda())).cpu().numpy()
        ypad = np.concatenate([y.astype(np.float64), np.zeros(len(x) - len(y))])
        nr_d, gain_d = R.behaviour(G, s, v, on, N, H, w, y=ypad)
        print(f"seed {seed}: model gap NR {nr_m:.2f} dB, SNR gain {gain_m:+.2f} dB; "
              f"device gap NR {nr_d:.2f} dB, SNR gain {gain_d:+.2f} dB")
        assert abs(nr_d - nr_m) <= 0.5 and abs(gain_d - gain_m) <= 0.5
        if seed == 7:
            assert nr_m >= 15.0 and gain_m >= 10.0
        dn.close()
    plan.close()
