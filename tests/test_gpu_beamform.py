"""GPU tests of the beamformer (include/crlot_dsp.h, "beamformer").

Bit for bit (a NaN equals a NaN: the sign and payload of a NaN are the hardware's, every
other value is compared by its bits): accumulate on the device's own crlot_stft rows equals
the float32 numpy restatement (tests/beamform_reference.py), through padded leading
dimensions and with sentinels around the state output, for each target; carry = 0 leaves
the object untouched; a run cut at every frame and carried equals the uncut run; a shared
mask equals the mask repeated; each group alone equals the batch; solve equals the
restatement in both modes on the object's state and on a caller's copy, the zero group
included; apply equals the restatement with caller and object weights; beamform equals the
hand composition with frame pairing on and off; hop over a run of hops equals the five-call
composition with update_every 1 and 3, and its weights equal solve on the carried state.
Launch records and grids, argument and counter errors through Python and through C, reset.

Against float64 (the model on numpy's FFT of the same x): planes and weights within the
larger of the CPU test's bars and 4 x what the float32 restatement shows on the oracle's
kiss_fftr spectra.  Behaviour: the scene of the CPU test at 512/128 with M = 4 through
beamform; the output's SINR improvement, measured by passing the target and the interferer
through the same weights with apply, is within 1 dB of the float64 model's.

Shapes: 256/128, 512/128, 1024/256, 960/240 (mixed radix); M = 2, 3, 4, 8; G = 1, 3;
F = 1, 3, 4, 5, 26 (the look-ahead's edges); N/2+1 bins put one live lane in the last wave.
With three groups, microphone 1 of group 0 carries a NaN, an Inf and a 1e-38 sample and
group 1 is all zeros.
"""
import ctypes as C

import numpy as np
import pytest

import beamform_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(256, 128), (512, 128), (1024, 256), (960, 240)]
MICS = (2, 3, 4, 8)
GROUPS = (1, 3)
FRAMES = (1, 3, 4, 5, 26)
F = 26
K_ACC, K_SOLVE, K_APPLY, K_HOP, K_STFT_HOP, K_ISTFT_HOP = 60, 61, 62, 63, 55, 56
CPU_BARS = dict(planes=1.5e-6, weights=7e-4)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "c":
        a, b = np.ascontiguousarray(a, np.complex64).view(np.float32), np.ascontiguousarray(b, np.complex64).view(np.float32)
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


_inputs, _plans, _spectra = {}, {}, {}


def signal(N, H, G, M, frames=F):
    """(x, mask): x (G, M, T) float32, group g the scene of seed 5 + g; with three groups,
    microphone 1 of group 0 carries a NaN, an Inf and a 1e-38 sample and group 1 is all zeros.
    mask (G, frames, bins) float32 uniform in [0, 1]."""
    key = (N, H, G, M, frames)
    if key not in _inputs:
        x = np.stack([R.scene(M, N, H, frames, seed=5 + g)[0] for g in range(G)]).astype(np.float32)
        if G >= 3:
            x[0, 1, 5], x[0, 1, N + 3], x[0, 1, 2 * N + 1] = np.nan, np.inf, np.float32(1e-38)
            x[1] = 0.0
        mask = np.random.default_rng(N + M).random((G, frames, N // 2 + 1)).astype(np.float32)
        x.setflags(write=False), mask.setflags(write=False)
        _inputs[key] = (x, mask)
    return _inputs[key]


def plan_of(pkg, N, H, pairing=False):
    if (N, H) not in _plans:
        _plans[(N, H)] = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True,
                                  boundary_mode=pkg.DROP, frame_pairing=False)
    p = _plans[(N, H)]
    p.set_frame_pairing(pairing)
    return p


def dev(torch, x):
    return torch.from_numpy(np.array(x)).cuda()


def device_spectra(torch, pkg, N, H, G, M):
    """(X, mask, Xn, maskn): the device's crlot_stft rows (G, M, F, bins) of signal(), the mask,
    and their host copies; computed once per shape."""
    key = (N, H, G, M)
    if key not in _spectra:
        x, mask = signal(N, H, G, M)
        X = plan_of(pkg, N, H).stft(dev(torch, x.reshape(G * M, -1))).view(G, M, F, N // 2 + 1)
        torch.cuda.synchronize()
        Xn = X.cpu().numpy()
        Xn.setflags(write=False)
        _spectra[key] = (X, dev(torch, mask), Xn, mask)
    return _spectra[key]


def padded(torch, S, fill=-7.0):
    """A copy of spectra (G, M, F, bins) inside a larger buffer: the frame and microphone strides padded."""
    G, M, Fr, bins = S.shape
    buf = torch.full((G, M, Fr + 1, bins + 3), fill, dtype=torch.complex64, device="cuda")
    view = buf[:, :, :Fr, :bins]
    view.copy_(S)
    return view


def padded_mask(torch, m, fill=-7.0):
    G, Fr, bins = m.shape
    buf = torch.full((G, Fr + 2, bins + 5), fill, dtype=torch.float32, device="cuda")
    view = buf[:, :Fr, :bins]
    view.copy_(m)
    return view


def fenced(torch, shape, dtype=None, fill=-7.0):
    """A contiguous tensor of `shape` with 64 sentinel elements on either side; returns (view, check)."""
    dtype = dtype or torch.float32
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), fill, dtype=dtype, device="cuda")
    view = buf[64:64 + n].view(*shape)
    return view, lambda: bool(torch.all(buf[:64] == fill)) and bool(torch.all(buf[64 + n:] == fill))


def steer_of(G, M, N):
    return np.stack([R.steering_from_delays((R.target_delays(M) - R.target_delays(M)[0]) + 0.25 * g, N) for g in range(G)])


# ------------------------------------------------------------------ 1. accumulate
@pytest.mark.parametrize("N,H", SHAPES)
def test_accumulate_equals_the_float32_restatement(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    for M in MICS:
        for G in GROUPS:
            X, mask, Xn, maskn = device_spectra(torch, pkg, N, H, G, M)
            assert X.shape == (G, M, F, bins)
            for alpha in (0.0, 0.9):
                bf = pkg.Beamformer(plan, M, G, alpha=alpha)
                other = pkg.Beamformer(plan, M, G + 1, alpha=alpha)
                for Fr in FRAMES if alpha else (5, F):
                    want = R.accumulate(Xn[:, :, :Fr], maskn[:, :Fr], 0, alpha)
                    if G >= 3:  # (crlot_stft maps the NaN and the Inf to 0: the spectra are finite)
                        assert np.all(want[1] == 0) and np.isfinite(want).all()
                    out, fence_ok = fenced(torch, (G, 2, M * M, bins))
                    got = other.accumulate(padded(torch, X[:, :, :Fr]), padded_mask(torch, mask[:, :Fr]), state_out=out)
                    torch.cuda.synchronize()
                    assert same(got.cpu().numpy(), want), (M, G, alpha, Fr)
                    assert fence_ok()
                    # carry = 0 takes any group count and leaves the object alone
                    assert other.frames == 0 and bool(torch.all(other.state() == 0))
                    rec = other.last_launch()
                    assert rec["kernels"] == [K_ACC] and rec["grids"] == [2 * G * ((bins + 63) // 64)]
                    assert rec["names"] == ["k_bf_acc"]
                    bf.reset()
                    live = bf.accumulate(X[:, :, :Fr], mask[:, :Fr], carry=True)
                    torch.cuda.synchronize()
                    assert same(live.cpu().numpy(), want) and bf.frames == Fr
                with pytest.raises(ValueError):
                    other.accumulate(X, mask, carry=True)
                bf.close(), other.close()


@pytest.mark.parametrize("N,H", [(256, 128), (960, 240)])
def test_each_target_updates_its_matrix_alone(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins, M, G = plan_of(pkg, N, H), N // 2 + 1, 3, 3
    X, mask, Xn, maskn = device_spectra(torch, pkg, N, H, G, M)
    bf = pkg.Beamformer(plan, M, G, alpha=0.9)
    for target in (pkg.BF_TARGET_SPEECH, pkg.BF_TARGET_NOISE):
        for m, mn in ((mask, maskn), (None, None)):
            want = R.accumulate(Xn, mn, target, 0.9)
            out, fence_ok = fenced(torch, (G, 2, M * M, bins))
            out.fill_(-3.0)
            bf.accumulate(X, m, target, state_out=out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert same(got[:, target - 1], want[:, target - 1]) and fence_ok()
            assert np.all(got[:, 2 - target] == -3.0)  # the other matrix is not written
            assert bf.last_launch()["grids"] == [G * ((bins + 63) // 64)]
            # carried: the other matrix keeps what it held
            bf.reset()
            bf.accumulate(X[:, :, :4], mask[:, :4], carry=True)
            before = bf.state().cpu().numpy()
            bf.accumulate(X[:, :, 4:], None if m is None else m[:, 4:], target, carry=True)
            after = bf.state().cpu().numpy()
            assert same(after[:, 2 - target], before[:, 2 - target]) and bf.frames == F
            assert same(after, R.accumulate(Xn[:, :, 4:], None if mn is None else mn[:, 4:], target, 0.9, state=before))
    with pytest.raises(ValueError):
        bf.accumulate(X, None, pkg.BF_TARGET_BOTH)
    bf.close()


@pytest.mark.parametrize("alpha", (0.0, 0.9))
@pytest.mark.parametrize("N,H", [(256, 128), (960, 240)])
def test_accumulate_cut_and_carried_equals_the_uncut_run(pkg, torch_cuda, N, H, alpha):
    torch = torch_cuda
    plan, M, G = plan_of(pkg, N, H), 3, 3
    X, mask, Xn, maskn = device_spectra(torch, pkg, N, H, G, M)
    bf = pkg.Beamformer(plan, M, G, alpha=alpha)
    whole = bf.accumulate(X, mask, carry=True).cpu().numpy()
    assert same(whole, R.accumulate(Xn, maskn, 0, alpha))
    for F1 in range(1, F):
        bf.reset()
        bf.accumulate(X[:, :, :F1], mask[:, :F1], carry=True)
        assert bf.frames == F1
        copy, fence_ok = fenced(torch, (G, 2, M * M, N // 2 + 1))
        bf.accumulate(X[:, :, F1:], mask[:, F1:], carry=True, state_out=copy)
        torch.cuda.synchronize()
        assert same(bf.state().cpu().numpy(), whole), F1
        assert same(copy.cpu().numpy(), whole) and fence_ok() and bf.frames == F
    bf.close()


@pytest.mark.parametrize("N,H", [(512, 128), (960, 240)])
def test_shared_mask_and_each_group_alone_equal_the_batch(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, M, G = plan_of(pkg, N, H), 4, 3
    X, mask, Xn, maskn = device_spectra(torch, pkg, N, H, G, M)
    for alpha in (0.0, 0.9):
        bf = pkg.Beamformer(plan, M, G, ref=2, alpha=alpha)
        batch = bf.accumulate(X, mask).cpu().numpy()
        w = bf.solve(bf.accumulate(X, mask, carry=True)).cpu().numpy()
        y = bf.apply(X).cpu().numpy()
        for g in range(G):
            st = bf.accumulate(X[g:g + 1], mask[g:g + 1])
            assert same(st.cpu().numpy()[0], batch[g]), g
            wg = torch.empty((1, M, N // 2 + 1), dtype=torch.complex64, device="cuda")
            bf.solve(st, weights=wg)
            assert same(wg.cpu().numpy()[0], w[g]), g
            assert same(bf.apply(X[g], wg).cpu().numpy(), y[g]), g
        rep = mask[2:3].repeat(G, 1, 1).contiguous()
        shared = bf.accumulate(X, mask[2]).cpu().numpy()
        assert same(shared, bf.accumulate(X, rep).cpu().numpy())
        assert same(shared, bf.accumulate(X, mask[2:3].expand(G, -1, -1)).cpu().numpy())
        assert same(shared, R.accumulate(Xn, maskn[2], 0, alpha))
        assert same(shared[2], batch[2]) and not same(shared[0], batch[0])
        bf.close()


# ------------------------------------------------------------------ 2. solve and apply
@pytest.mark.parametrize("N,H", SHAPES)
def test_solve_and_apply_equal_the_restatement(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    for M in MICS:
        for G in GROUPS:
            X, mask, Xn, maskn = device_spectra(torch, pkg, N, H, G, M)
            steer = steer_of(G, M, N)
            for mode, ref, alpha in (("souden", M - 1, 0.0), ("steered", 0, 0.9)):
                bf = pkg.Beamformer(plan, M, G, ref=ref, mode=mode, alpha=alpha)
                assert same(bf.weights().cpu().numpy(), R.passthrough(M, bins, ref, (G,)))
                assert same(bf.apply(X).cpu().numpy(), Xn[:, ref])  # the reference microphone passes through
                bf.set_steering(steer)
                st = bf.accumulate(X, mask, carry=True)
                stn = st.cpu().numpy()
                want = R.solve(stn, M, ref, bf.mode, 1e-3, steer)
                if G >= 3:  # the zero group: everything clamps at tiny
                    assert np.isfinite(want[1].view(np.float32)).all()
                    assert np.all(want[1] == 0) if mode == "souden" else True
                w = bf.solve()
                torch.cuda.synchronize()
                assert same(w.cpu().numpy(), want), (M, G, mode)
                rec = bf.last_launch()
                assert rec["names"] == ["k_bf_solve"] and rec["grids"] == [G * ((bins + 63) // 64)]
                # a caller's copies of the three blocks
                wc, fence_ok = fenced(torch, (G, M, bins), torch.complex64)
                other = pkg.Beamformer(plan, M, G + 2, ref=ref, mode=mode, alpha=alpha)
                other.solve(st.clone(), dev(torch, steer), wc)
                torch.cuda.synchronize()
                assert same(wc.cpu().numpy(), want) and fence_ok()
                assert same(other.weights().cpu().numpy(), R.passthrough(M, bins, ref, (G + 2,)))
                other.close()
                # apply: the object's weights, then a caller's with padded rows on both sides
                for Fr in (1, 5, F):
                    wanty = R.apply(Xn[:, :, :Fr], want)
                    assert same(bf.apply(X[:, :, :Fr]).cpu().numpy(), wanty), (M, G, mode, Fr)
                    buf = torch.full((G, Fr + 1, bins + 2), -7.0, dtype=torch.complex64, device="cuda")
                    bf.apply(padded(torch, X[:, :, :Fr]), wc, out=buf[:, :Fr, :bins])
                    torch.cuda.synchronize()
                    assert same(buf[:, :Fr, :bins].cpu().numpy(), wanty)
                    assert bool(torch.all(buf[:, Fr:] == -7.0)) and bool(torch.all(buf[:, :, bins:] == -7.0))
                    assert bf.last_launch()["names"] == ["k_bf_apply"]
                bf.close()


def test_non_finite_spectra_propagate_as_in_the_restatement(pkg, torch_cuda):
    """crlot_stft never stores a NaN, but a caller's spectra may hold one: the clamps are a
    compare and a select, so the NaNs land where the restatement puts them."""
    torch = torch_cuda
    N, H, M, G = 256, 128, 3, 1
    plan = plan_of(pkg, N, H)
    X, mask, Xn, maskn = device_spectra(torch, pkg, N, H, G, M)
    Xn = Xn.copy()
    Xn[0, 1, 2, 7], Xn[0, 0, 3, 9], Xn[0, 2, 4, 11] = np.nan, np.inf, complex(0.0, -np.inf)
    Xd = dev(torch, Xn)
    for mode in ("souden", "steered"):
        bf = pkg.Beamformer(plan, M, G, mode=mode, alpha=0.9)
        steer = steer_of(G, M, N)
        bf.set_steering(steer)
        st = bf.accumulate(Xd, mask, carry=True).cpu().numpy()
        want = R.accumulate(Xn, maskn, 0, 0.9)
        assert np.isnan(want[..., 7]).any() and not np.isfinite(want[..., 9]).all() and not np.isfinite(want[..., 11]).all()
        assert same(st, want)
        w = bf.solve().cpu().numpy()
        wantw = R.solve(want, M, 0, bf.mode, 1e-3, steer)
        assert same(w, wantw)
        assert same(bf.apply(Xd).cpu().numpy(), R.apply(Xn, wantw))
        bf.close()


def test_apply_chunking_changes_no_bit(pkg, torch_cuda):
    """A long run at one group is cut into chunks of frames across the grid; a group of the
    same spectra repeated (fewer chunks per group) gives the same rows."""
    torch = torch_cuda
    N, H, M = 256, 128, 2
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    rng = np.random.default_rng(9)
    Xn = (rng.standard_normal((1, M, 700, bins)) + 1j * rng.standard_normal((1, M, 700, bins))).astype(np.complex64)
    wn = (rng.standard_normal((1, M, bins)) + 1j * rng.standard_normal((1, M, bins))).astype(np.complex64)
    bf = pkg.Beamformer(plan, M, 1)
    y1 = bf.apply(dev(torch, Xn), dev(torch, wn)).cpu().numpy()
    g1 = bf.last_launch()["grids"][0]
    assert g1 > (bins + 63) // 64  # more than one chunk of frames
    assert same(y1, R.apply(Xn, wn))
    y4 = bf.apply(dev(torch, np.repeat(Xn, 4, 0)), dev(torch, np.repeat(wn, 4, 0))).cpu().numpy()
    for g in range(4):
        assert same(y4[g], y1[0])
    bf.close()


# ------------------------------------------------------------------ 3. the composite entry
@pytest.mark.parametrize("pairing", (False, True))
@pytest.mark.parametrize("N,H", SHAPES)
def test_beamform_equals_the_hand_composition(pkg, torch_cuda, N, H, pairing):
    torch = torch_cuda
    bins = N // 2 + 1
    for M, G in ((4, 3), (2, 1), (8, 1)):
        x, maskn = signal(N, H, G, M)
        xd, mask = dev(torch, x), dev(torch, maskn)
        steer = steer_of(G, M, N)
        for mode, m in (("souden", mask), ("steered", mask), ("steered", None)):
            plan = plan_of(pkg, N, H, pairing)
            bf = pkg.Beamformer(plan, M, G, ref=1, mode=mode, alpha=0.9)
            bf.set_steering(steer)
            X = plan.stft(xd.view(G * M, -1)).view(G, M, F, bins)
            st = bf.accumulate(X, m, pkg.BF_TARGET_BOTH if m is not None else pkg.BF_TARGET_NOISE)
            w = torch.empty((G, M, bins), dtype=torch.complex64, device="cuda")
            bf.solve(st, dev(torch, steer), w)
            want = plan.istft_ola(bf.apply(X, w))
            buf = torch.full((G, F * H + 7), -7.0, device="cuda")
            got = bf.beamform(xd, m, y=buf[:, :F * H])
            torch.cuda.synchronize()
            assert same(got.cpu().numpy(), want.cpu().numpy()), (M, G, mode, m is None)
            assert bool(torch.all(buf[:, F * H:] == -7.0))
            assert bf.last_launch()["names"] == ["k_bf_acc", "k_bf_solve", "k_bf_apply"]
            # the object is untouched
            assert bf.frames == 0 and bool(torch.all(bf.state() == 0))
            assert same(bf.weights().cpu().numpy(), R.passthrough(M, bins, 1, (G,)))
            if G == 3:
                gotn = got.cpu().numpy()
                assert np.all(gotn[1] == 0) and np.isfinite(gotn[2]).all()
            bf.close()
    plan = plan_of(pkg, N, H, False)
    bf = pkg.Beamformer(plan, 2, 1)
    x, maskn = signal(N, H, 1, 2)
    with pytest.raises(ValueError):
        bf.beamform(dev(torch, x), None)  # SOUDEN needs a mask
    plan.set_spectral_mask(dev(torch, maskn[0]))
    try:
        with pytest.raises(ValueError):
            bf.beamform(dev(torch, x), dev(torch, maskn))
    finally:
        plan.set_spectral_mask(None)
    bf.close()


# ------------------------------------------------------------------ 4. the per-hop entry
@pytest.mark.parametrize("update_every", (1, 3))
@pytest.mark.parametrize("N,H,M,G", [(256, 128, 4, 3), (960, 240, 3, 1), (512, 128, 8, 1)])
def test_hop_equals_the_five_call_composition(pkg, torch_cuda, N, H, M, G, update_every):
    torch = torch_cuda
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    hops = N // H - 1 + 8
    x, maskn = signal(N, H, G, M)
    xd, mask = dev(torch, x.reshape(G * M, -1)), dev(torch, maskn)
    for mode in ("souden", "steered"):
        a = pkg.Beamformer(plan, M, G, ref=1, mode=mode, alpha=0.9, update_every=update_every)
        b = pkg.Beamformer(plan, M, G, ref=1, mode=mode, alpha=0.9, update_every=update_every)
        a.set_steering(steer_of(G, M, N)), b.set_steering(steer_of(G, M, N))
        sa_in, sa_out = pkg.Stream(plan, G * M), pkg.Stream(plan, G)
        sb_in, sb_out = pkg.Stream(plan, G * M), pkg.Stream(plan, G)
        k = 0
        for q in range(hops):
            hop = xd[:, q * H:(q + 1) * H].contiguous()
            out = torch.full((G, H), -7.0, device="cuda")
            row = mask[:, k] if k % 2 else mask[0, k]  # a row per group, or one shared row
            got, em = a.hop(sa_in, sa_out, hop, row, out)
            rec = a.last_launch()
            spec, em_b = sb_in.stft_hop(hop)
            if q < N // H - 1:
                assert em == 0 and em_b == 0 and bool(torch.all(out == -7.0)) and a.frames == 0
                assert rec["kernels"] == [K_STFT_HOP]
                continue
            assert em == H and em_b == 1
            spec4 = spec.view(G, M, 1, bins)
            row_b = row[:, None, :] if k % 2 else row[None, :]
            b.accumulate(spec4, row_b, carry=True)
            due = (k + 1) % update_every == 0
            if due:
                b.solve()
            want = sb_out.istft_hop(b.apply(spec4)[:, 0].contiguous())
            torch.cuda.synchronize()
            assert same(got.cpu().numpy(), want.cpu().numpy()), (mode, q)
            assert same(a.state().cpu().numpy(), b.state().cpu().numpy()), (mode, q)
            assert same(a.weights().cpu().numpy(), b.weights().cpu().numpy()), (mode, q)
            assert rec["kernels"] == [K_STFT_HOP, K_HOP, K_ISTFT_HOP] and rec["grids"][1] == G * ((bins + 63) // 64)
            assert rec["names"][1] == "k_bf_hop"
            k += 1
            assert a.frames == k == b.frames
        # its weights are solve on the carried state (as of the last frame a solve was due)
        if update_every == 1:
            w = torch.empty((G, M, bins), dtype=torch.complex64, device="cuda")
            a.solve(a.state().clone(), weights=w)
            assert same(w.cpu().numpy(), a.weights().cpu().numpy())
        # counters that differ are refused; reset brings all three back
        other = pkg.Stream(plan, G)
        with pytest.raises(RuntimeError):
            a.hop(sa_in, other, xd[:, :H].contiguous(), mask[0, 0])
        a.reset(), sa_in.reset(), sa_out.reset()
        assert a.frames == 0 and bool(torch.all(a.state() == 0))
        assert same(a.weights().cpu().numpy(), R.passthrough(M, bins, 1, (G,)))
        _, em = a.hop(sa_in, sa_out, xd[:, :H].contiguous(), mask[0, 0])
        assert em == 0
        for o in (a, b, sa_in, sa_out, sb_in, sb_out, other):
            o.close()


# ------------------------------------------------------------------ 5. arguments
def test_argument_and_counter_errors(pkg, torch_cuda):
    torch = torch_cuda
    N, H, M, G = 256, 128, 3, 2
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    other_plan = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True, boundary_mode=pkg.DROP)
    for kw in (dict(mics=1), dict(mics=9), dict(ref=3), dict(mode="gev"), dict(alpha=1.0), dict(loading=-1.0),
               dict(update_every=0), dict(groups=0)):
        with pytest.raises(ValueError):
            pkg.Beamformer(plan, **{"mics": M, **kw})
    bf = pkg.Beamformer(plan, M, G)
    X = torch.zeros((G, M, 4, bins), dtype=torch.complex64, device="cuda")
    mask = torch.ones((G, 4, bins), device="cuda")
    with pytest.raises(ValueError):
        bf.accumulate(X[:, :2], mask)  # the microphone count
    with pytest.raises(ValueError):
        bf.accumulate(X.cpu(), mask)
    with pytest.raises(ValueError):
        bf.accumulate(X, mask.double())
    with pytest.raises(ValueError):
        bf.accumulate(X, mask[:, :3])
    with pytest.raises(ValueError):
        bf.accumulate(X, mask, target=3)
    with pytest.raises(ValueError):
        bf.accumulate(X[:1], mask[:1], carry=True)  # carry needs the object's group count
    with pytest.raises(ValueError):
        bf.accumulate(X, mask, state_out=torch.zeros((G, 2, M * M, bins + 1), device="cuda"))
    with pytest.raises(ValueError):
        bf.solve(torch.zeros((G + 1, 2, M * M, bins), device="cuda"))  # the object's weights: G groups
    with pytest.raises(ValueError):
        bf.apply(X[:1])
    with pytest.raises(ValueError):
        bf.apply(X, out=torch.zeros((G, 4, bins), dtype=torch.complex64))
    with pytest.raises(ValueError):
        bf.set_weights(np.zeros((G, M, bins + 1), np.complex64))
    # through C: the checks the Python layer makes first
    L = pkg.lib()
    st = torch.zeros((G, 2, M * M, bins), device="cuda")
    row = 2 * bins
    args = dict(spec=X.data_ptr(), ld=4 * row, ldf=row, mask=mask.data_ptr(), ldm=4 * bins, ldfm=bins)

    def acc(spec=args["spec"], ld=args["ld"], ldf=args["ldf"], m=args["mask"], ldm=args["ldm"], ldfm=args["ldfm"], g=G,
            f=4, target=0, carry=0, out=st.data_ptr()):
        return L.crlot_beamform_accumulate(bf._h, spec, ld, ldf, m, ldm, ldfm, g, f, target, carry, out, None)

    assert acc() == 0
    assert acc(g=0) == 0 and acc(f=0) == 0
    for bad in (dict(spec=None), dict(out=None), dict(m=None), dict(ld=4 * row - 2), dict(ldf=row - 2), dict(ldf=row + 1),
                dict(ld=4 * row + 1), dict(spec=X.data_ptr() + 4), dict(ldfm=bins - 1), dict(ldm=4 * bins - 1),
                dict(target=3), dict(target=-1), dict(carry=2), dict(g=-1), dict(f=-1), dict(g=G + 1, carry=1),
                dict(out=X.data_ptr()), dict(out=mask.data_ptr())):
        assert acc(**bad) == pkg.EINVAL, bad
    assert acc(carry=1, out=bf.state().data_ptr()) == pkg.EINVAL  # the state output is the object's state
    assert bf.frames == 0
    w = torch.zeros((G, M, bins), dtype=torch.complex64, device="cuda")
    assert L.crlot_beamform_solve(bf._h, st.data_ptr(), None, G, w.data_ptr(), None) == 0
    assert L.crlot_beamform_solve(bf._h, st.data_ptr(), None, G, st.data_ptr(), None) == pkg.EINVAL
    assert L.crlot_beamform_solve(bf._h, None, None, G + 1, w.data_ptr(), None) == pkg.EINVAL
    assert L.crlot_beamform_solve(bf._h, st.data_ptr(), None, -1, w.data_ptr(), None) == pkg.EINVAL
    out = torch.zeros((G, 4, bins), dtype=torch.complex64, device="cuda")

    def app(spec=X.data_ptr(), wp=w.data_ptr(), g=G, o=out.data_ptr(), ldo=4 * row, ldfo=row):
        return L.crlot_beamform_apply(bf._h, spec, 4 * row, row, wp, g, 4, o, ldo, ldfo, None)

    assert app() == 0
    for bad in (dict(spec=None), dict(o=None), dict(o=X.data_ptr()), dict(o=w.data_ptr()), dict(ldo=4 * row - 2),
                dict(ldfo=row - 2), dict(ldfo=row + 1), dict(wp=None, g=G - 1), dict(o=out.data_ptr() + 4)):
        assert app(**bad) == pkg.EINVAL, bad
    # the per-hop entry: channel counts, plans, a stream in whole-hop mode
    hop = torch.zeros((G * M, H), device="cuda")
    mrow = torch.ones((bins,), device="cuda")
    s_in, s_out = pkg.Stream(plan, G * M), pkg.Stream(plan, G)
    with pytest.raises(ValueError):
        bf.hop(s_out, s_out, hop, mrow)
    with pytest.raises(ValueError):
        bf.hop(s_in, pkg.Stream(other_plan, G), hop, mrow)
    with pytest.raises(ValueError):
        bf.hop(s_in, s_out, hop, None)
    em = C.c_int32(7)
    o = torch.zeros((G, H), device="cuda")
    hopc = lambda a, b: L.crlot_stream_beamform_hop(a, b, bf._h, hop.data_ptr(), mrow.data_ptr(), 0, o.data_ptr(),  # noqa: E731
                                                    C.byref(em), None)
    assert hopc(s_out._h, s_out._h) == pkg.EINVAL and em.value == 0
    assert hopc(s_in._h, s_in._h) == pkg.EINVAL
    wrong = pkg.Stream(other_plan, G)
    assert hopc(s_in._h, wrong._h) == pkg.EINVAL
    whole = pkg.Stream(plan, G)
    whole.push_hop(torch.zeros((G, H), device="cuda"))
    assert hopc(s_in._h, whole._h) == pkg.ERUNTIME
    bf.accumulate(X, mask, carry=True)  # the object's counter now leads the streams'
    assert hopc(s_in._h, s_out._h) == pkg.ERUNTIME
    bf.reset()
    assert hopc(s_in._h, s_out._h) == 0 and em.value == 0
    torch.cuda.synchronize()
    for obj in (bf, s_in, s_out, wrong, whole, other_plan):
        obj.close()


# ------------------------------------------------------------------ 6. against float64, behaviour
def _model(pkg, oracle, N, H, M, x, mask):
    """The float64 model on numpy's FFT of x (M, T), and the float32 restatement on the
    oracle's kiss_fftr spectra of the same input: (state, weights) of each."""
    w32 = pkg.window_table(pkg.HANN, N, True)
    st64 = R.accumulate(R.stft(x, N, H, w32.astype(np.float64)), mask, 0, 0.0, np.float64)
    k = oracle.KissR(N)
    Fr = (x.shape[-1] - N) // H + 1
    X32 = np.stack([np.stack([k.forward(row[f * H:f * H + N].astype(np.float32) * w32) for f in range(Fr)]) for row in x])
    st32 = R.accumulate(X32, mask.astype(np.float32), 0, 0.0)
    return (st64, R.solve(st64, M, 0, R.SOUDEN, 1e-3, None, np.float64)), (st32, R.solve(st32, M, 0))


def _differences(st, w, st64, w64):
    planes = max(np.abs(st[m].astype(np.float64) - st64[m]).max() / np.abs(st64[m]).max() for m in range(2))
    return dict(planes=planes, weights=np.abs(w - w64).max() / np.abs(w64).max())


@pytest.mark.parametrize("M", (4, 8))
@pytest.mark.parametrize("N,H", SHAPES)
def test_state_and_weights_against_the_float64_model(pkg, oracle, torch_cuda, N, H, M):
    torch = torch_cuda
    plan = plan_of(pkg, N, H)
    x, s, v = R.scene(M, N, H, 60)
    wn = R.hann(N)
    mask = R.ideal_ratio_mask(R.stft(s, N, H, wn), R.stft(v, N, H, wn))
    (st64, w64), (st32, w32) = _model(pkg, oracle, N, H, M, x, mask)
    bf = pkg.Beamformer(plan, M, 1)
    X = plan.stft(dev(torch, x.astype(np.float32))).view(1, M, 60, N // 2 + 1)
    st = bf.accumulate(X, dev(torch, mask.astype(np.float32)), carry=True)
    w = bf.solve()
    torch.cuda.synchronize()
    model = _differences(st32, w32, st64, w64)
    device = _differences(st.cpu().numpy()[0], w.cpu().numpy()[0], st64, w64)
    bf.close()
    for k, floor in CPU_BARS.items():
        print(f"beamform-f64 {N}/{H} M={M} {k}: restatement on kiss_fftr {model[k]:.2e}, "
              f"bar {max(floor, 4 * model[k]):.2e}, device {device[k]:.2e}")
    for k, floor in CPU_BARS.items():
        assert device[k] <= max(floor, 4 * model[k]), k


def test_sinr_improvement_is_the_models(pkg, torch_cuda):
    torch = torch_cuda
    N, H, M = 512, 128, 4
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    x, s, v = R.scene(M, N, H, 60)
    wn = R.hann(N)
    S64, V64 = R.stft(s, N, H, wn), R.stft(v, N, H, wn)
    mask = R.ideal_ratio_mask(S64, V64)
    st64 = R.accumulate(R.stft(x, N, H, wn), mask, 0, 0.0, np.float64)
    g64 = R.sinr_gain_db(S64, V64, R.solve(st64, M, 0, R.SOUDEN, 1e-3, None, np.float64))
    bf = pkg.Beamformer(plan, M, 1)
    xd, md = dev(torch, x.astype(np.float32)), dev(torch, mask.astype(np.float32))
    y = bf.beamform(xd, md)
    # the same weights by hand (beamform keeps its own in scratch), then the target and the
    # interferer through them separately
    X = plan.stft(xd).view(1, M, 60, bins)
    bf.accumulate(X, md, carry=True)
    bf.solve()
    assert same(plan.istft_ola(bf.apply(X)).cpu().numpy(), y.cpu().numpy()[None] if y.dim() == 1 else y.cpu().numpy())
    Sd = plan.stft(dev(torch, s.astype(np.float32))).view(1, M, 60, bins)
    Vd = plan.stft(dev(torch, v.astype(np.float32))).view(1, M, 60, bins)
    Ys, Yv = bf.apply(Sd).cpu().numpy().astype(np.complex128), bf.apply(Vd).cpu().numpy().astype(np.complex128)
    torch.cuda.synchronize()
    gain = R.sinr_db(Ys, Yv) - R.sinr_db(Sd.cpu().numpy()[0, 0].astype(np.complex128),
                                         Vd.cpu().numpy()[0, 0].astype(np.complex128))
    print(f"SINR improvement: device {gain:.2f} dB, float64 model {g64:.2f} dB")
    assert abs(gain - g64) <= 1.0
    bf.close()
