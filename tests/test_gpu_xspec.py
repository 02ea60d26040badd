"""GPU tests of the cross-spectral estimator (include/crlot_dsp.h, "cross-spectral estimation").

Bit for bit: accumulate on the device's own crlot_stft rows equals the float32 numpy
restatement (tests/xspec_reference.py), through padded leading dimensions and with
sentinels around the state output; carry = 0 leaves the object untouched; a run cut at
every frame and carried equals the uncut run; a shared reference equals the reference
repeated; each pair alone equals the batch; derive's subsets equal the restatement and
the all-three call; peak equals the restatement on crafted rows; estimate and delay equal
their hand compositions; F = 1 accumulates on Stream.stft_hop rows equal estimate over the
whole input.  Against float64 (the model on numpy's FFT of the same x): coherence, PHAT W
and the planes within the larger of the CPU test's bars and 4 x what the float32
restatement shows on the oracle's kiss_fftr spectra; the integer lag of five delays exact
at every power-of-two shape; frac within 4 x the restatement's difference (floor 1e-5).
Behaviour: H1 turned into taps cancels the echo of the same system by 30 dB or more.

Shapes: 256/128, 512/128, 1024/256, 2048/512, 960/240 (mixed radix); pairs 1, 3, 5;
F = 1, 3, 4, 5, 26 (the look-ahead's edges); N/2+1 bins put one live lane in the last wave.
With three pairs or more, b of pair 1 carries a NaN, an Inf and a 1e-38 sample and pair 2
is all zeros.
"""
import ctypes

import numpy as np
import pytest

import xspec_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(256, 128), (512, 128), (1024, 256), (2048, 512), (960, 240)]
POW2 = SHAPES[:4]
PAIRS = (1, 3, 5)
FRAMES = (1, 3, 4, 5, 26)
F = 26
ALPHAS = (0.0, 0.9)
K_ACC, K_DERIVE, K_PEAK = 57, 58, 59
DELAYS = (3, 0, -20, 37, 1)  # pair p of a batch is delayed by DELAYS[p]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "c":
        a, b = np.ascontiguousarray(a, np.complex64).view(np.float32), np.ascontiguousarray(b, np.complex64).view(np.float32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


_inputs, _plans = {}, {}


def signal(N, H, P, frames=F):
    """(a, b), each (P, T) float32: pair p is a white reference and its copy delayed by
    DELAYS[p] plus noise; with three pairs or more b of pair 1 carries a NaN, an Inf and a
    1e-38 sample and pair 2 is all zeros."""
    key = (N, H, P, frames)
    if key not in _inputs:
        T = R.length(N, H, frames)
        rows = [R.delayed_pair(T, DELAYS[p], seed=11 + p) for p in range(P)]
        a = np.stack([r[0] for r in rows]).astype(np.float32)
        b = np.stack([r[1] for r in rows]).astype(np.float32)
        if P >= 3:
            b[1, 5], b[1, N + 3], b[1, 2 * N + 1] = np.nan, np.inf, np.float32(1e-38)
            a[2], b[2] = 0.0, 0.0
        a.setflags(write=False), b.setflags(write=False)
        _inputs[key] = (a, b)
    return _inputs[key]


def plan_of(pkg, N, H):
    if (N, H) not in _plans:
        _plans[(N, H)] = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True,
                                  boundary_mode=pkg.DROP, frame_pairing=False)
    p = _plans[(N, H)]
    p.set_frame_pairing(False)
    return p


def dev(torch, x):
    return torch.from_numpy(np.array(x)).cuda()


def device_spectra(torch, plan, N, H, P, frames=F):
    a, b = signal(N, H, P, frames)
    A, B = plan.stft(dev(torch, a)), plan.stft(dev(torch, b))
    torch.cuda.synchronize()
    return A, B


def padded(torch, S, fill=-7.0):
    """A copy of spectra (P, F, bins) inside a larger buffer: both leading dimensions padded."""
    P, Fr, bins = S.shape
    buf = torch.full((P, Fr + 1, bins + 3), fill, dtype=torch.complex64, device="cuda")
    view = buf[:, :Fr, :bins]
    view.copy_(S)
    return view


def fenced_state(torch, P, bins):
    """A (P, 4, bins) state output with 64 sentinel floats on either side; returns (view, check)."""
    n = P * 4 * bins
    buf = torch.full((n + 128,), -7.0, device="cuda")
    view = buf[64:64 + n].view(P, 4, bins)
    return view, lambda: bool(torch.all(buf[:64] == -7.0)) and bool(torch.all(buf[64 + n:] == -7.0))


# ------------------------------------------------------------------ 1. accumulate
@pytest.mark.parametrize("N,H", SHAPES)
def test_accumulate_equals_the_float32_restatement(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins = plan_of(pkg, N, H), N // 2 + 1
    for P in PAIRS:
        A, B = device_spectra(torch, plan, N, H, P)
        assert A.shape == (P, F, bins)
        An, Bn = A.cpu().numpy(), B.cpu().numpy()
        assert np.isfinite(Bn).all()
        for alpha in ALPHAS:
            xs = pkg.CrossSpectrum(plan, P, alpha)
            other = pkg.CrossSpectrum(plan, P + 1, alpha)
            for Fr in FRAMES:
                want = R.accumulate(An[:, :Fr], Bn[:, :Fr], alpha)
                if P >= 3:
                    assert np.all(want[2] == 0)
                out, fence_ok = fenced_state(torch, P, bins)
                got = other.accumulate(padded(torch, A[:, :Fr]), padded(torch, B[:, :Fr]), state_out=out)
                torch.cuda.synchronize()
                assert same(got.cpu().numpy(), want), (P, alpha, Fr)
                assert fence_ok()
                # carry = 0 takes any pair count and leaves the object alone
                assert other.frames == 0 and bool(torch.all(other.state() == 0))
                rec = other.last_launch()
                assert rec["kernels"] == [K_ACC] and rec["grids"] == [P * ((bins + 63) // 64)]
                assert rec["names"] == ["k_xspec_acc"]
                xs.reset()
                live = xs.accumulate(A[:, :Fr], B[:, :Fr], carry=True)
                torch.cuda.synchronize()
                assert same(live.cpu().numpy(), want) and xs.frames == Fr
            with pytest.raises(ValueError):
                other.accumulate(A, B, carry=True)
            xs.close(), other.close()


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,H", [(256, 128), (960, 240)])
def test_accumulate_cut_and_carried_equals_the_uncut_run(pkg, torch_cuda, N, H, alpha):
    torch = torch_cuda
    plan, P = plan_of(pkg, N, H), 3
    A, B = device_spectra(torch, plan, N, H, P)
    xs = pkg.CrossSpectrum(plan, P, alpha)
    whole = xs.accumulate(A, B, carry=True).cpu().numpy()
    assert same(whole, R.accumulate(A.cpu().numpy(), B.cpu().numpy(), alpha))
    for F1 in range(1, F):
        xs.reset()
        xs.accumulate(A[:, :F1], B[:, :F1], carry=True)
        assert xs.frames == F1
        copy, fence_ok = fenced_state(torch, P, N // 2 + 1)
        xs.accumulate(A[:, F1:], B[:, F1:], carry=True, state_out=copy)
        torch.cuda.synchronize()
        assert same(xs.state().cpu().numpy(), whole), F1
        assert same(copy.cpu().numpy(), whole) and fence_ok() and xs.frames == F
    xs.close()


@pytest.mark.parametrize("N,H", [(512, 128), (960, 240)])
def test_shared_reference_and_each_pair_alone_equal_the_batch(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, P = plan_of(pkg, N, H), 5
    A, B = device_spectra(torch, plan, N, H, P)
    for alpha in ALPHAS:
        xs = pkg.CrossSpectrum(plan, P, alpha)
        batch = xs.accumulate(A, B).cpu().numpy()
        for p in range(P):
            assert same(xs.accumulate(A[p:p + 1], B[p:p + 1]).cpu().numpy()[0], batch[p]), p
        rep = A[3:4].repeat(P, 1, 1).contiguous()
        shared = xs.accumulate(A[3], B).cpu().numpy()
        assert same(shared, xs.accumulate(rep, B).cpu().numpy())
        assert same(shared, R.accumulate(A[3].cpu().numpy(), B.cpu().numpy(), alpha))
        assert same(shared[3], batch[3]) and not same(shared[0], batch[0])
        xs.close()


# ------------------------------------------------------------------ 2. derive
@pytest.mark.parametrize("N,H", SHAPES)
def test_derive_subsets_equal_the_restatement(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins, P = plan_of(pkg, N, H), N // 2 + 1, 5
    A, B = device_spectra(torch, plan, N, H, P)
    names = ("coherence", "transfer", "weighted")
    for alpha in ALPHAS:
        xs = pkg.CrossSpectrum(plan, P, alpha)
        state = xs.accumulate(A, B, carry=True)
        st = state.cpu().numpy()
        for wt in (pkg.XSPEC_NONE, pkg.XSPEC_PHAT):
            want = dict(zip(names, R.derive(st, wt)))
            assert np.all(want["coherence"][2] == 0) and np.all(want["weighted"][2] == 0)
            for subset in range(1, 8):
                pick = [n for i, n in enumerate(names) if subset >> i & 1]
                bufs = {n: torch.full((P + 1, bins + 3), -7.0, device="cuda",
                                      dtype=torch.float32 if n == "coherence" else torch.complex64) for n in pick}
                # the object's own state on odd subsets, the caller's copy on even ones
                got = xs.derive(None if subset & 1 else state.clone(), wt, want=(),
                                **{n: b[:P, :bins] for n, b in bufs.items()})
                torch.cuda.synchronize()
                assert sorted(got) == sorted(pick)
                for n in pick:
                    assert same(got[n].cpu().numpy(), want[n]), (alpha, wt, subset, n)
                    assert bool(torch.all(bufs[n][P:] == -7.0)) and bool(torch.all(bufs[n][:, bins:] == -7.0))
                rec = xs.last_launch()
                assert rec["kernels"] == [K_DERIVE] and rec["grids"] == [P * ((bins + 255) // 256)]
        assert same(xs.coherence().cpu().numpy(), R.derive(st)[0])
        assert same(xs.transfer().cpu().numpy(), R.derive(st)[1])
        assert same(xs.weighted().cpu().numpy(), R.derive(st, R.PHAT)[2])
        xs.close()


# ------------------------------------------------------------------ 3. peak
def crafted_rows(N):
    """Rows for the peak search at max_lag m, as (rows, m) cases."""
    rng = np.random.default_rng(5)
    cases = []
    for m in (1, 33, N // 2 - 1):
        J = 2 * m

        def at(j):
            return (j - m) % N

        base = (rng.standard_normal(N) * 0.1).astype(np.float32)
        rows = [base.copy()]
        for first, step in ((0, 64), (1, 63), (J // 2, 65), (2, 1), (J - 1, 64)):  # ties across lanes
            r = base.copy()
            r[[at(j) for j in range(first, J + 1, step)]] = 5.0
            rows.append(r)
        r = base.copy(); r[at(0)] = 7.0; rows.append(r)  # noqa: E702  a maximum at either end
        r = base.copy(); r[at(J)] = 7.0; rows.append(r)  # noqa: E702
        r = base.copy(); r[at(0)] = r[at(J)] = 7.0; rows.append(r)  # noqa: E702
        for j in (1, J // 2, J):  # a NaN elsewhere than the winner
            r = base.copy(); r[at(j)] = np.nan; r[at(J // 2 - 1 if j == J // 2 else J // 2)] = 3.0; rows.append(r)  # noqa: E702
        rows.append(np.full(N, 0.25, np.float32))  # den = 0
        r = np.full(N, -1.0, np.float32); r[at(0)], r[at(1)] = 0.0, -0.0; rows.append(r)  # noqa: E702
        r = np.zeros(N, np.float32); r[at(m - 1)], r[at(m)], r[at(m + 1)] = 1.0, 2.0, 2.0; rows.append(r)  # noqa: E702
        cases.append((np.stack(rows), m))
    return cases


@pytest.mark.parametrize("N,H", [(256, 128), (2048, 512), (960, 240)])
def test_peak_equals_the_restatement_on_crafted_rows(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan = plan_of(pkg, N, H)
    xs = pkg.CrossSpectrum(plan, 1)
    for rows, m in crafted_rows(N):
        P = len(rows)
        want = R.peak(rows, m)
        cc = torch.full((P, N + 5), -9.0, device="cuda")
        cc[:, :N] = dev(torch, rows)
        buf = torch.full((P + 1, 4), -7.0, device="cuda")
        got = xs.peak(cc[:, :N], m, out=buf[:P, :3])
        torch.cuda.synchronize()
        g = got.cpu().numpy()
        ok = np.array_equal(bits(g), bits(want)) or (np.array_equal(np.isnan(g), np.isnan(want)) and
                                                      np.array_equal(bits(np.nan_to_num(g)), bits(np.nan_to_num(want))))
        assert ok, (m, g, want)
        assert bool(torch.all(buf[P:] == -7.0)) and bool(torch.all(buf[:, 3:] == -7.0))
        rec = xs.last_launch()
        assert rec["kernels"] == [K_PEAK] and rec["grids"] == [P] and rec["names"] == ["k_xspec_peak"]
        assert same(xs.peak(cc[3:4, :N], m).cpu().numpy(), want[3:4])  # a row alone
    xs.close()


# ------------------------------------------------------------------ 4. the composites
@pytest.mark.parametrize("N,H", SHAPES)
@pytest.mark.parametrize("pairing", [False, True])
def test_estimate_equals_the_hand_composition(pkg, torch_cuda, N, H, pairing):
    torch = torch_cuda
    plan, bins, P = plan_of(pkg, N, H), N // 2 + 1, 5
    plan.set_frame_pairing(pairing)
    a, b = signal(N, H, P)
    xa, xb = dev(torch, a), dev(torch, b)
    for alpha in ALPHAS:
        xs = pkg.CrossSpectrum(plan, P, alpha)
        A, B = plan.stft(xa), plan.stft(xb)
        want = xs.accumulate(A, B).cpu().numpy()
        out, fence_ok = fenced_state(torch, P, bins)
        got = xs.estimate(xa, xb, state_out=out)
        torch.cuda.synchronize()
        assert same(got.cpu().numpy(), want) and fence_ok() and xs.frames == 0
        assert "k_xspec_acc" in plan.last_launch()["kernels"]
        assert xs.last_launch()["kernels"] == [K_ACC]
        # a shared reference: one transform of it
        want_sh = xs.accumulate(plan.stft(xa[1]), B).cpu().numpy()
        assert same(xs.estimate(xa[1], xb).cpu().numpy(), want_sh)
        # carried: twice the input is the state of the spectra run twice
        xs.estimate(xa, xb, carry=True)
        live = xs.estimate(xa, xb, carry=True)
        assert xs.frames == 2 * F
        twice = xs.accumulate(torch.cat([A, A], dim=1), torch.cat([B, B], dim=1)).cpu().numpy()
        assert same(live.cpu().numpy(), twice)
        xs.close()
    plan.set_frame_pairing(False)


@pytest.mark.parametrize("N,H", SHAPES)
def test_delay_equals_derive_irfft_peak(pkg, torch_cuda, N, H):
    torch = torch_cuda
    plan, bins, P = plan_of(pkg, N, H), N // 2 + 1, 5
    A, B = device_spectra(torch, plan, N, H, P)
    xs = pkg.CrossSpectrum(plan, P)
    state = xs.accumulate(A, B, carry=True)
    for wt in (pkg.XSPEC_PHAT, pkg.XSPEC_NONE):
        for m in (1, 40, N // 2 - 1):
            cc = plan.irfft(xs.weighted(None, wt))
            want = xs.peak(cc, m).cpu().numpy()
            buf = torch.full((P + 1, 5), -7.0, device="cuda")
            got = xs.delay(None, wt, m, out=buf[:P, :3])
            torch.cuda.synchronize()
            assert same(got.cpu().numpy(), want), (wt, m)
            assert bool(torch.all(buf[P:] == -7.0)) and bool(torch.all(buf[:, 3:] == -7.0))
            rec = xs.last_launch()
            assert rec["kernels"] == [K_DERIVE, K_PEAK] and rec["grids"] == [P * ((bins + 255) // 256), P]
            assert same(xs.delay(state.clone(), wt, m).cpu().numpy(), want)
            assert same(xs.delay(state[1:3].clone(), wt, m).cpu().numpy(), want[1:3])
    lags = xs.delay().cpu().numpy()[:, 0]
    assert [int(v) for v in lags[[0, 1, 3, 4]]] == [DELAYS[p] for p in (0, 1, 3, 4)]
    xs.close()


@pytest.mark.parametrize("N,H", SHAPES)
def test_hops_of_two_streams_equal_estimate(pkg, torch_cuda, N, H):
    """F = 1 accumulates on Stream.stft_hop rows, hop by hop, equal estimate over the whole
    input (pairing off, DROP), and the delay follows."""
    torch = torch_cuda
    plan, P = plan_of(pkg, N, H), 3
    a, b = signal(N, H, P)
    xa, xb = dev(torch, a), dev(torch, b)
    for alpha in ALPHAS:
        ref = pkg.CrossSpectrum(plan, P, alpha)
        want = ref.estimate(xa, xb).cpu().numpy()
        xs = pkg.CrossSpectrum(plan, P, alpha)
        sa, sb = pkg.Stream(plan, P), pkg.Stream(plan, P)
        done = 0
        for q in range(xa.shape[1] // H):
            ra, ea = sa.stft_hop(xa[:, q * H:(q + 1) * H].contiguous())
            rb, eb = sb.stft_hop(xb[:, q * H:(q + 1) * H].contiguous())
            assert ea == eb
            if ea:
                xs.accumulate(ra[:, None, :], rb[:, None, :], carry=True)
                done += 1
                assert xs.frames == done
        torch.cuda.synchronize()
        assert done == F and same(xs.state().cpu().numpy(), want)
        assert same(xs.delay().cpu().numpy(), ref.delay(dev(torch, want)).cpu().numpy())
        sa.close(), sb.close(), xs.close(), ref.close()


# ------------------------------------------------------------------ 5. arguments and counters
def test_argument_and_counter_errors(pkg, torch_cuda):
    torch = torch_cuda
    N, H, P = 256, 128, 3
    plan, bins, L = plan_of(pkg, N, H), N // 2 + 1, pkg.lib()
    A, B = device_spectra(torch, plan, N, H, P)
    for alpha in (-0.5, 1.0, float("nan")):
        with pytest.raises(ValueError):
            pkg.CrossSpectrum(plan, P, alpha)
    with pytest.raises(ValueError):
        pkg.CrossSpectrum(plan, 0)
    xs = pkg.CrossSpectrum(plan, P, 0.5)
    assert xs.factors == (0.5, 0.5) and xs.frames == 0
    assert xs.last_launch() == {"kernels": [], "names": [], "grids": []}
    st = xs.accumulate(A, B, carry=True)
    assert xs.frames == F
    xs.accumulate(A[:, :0], B[:, :0], carry=True)  # no frames: nothing written, nothing counted
    assert xs.frames == F
    xs.reset()
    assert xs.frames == 0 and bool(torch.all(xs.state() == 0)) and xs.last_launch()["kernels"] == []
    with pytest.raises(ValueError):
        xs.accumulate(A[:2], B[:2], carry=True)  # another pair count
    with pytest.raises(ValueError):
        xs.accumulate(A[:2], B)  # a's pairs differ from b's
    with pytest.raises(ValueError):
        xs.accumulate(A, B, state_out=torch.empty((P, 4, bins + 1), device="cuda"))
    with pytest.raises(ValueError):
        xs.accumulate(A.cpu(), B)
    with pytest.raises(ValueError):
        xs.derive(want=())
    with pytest.raises(ValueError):
        xs.derive(weighting=2)
    with pytest.raises(ValueError):
        xs.derive(torch.zeros((2, 4, bins), device="cuda"), coherence=torch.empty((3, bins), device="cuda"))
    for m in (0, N // 2, -1):
        with pytest.raises(ValueError):
            xs.delay(max_lag=m)
        with pytest.raises(ValueError):
            xs.peak(torch.zeros((P, N), device="cuda"), m)
    with pytest.raises(ValueError):
        xs.peak(torch.zeros((P, N + 1), device="cuda"))
    # the C entries' own checks
    a, b, h, EINVAL = A.data_ptr(), B.data_ptr(), xs._h, pkg.EINVAL
    out = torch.zeros((P, 4, bins), device="cuda")
    o, row = out.data_ptr(), 2 * bins
    ok = (h, a, b, P, F, F * row, row, F * row, row, 0, o, None)
    assert L.crlot_xspec_accumulate(*ok) == pkg.OK

    def acc(**kw):
        names = ("xs", "a", "b", "P", "F", "ld_a", "ldf_a", "ld_b", "ldf_b", "carry", "out", "stream")
        v = dict(zip(names, ok))
        v.update(kw)
        return L.crlot_xspec_accumulate(*[v[n] for n in names])

    assert acc(out=None) == EINVAL          # carry = 0 needs an output
    assert acc(a=None) == EINVAL and acc(b=None) == EINVAL
    assert acc(ldf_a=row - 2) == EINVAL and acc(ldf_b=row + 1) == EINVAL
    assert acc(ld_b=F * row - 2) == EINVAL and acc(ld_a=F * row + 1) == EINVAL
    assert acc(a=a + 4) == EINVAL           # 8-byte alignment
    assert acc(out=a) == EINVAL and acc(out=b + 8) == EINVAL  # overlaps
    assert acc(carry=2) == EINVAL and acc(P=-1) == EINVAL and acc(F=-1) == EINVAL
    assert acc(carry=1, P=2) == EINVAL
    assert acc(P=0) == pkg.OK and acc(F=0) == pkg.OK and acc(P=0, a=None, out=None) == pkg.OK
    assert acc(carry=1, out=None) == pkg.OK and xs.frames == F
    co = torch.zeros((P, bins), device="cuda")
    sp = torch.zeros((P, bins), dtype=torch.complex64, device="cuda")
    c, w = co.data_ptr(), sp.data_ptr()
    assert L.crlot_xspec_derive(h, o, P, 0, c, bins, None, 0, w, row, None) == pkg.OK
    assert L.crlot_xspec_derive(h, o, P, 0, None, 0, None, 0, None, 0, None) == EINVAL
    assert L.crlot_xspec_derive(h, o, P, 2, c, bins, None, 0, None, 0, None) == EINVAL
    assert L.crlot_xspec_derive(h, o, P, 0, c, bins - 1, None, 0, None, 0, None) == EINVAL
    assert L.crlot_xspec_derive(h, o, P, 0, None, 0, w, row + 1, None, 0, None) == EINVAL
    assert L.crlot_xspec_derive(h, o, P, 0, None, 0, w, row, w + 8, row, None) == EINVAL  # outputs overlap
    assert L.crlot_xspec_derive(h, o, P, 0, o, bins, None, 0, None, 0, None) == EINVAL    # output on the state
    assert L.crlot_xspec_derive(h, None, 2, 0, c, bins, None, 0, None, 0, None) == EINVAL  # the object's state: P pairs
    pk = torch.zeros((P, 3), device="cuda")
    ccr = torch.zeros((P, N), device="cuda")
    assert L.crlot_xspec_peak(h, ccr.data_ptr(), N, P, 5, pk.data_ptr(), 3, None) == pkg.OK
    assert L.crlot_xspec_peak(h, ccr.data_ptr(), N, P, N // 2, pk.data_ptr(), 3, None) == EINVAL
    assert L.crlot_xspec_peak(h, ccr.data_ptr(), N - 1, P, 5, pk.data_ptr(), 3, None) == EINVAL
    assert L.crlot_xspec_peak(h, ccr.data_ptr(), N, P, 5, pk.data_ptr(), 2, None) == EINVAL
    assert L.crlot_xspec_peak(h, None, N, P, 5, pk.data_ptr(), 3, None) == EINVAL
    assert L.crlot_xspec_peak(h, ccr.data_ptr(), N, P, 5, ccr.data_ptr(), 3, None) == EINVAL
    assert L.crlot_xspec_delay(h, None, P, 1, 5, None, 3, None) == EINVAL
    assert L.crlot_xspec_delay(h, None, P, 1, 0, pk.data_ptr(), 3, None) == EINVAL
    assert L.crlot_xspec_delay(h, None, P, 3, 5, pk.data_ptr(), 3, None) == EINVAL
    assert L.crlot_xspec_delay(h, None, 2, 1, 5, pk.data_ptr(), 3, None) == EINVAL
    x = torch.zeros((P, R.length(N, H, 4)), device="cuda")
    T = x.shape[1]
    assert L.crlot_xspec_estimate(h, x.data_ptr(), x.data_ptr(), P, T, T, T, 0, None, None) == EINVAL
    assert L.crlot_xspec_estimate(h, x.data_ptr(), x.data_ptr(), P, T, T - 1, T, 0, o, None) == EINVAL
    assert L.crlot_xspec_estimate(h, None, x.data_ptr(), P, T, T, T, 0, o, None) == EINVAL
    assert L.crlot_xspec_estimate(h, x.data_ptr(), x.data_ptr(), 2, T, T, T, 1, None, None) == EINVAL
    assert L.crlot_xspec_estimate(h, x.data_ptr(), x.data_ptr(), P, N - 1, T, T, 0, o, None) == pkg.OK  # no frame
    torch.cuda.synchronize()
    del st
    xs.close()


# ------------------------------------------------------------------ 6. against float64
CPU_BARS = dict(coherence=4e-6, w=1e-6, planes=2e-6)


def _model_errors(pkg, oracle, N, H, a, b, alpha):
    """The float64 model on numpy's FFT of (a, b), and what the float32 restatement on the
    oracle's kiss_fftr spectra of the same input differs from it by."""
    w32 = pkg.window_table(pkg.HANN, N, True)
    w = w32.astype(np.float64)
    s64 = R.accumulate(R.stft(a, N, H, w), R.stft(b, N, H, w), alpha, np.float64)
    k = oracle.KissR(N)
    Fr = (len(a) - N) // H + 1

    def kiss(x):
        return np.stack([k.forward(x[f * H:f * H + N].astype(np.float32) * w32) for f in range(Fr)])

    s32 = R.accumulate(kiss(a), kiss(b), alpha, np.float32)
    return s64, s32


def _differences(s, s64):
    c64, _, w64 = R.derive(s64, R.PHAT, np.float64)
    c, _, w = R.derive(np.asarray(s, np.float32), R.PHAT, np.float32)
    return dict(coherence=float(np.abs(c - c64).max()), w=float(np.abs(w - w64).max()),
                planes=max(float(np.abs(s[j].astype(np.float64) - s64[j]).max() / np.abs(s64[j]).max())
                           for j in range(4)))


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("N,H", SHAPES)
def test_estimate_against_the_float64_model(pkg, oracle, torch_cuda, N, H, alpha):
    torch = torch_cuda
    plan = plan_of(pkg, N, H)
    a, b = R.delayed_pair(R.length(N, H, 24), 5)
    s64, s32 = _model_errors(pkg, oracle, N, H, a, b, alpha)
    xs = pkg.CrossSpectrum(plan, 1, alpha)
    got = xs.estimate(dev(torch, a.astype(np.float32)), dev(torch, b.astype(np.float32))).cpu().numpy()[0]
    xs.close()
    model, device = _differences(s32, s64), _differences(got, s64)
    for k, floor in CPU_BARS.items():
        bar = max(floor, 4 * model[k])
        print(f"xspec-f64 {N}/{H} alpha={alpha} {k}: restatement on kiss_fftr {model[k]:.2e}, bar {bar:.2e}, "
              f"device {device[k]:.2e}")
    for k, floor in CPU_BARS.items():
        assert device[k] <= max(floor, 4 * model[k]), k


@pytest.mark.parametrize("N,H", POW2)
def test_delays_against_the_float64_model(pkg, oracle, torch_cuda, N, H):
    torch = torch_cuda
    plan, m = plan_of(pkg, N, H), N // 2 - 1
    xs = pkg.CrossSpectrum(plan, 1)
    for D in (0, 1, -20, 37, N // 4):
        a, b = R.delayed_pair(R.length(N, H, 24), D)
        s64, s32 = _model_errors(pkg, oracle, N, H, a, b, 0.0)
        want = R.delay(s64, N, R.PHAT, m, np.float64)[0]
        rest = R.delay(s32, N, R.PHAT, m, np.float32)[0]
        st = xs.estimate(dev(torch, a.astype(np.float32)), dev(torch, b.astype(np.float32)))
        got = xs.delay(st, pkg.XSPEC_PHAT, m).cpu().numpy()[0]
        bar = max(1e-5, 4 * abs(float(rest[1]) - float(want[1])))
        print(f"xspec-delay {N}/{H} D={D}: lag {got[0]:.0f} frac {got[1]:+.3e} (float64 {want[1]:+.3e}, restatement "
              f"off by {abs(float(rest[1]) - float(want[1])):.2e}, bar {bar:.2e}, device off by "
              f"{abs(float(got[1]) - float(want[1])):.2e}) peak {got[2]:.4f}")
        assert int(got[0]) == D and int(want[0]) == D
        assert abs(float(got[1]) - float(want[1])) <= bar
    xs.close()


# ------------------------------------------------------------------ 7. behaviour
def test_h1_taps_cancel_the_echo_of_the_same_system(pkg, torch_cuda):
    """H1 from estimate at 512/128 over 60 frames -> irfft -> the first 128 samples as the
    taps of an adaptive filter with adaptation off: over a fresh stretch of the same system
    the error energy is 30 dB or more below the zero-taps run.  The model's tap error
    (<= 5.5e-4 over 128 taps) bounds the residual near -44 dB of |h|^2; the 0.01 noise puts
    the floor near -40 dB."""
    torch = torch_cuda
    N, H, blk = 512, 128, 128
    plan = plan_of(pkg, N, H)
    a, b = R.fir_pair(R.length(N, H, 60))
    xs = pkg.CrossSpectrum(plan, 1)
    xs.estimate(dev(torch, a.astype(np.float32)), dev(torch, b.astype(np.float32)), carry=True)
    assert xs.frames == 60
    h = plan.irfft(xs.transfer()).cpu().numpy()[0]
    assert float(xs.coherence().min()) >= 0.98
    print(f"xspec-h1: taps within {np.abs(h[:8] - R.FIR).max():.2e}, elsewhere {np.abs(h[8:]).max():.2e}")
    fresh_a, fresh_b = R.fir_pair(40 * blk, seed=99)
    energy = {}
    for name, taps in (("zero", np.zeros(blk, np.float32)), ("h1", h[:blk])):
        af = pkg.AdaptiveFilter(blk, blk, 1)
        af.set_taps(taps)
        af.set_adapt(False)
        e = [af.push(dev(torch, fresh_a[None, q * blk:(q + 1) * blk].astype(np.float32)),
                     dev(torch, fresh_b[None, q * blk:(q + 1) * blk].astype(np.float32))).cpu().numpy()
             for q in range(40)]
        energy[name] = float(np.sum(np.concatenate(e, axis=1)[:, blk:].astype(np.float64) ** 2))
        af.close()
    db = 10 * np.log10(energy["h1"] / energy["zero"])
    print(f"xspec-h1: error energy {db:.1f} dB against the zero-taps run")
    assert db <= -30.0
    xs.close()
