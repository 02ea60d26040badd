"""GPU tests of the WPE dereverberator (include/crlot_dsp.h, "dereverberation").

Bit for bit (a NaN equals a NaN: the sign and payload of a NaN are the hardware's, every
other value is compared by its bits) against the float32 numpy restatement
(tests/wpe_reference.py) on the device's own crlot_stft rows: power; accumulate at every
extent, through padded leading dimensions and with sentinels around the state output,
carry = 0 leaving the object untouched, a run cut at every frame and carried equal to the
uncut run, each group alone equal to the batch; solve, the zero group included; filter
across chunkings and cuts; rls with its output, Q and taps at every extent, carried from
one extent to the next, and against single-frame calls; dereverb against the hand
composition with frame pairing on and off at 1 and 3 iterations; hop over a run of hops
against stft_hop -> rls -> istft_hop, state included.  Launch records and grids, argument
and counter errors through Python and through C, reset.

Against float64 (the textbook model of tests/wpe_reference.py on the device's own spectra
of the issue's scene, 512/128, M = 2, K = 10, delay 3): the early-signal error of the
device's output is within 1 dB of the model's and the model's improves on the input; the
output, the state planes and Q are within 4 x what the float32 restatement shows against
the model on the CPU (tests/test_wpe_reference.py measures and holds those figures).  Taps
are compared through the output they produce, never directly.

Shapes: 256/128, 512/128, 960/240 (129, 257, 481 bins: the last wave of a group is partly
live) and one case at 1024/256; (M, K, delay) = (1,1,1) (2,3,1) (3,5,3) (4,8,2) (8,8,3); G = 1,
3; F = 1, delay, delay + K, 26 (the stack all zeros, partly zeros, full).  The full cross
product runs at 256/128; the larger shapes take the configurations listed in CASES; every
test that takes a case runs all of CASES.  The hop test runs max(8, delay + K + 2) frames, so
that every ring of delay + K rows wraps.  With
three groups, one stream of group 0 carries a NaN, an Inf and a 1e-38 sample and group 1 is
all zeros.
"""
import ctypes as C

import numpy as np
import pytest

import wpe_reference as W
from wpe_reference import MEASURED

pytestmark = pytest.mark.gpu

F = 26
CONFIGS = [(1, 1, 1), (2, 3, 1), (3, 5, 3), (4, 8, 2), (8, 8, 3)]
CASES = ([(256, 128) + c + (g,) for c in CONFIGS for g in (1, 3)] +
         [(512, 128, 2, 3, 1, 3), (512, 128, 3, 5, 3, 1), (512, 128, 8, 8, 3, 1),
          (960, 240, 1, 1, 1, 3), (960, 240, 3, 5, 3, 3), (960, 240, 4, 8, 2, 1),
          (1024, 256, 4, 8, 2, 1)])
K_POWER, K_ACC, K_SOLVE, K_FILTER, K_GAIN, K_UPDATE, K_STFT_HOP, K_ISTFT_HOP = 64, 65, 66, 67, 68, 69, 55, 56
ALPHA = 0.99


def extents(K, D):
    return sorted({1, D, D + K, F})


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "c":
        a, b = np.ascontiguousarray(a, np.complex64).view(np.float32), np.ascontiguousarray(b, np.complex64).view(np.float32)
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


_inputs, _plans, _spectra, _refs = {}, {}, {}, {}


def signal(N, H, G, M):
    """x (G, M, T) float32, T = N + 25 H: white noise with an echo a few hops back; with three
    groups, one stream of group 0 carries a NaN, an Inf and a 1e-38 sample and group 1 is all
    zeros."""
    key = (N, H, G, M)
    if key not in _inputs:
        T = W.length(N, H, F)
        rng = np.random.default_rng(N + 7 * M + G)
        x = rng.standard_normal((G, M, T + 4 * H))
        x = (x[..., 4 * H:] + 0.5 * x[..., 2 * H:-2 * H] + 0.3 * x[..., :-4 * H]).astype(np.float32)
        if G >= 3:
            m = min(1, M - 1)
            x[0, m, 5], x[0, m, N + 3], x[0, m, 2 * N + 1] = np.nan, np.inf, np.float32(1e-38)
            x[1] = 0.0
        x.setflags(write=False)
        _inputs[key] = x
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
    """(X, Xn): the device's crlot_stft rows (G, M, F, bins) of signal() and their host copy."""
    key = (N, H, G, M)
    if key not in _spectra:
        x = signal(N, H, G, M)
        X = plan_of(pkg, N, H).stft(dev(torch, x.reshape(G * M, -1))).view(G, M, F, N // 2 + 1)
        torch.cuda.synchronize()
        Xn = X.cpu().numpy()
        Xn.setflags(write=False)
        _spectra[key] = (X, Xn)
    return _spectra[key]


def reference(Xn, case):
    """The restatement on the device's rows, computed once per case and shared: the power rows,
    and at every extent the state (carried from the previous extent), the taps and the
    estimate; the RLS run's output, Q and taps at every extent (carried likewise)."""
    if case not in _refs:
        N, H, M, K, D, G = case
        bins, L = N // 2 + 1, M * K
        r = {"iota": W.power(Xn), "state": {}, "taps": {}, "est": {}, "rls": {}}
        S, prev = None, 0
        Q, Gt, outs = W.eye_cov((G,), M, K, bins), np.zeros((G, L, M, bins), np.complex64), []
        for Fe in extents(K, D):
            S = W.accumulate(Xn, r["iota"], K, D, prev, Fe, state=S)
            r["state"][Fe] = S.copy()
            r["taps"][Fe] = W.solve(S, M, K)
            r["est"][Fe] = W.filt(Xn[..., :Fe, :], r["taps"][Fe], K, D)
            o, Q, Gt = W.rls(Xn, Q, Gt, K, D, ALPHA, f0=prev, f1=Fe)
            outs.append(o)
            r["rls"][Fe] = (np.concatenate(outs, axis=-2), Q.copy(), Gt.copy())
            prev = Fe
        _refs[case] = r
    return _refs[case]


def padded(torch, S, fill=-7.0):
    """A copy of spectra (G, M, F, bins) inside a larger buffer: the frame and microphone strides padded."""
    G, M, Fr, bins = S.shape
    buf = torch.full((G, M, Fr + 1, bins + 3), fill, dtype=torch.complex64, device="cuda")
    view = buf[:, :, :Fr, :bins]
    view.copy_(S)
    return view, buf


def fenced(torch, shape, dtype=None, fill=-7.0):
    """A contiguous tensor of `shape` with 64 sentinel elements on either side; returns (view, check)."""
    dtype = dtype or torch.float32
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), fill, dtype=dtype, device="cuda")
    view = buf[64:64 + n].view(*shape)
    return view, lambda: bool(torch.all(buf[:64] == fill)) and bool(torch.all(buf[64 + n:] == fill))


def make(pkg, case, plan=None, **kw):
    N, H, M, K, D, G = case
    return pkg.Dereverberator(plan or plan_of(pkg, N, H), M, taps=K, delay=D, groups=G, alpha=ALPHA, **kw)


def ids(c):
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------ 1. power and accumulate
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_power_and_accumulate_equal_the_restatement(pkg, torch_cuda, case):
    torch = torch_cuda
    N, H, M, K, D, G = case
    bins, L = N // 2 + 1, M * K
    X, Xn = device_spectra(torch, pkg, N, H, G, M)
    ref = reference(Xn, case)
    d = make(pkg, case)
    Xp, _ = padded(torch, X)
    # power: contiguous and padded rows, a sub-run leaves the other rows alone
    io = d.power(X)
    assert d.last_launch()["names"] == ["k_wpe_power"]
    buf = torch.full((G, F + 2, bins + 5), -7.0, device="cuda")
    iop = d.power(Xp, out=buf[:, :F, :bins])
    part = torch.full((G, F, bins), -7.0, device="cuda")
    d.power(X, 3, 11, out=part)
    torch.cuda.synchronize()
    assert same(io.cpu().numpy(), ref["iota"])
    assert same(iop.cpu().numpy(), ref["iota"])
    assert bool(torch.all(buf[:, F:] == -7.0)) and bool(torch.all(buf[:, :, bins:] == -7.0))
    assert same(part[:, 3:11].cpu().numpy(), ref["iota"][:, 3:11])
    assert bool(torch.all(part[:, :3] == -7.0)) and bool(torch.all(part[:, 11:] == -7.0))
    # accumulate at every extent, fenced output, padded inputs; the object stays untouched
    planes = L * L + 2 * L * M
    for Fe in extents(K, D):
        out, fence_ok = fenced(torch, (G, planes, bins))
        d.accumulate(Xp, iop, 0, Fe, state_out=out)
        rec = d.last_launch()
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), ref["state"][Fe]), Fe
        assert fence_ok()
        nt = (L + 3) // 4
        assert rec["names"] == ["k_wpe_acc"]
        assert rec["grids"] == [G * ((bins + 63) // 64) * (nt * (nt + 1) // 2 + nt * ((M + 3) // 4))]
    assert d.frames == 0 and bool(torch.all(d.state() == 0))
    # each group alone equals the batch
    if G > 1:
        for g in range(G):
            alone = d.accumulate(X[g:g + 1], io[g:g + 1])
            torch.cuda.synchronize()
            assert same(alone.cpu().numpy(), ref["state"][F][g:g + 1]), g
    d.close()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_a_cut_at_every_frame_equals_the_uncut_run(pkg, torch_cuda, case):
    torch = torch_cuda
    N, H, M, K, D, G = case
    X, Xn = device_spectra(torch, pkg, N, H, G, M)
    ref = reference(Xn, case)
    io = dev(torch, ref["iota"])
    d = make(pkg, case)
    for cut in range(1, F):
        d.reset()
        d.accumulate(X, io, 0, cut, carry=True)
        assert d.frames == cut
        st = d.accumulate(X, io, cut, F, carry=True)
        torch.cuda.synchronize()
        assert d.frames == F
        assert same(st.cpu().numpy(), ref["state"][F]), cut
    d.close()


# ------------------------------------------------------------------ 2. solve and filter
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_solve_and_filter_equal_the_restatement(pkg, torch_cuda, case):
    torch = torch_cuda
    N, H, M, K, D, G = case
    bins, L = N // 2 + 1, M * K
    X, Xn = device_spectra(torch, pkg, N, H, G, M)
    ref = reference(Xn, case)
    d = make(pkg, case)
    Xp, _ = padded(torch, X)
    for Fe in sorted(ref["taps"]):
        state = dev(torch, ref["state"][Fe])
        taps, fence_ok = fenced(torch, (G, L, M, bins), torch.complex64)
        d.solve(state, taps)
        assert d.last_launch() == {"kernels": [K_SOLVE], "names": ["k_wpe_solve"], "grids": [G * ((bins + 63) // 64)]}
        torch.cuda.synchronize()
        assert same(taps.cpu().numpy(), ref["taps"][Fe]), Fe
        assert fence_ok()
        # the object's own blocks
        d.state().copy_(state)
        d.solve()
        torch.cuda.synchronize()
        assert same(d.taps().cpu().numpy(), ref["taps"][Fe]), Fe
        # the filter over the extent: whole, padded in and out, and in two runs
        est = d.filter(X, taps, 0, Fe)
        assert d.last_launch()["names"] == ["k_wpe_filter"]
        obuf = torch.full((G, M, F + 1, bins + 3), -7.0, dtype=torch.complex64, device="cuda")
        estp = d.filter(Xp, None, 0, Fe, out=obuf[:, :, :F, :bins])
        two = torch.zeros_like(est)
        cut = max(1, Fe // 3)
        d.filter(X, taps, 0, cut, out=two)
        d.filter(X, taps, cut, Fe, out=two)
        torch.cuda.synchronize()
        for got in (est, estp, two):
            assert same(got[:, :, :Fe].cpu().numpy(), ref["est"][Fe]), Fe
        assert bool(torch.all(obuf[:, :, Fe:] == -7.0)) and bool(torch.all(obuf[:, :, :, bins:] == -7.0))
        assert bool(torch.all(est[:, :, Fe:] == 0))
    if G == 3:
        g26 = ref["taps"][F]
        assert np.all(g26[1] == 0) and np.isfinite(g26[2]).all()  # the zero group solves to zero taps
    # zero taps pass the observation through
    d.reset()
    thru = d.filter(X)
    torch.cuda.synchronize()
    assert same(thru.cpu().numpy(), W.filt(Xn, np.zeros((G, L, M, bins), np.complex64), K, D))
    d.close()


# ------------------------------------------------------------------ 3. the recursive step
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_rls_equals_the_restatement_carried_and_frame_by_frame(pkg, torch_cuda, case):
    torch = torch_cuda
    N, H, M, K, D, G = case
    bins, L = N // 2 + 1, M * K
    X, Xn = device_spectra(torch, pkg, N, H, G, M)
    ref = reference(Xn, case)
    a, b = make(pkg, case), make(pkg, case)
    Xp, _ = padded(torch, X)
    out = torch.full((G, M, F + 1, bins + 3), -7.0, dtype=torch.complex64, device="cuda")
    view = out[:, :, :F, :bins]
    prev = 0
    for Fe in extents(K, D):
        a.rls(Xp, prev, Fe, out=view)
        rec = a.last_launch()
        torch.cuda.synchronize()
        want, Q, Gt = ref["rls"][Fe]
        assert same(view[:, :, :Fe].cpu().numpy(), want), Fe
        assert same(a.inv_cov().cpu().numpy(), Q), Fe
        assert same(a.taps().cpu().numpy(), Gt), Fe
        assert a.frames == Fe
        nb = G * ((bins + 63) // 64)
        assert rec == {"kernels": [K_GAIN, K_UPDATE], "names": ["k_wpe_gain", "k_wpe_update"],
                       "grids": [nb * L, nb * (L + M)]}
        prev = Fe
    assert bool(torch.all(out[:, :, F:] == -7.0)) and bool(torch.all(out[:, :, :, bins:] == -7.0))
    single = torch.zeros((G, M, F, bins), dtype=torch.complex64, device="cuda")
    for t in range(F):
        b.rls(X, t, t + 1, out=single)
    torch.cuda.synchronize()
    assert same(single.cpu().numpy(), ref["rls"][F][0])
    assert same(b.inv_cov().cpu().numpy(), ref["rls"][F][1]) and same(b.taps().cpu().numpy(), ref["rls"][F][2])
    # reset: Q the identity, the taps zero, the counter zero
    a.reset()
    assert a.frames == 0 and bool(torch.all(a.taps() == 0)) and bool(torch.all(a.state() == 0))
    assert same(a.inv_cov().cpu().numpy(), W.eye_cov((G,), M, K, bins))
    a.close(), b.close()


# ------------------------------------------------------------------ 4. the composite entry
@pytest.mark.parametrize("pairing", (False, True))
@pytest.mark.parametrize("case", [(256, 128, 2, 3, 1, 3), (512, 128, 3, 5, 3, 1), (960, 240, 4, 8, 2, 1),
                                  (256, 128, 8, 8, 3, 1), (1024, 256, 1, 1, 1, 3)], ids=ids)
def test_dereverb_equals_the_hand_composition(pkg, torch_cuda, case, pairing):
    torch = torch_cuda
    N, H, M, K, D, G = case
    bins = N // 2 + 1
    xd = dev(torch, signal(N, H, G, M))
    for iterations in (1, 3):
        plan = plan_of(pkg, N, H, pairing)
        d = make(pkg, case, plan, iterations=iterations)
        X = plan.stft(xd.view(G * M, -1)).view(G, M, F, bins)
        Z = X
        for _ in range(iterations):
            st = d.accumulate(X, d.power(Z))
            taps = torch.zeros((G, M * K, M, bins), dtype=torch.complex64, device="cuda")
            d.solve(st, taps)
            Z = d.filter(X, taps)
        want = plan.istft_ola(Z.view(G * M, F, bins)).view(G, M, F * H)
        got, fence_ok = fenced(torch, (G, M, F * H))
        d.dereverb(xd, y=got)
        assert d.last_launch()["names"] == ["k_wpe_power", "k_wpe_acc", "k_wpe_solve", "k_wpe_filter"]
        torch.cuda.synchronize()
        assert same(got.cpu().numpy(), want.cpu().numpy()), iterations
        assert fence_ok()
        # the object is untouched
        assert d.frames == 0 and bool(torch.all(d.state() == 0)) and bool(torch.all(d.taps() == 0))
        assert same(d.inv_cov().cpu().numpy(), W.eye_cov((G,), M, K, bins))
        if G == 3:
            gn = got.cpu().numpy()
            assert np.all(gn[1] == 0) and np.isfinite(gn[2]).all()
        d.close()
    plan = plan_of(pkg, N, H, False)
    d = make(pkg, case, plan)
    plan.set_spectral_mask(torch.ones((F, bins), device="cuda"))
    try:
        with pytest.raises(ValueError):
            d.dereverb(xd)
    finally:
        plan.set_spectral_mask(None)
    d.close()


# ------------------------------------------------------------------ 5. the per-hop entry
@pytest.mark.parametrize("case", [(256, 128, 4, 8, 2, 3), (960, 240, 3, 5, 3, 1), (512, 128, 8, 8, 3, 1),
                                  (256, 128, 1, 1, 1, 1)], ids=ids)
def test_hop_equals_stft_hop_rls_istft_hop(pkg, torch_cuda, case):
    torch = torch_cuda
    N, H, M, K, D, G = case
    plan, bins, Cn = plan_of(pkg, N, H), N // 2 + 1, G * M
    frames = max(8, D + K + 2)  # past the ring of D + K rows: frame k lands in row k mod (D + K)
    hops = N // H - 1 + frames
    xd = dev(torch, signal(N, H, G, M).reshape(Cn, -1))
    a, b = make(pkg, case), make(pkg, case)
    sa_in, sa_out = pkg.Stream(plan, Cn), pkg.Stream(plan, Cn)
    sb_in, sb_out = pkg.Stream(plan, Cn), pkg.Stream(plan, Cn)
    lin = torch.zeros((G, M, frames, bins), dtype=torch.complex64, device="cuda")
    pred = torch.zeros_like(lin)
    k = 0
    for q in range(hops):
        hop = xd[:, q * H:(q + 1) * H].contiguous()
        out = torch.full((Cn, H), -7.0, device="cuda")
        got, em = a.hop(sa_in, sa_out, hop, out)
        rec = a.last_launch()
        spec, em_b = sb_in.stft_hop(hop)
        if q < N // H - 1:
            assert em == 0 and em_b == 0 and bool(torch.all(out == -7.0)) and a.frames == 0
            assert rec["kernels"] == [K_STFT_HOP]
            continue
        assert em == H and em_b == 1
        lin[:, :, k].copy_(spec.view(G, M, bins))
        b.rls(lin, k, k + 1, out=pred)
        want = sb_out.istft_hop(pred[:, :, k].reshape(Cn, bins).contiguous())
        torch.cuda.synchronize()
        assert same(got.cpu().numpy(), want.cpu().numpy()), q
        assert same(a.inv_cov().cpu().numpy(), b.inv_cov().cpu().numpy()), q
        assert same(a.taps().cpu().numpy(), b.taps().cpu().numpy()), q
        nb = G * ((bins + 63) // 64)
        assert rec["kernels"] == [K_STFT_HOP, K_GAIN, K_UPDATE, K_ISTFT_HOP]
        assert rec["grids"][1:3] == [nb * M * K, nb * (M * K + M)]
        k += 1
        assert a.frames == k == b.frames
    assert k == frames
    # counters that differ are refused; reset brings all three back
    other = pkg.Stream(plan, Cn)
    with pytest.raises(RuntimeError):
        a.hop(sa_in, other, xd[:, :H].contiguous())
    a.reset(), sa_in.reset(), sa_out.reset()
    assert a.frames == 0 and bool(torch.all(a.taps() == 0))
    _, em = a.hop(sa_in, sa_out, xd[:, :H].contiguous())
    assert em == 0
    for o in (a, b, sa_in, sa_out, sb_in, sb_out, other):
        o.close()


# ------------------------------------------------------------------ 6. arguments
def test_argument_and_counter_errors(pkg, torch_cuda):
    torch = torch_cuda
    N, H, M, K, D, G = 256, 128, 3, 2, 2, 2
    plan, bins, L = plan_of(pkg, N, H), N // 2 + 1, M * K
    planes = L * L + 2 * L * M
    d = pkg.Dereverberator(plan, M, taps=K, delay=D, groups=G)
    X = torch.zeros((G, M, 6, bins), dtype=torch.complex64, device="cuda")
    io = torch.ones((G, 6, bins), device="cuda")
    for bad in (dict(mics=0), dict(mics=9), dict(taps=0), dict(taps=17), dict(mics=8, taps=9), dict(delay=0), dict(delay=9),
                dict(iterations=0), dict(iterations=11), dict(alpha=0.0), dict(alpha=1.5), dict(loading=-1.0),
                dict(floor=0.0), dict(groups=0)):
        kw = dict(mics=M, taps=K, delay=D)
        kw.update(bad)
        with pytest.raises(ValueError):
            pkg.Dereverberator(plan, kw.pop("mics"), **kw)
    with pytest.raises(ValueError):
        d.power(X.cpu())                                    # a host tensor
    with pytest.raises(ValueError):
        d.power(X.to(torch.complex128))                     # dtype
    with pytest.raises(ValueError):
        d.power(X[:, :2])                                   # wrong microphone count
    with pytest.raises(ValueError):
        d.power(X, 4, 3)                                    # f0 > f1
    with pytest.raises(ValueError):
        d.power(X, 0, 7)                                    # f1 past the frames given
    with pytest.raises(ValueError):
        d.accumulate(X, io[:, :5])                          # power rows of another extent
    with pytest.raises(ValueError):
        d.accumulate(X[:1], io[:1], carry=True)             # carry needs the object's groups
    with pytest.raises(ValueError):
        d.accumulate(X, io, state_out=torch.zeros((G, planes - 1, bins), device="cuda"))
    with pytest.raises(ValueError):
        d.solve(torch.zeros((3, planes, bins), device="cuda"), torch.zeros((3, L, M, bins), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        d.solve(torch.zeros((1, planes, bins), device="cuda"))   # the object's taps need G groups
    with pytest.raises(ValueError):
        d.filter(X, out=X)                                  # out overlaps the spectra
    with pytest.raises(ValueError):
        d.rls(X[:1])                                        # rls runs the object's groups
    # through C: the checks the Python layer makes first are the library's too
    Lc = pkg.lib()
    st = torch.zeros((G, planes, bins), device="cuda")
    xp, ip, sp = X.data_ptr(), io.data_ptr(), st.data_ptr()
    ld, ldf = 6 * 2 * bins, 2 * bins
    E = pkg.EINVAL
    assert Lc.crlot_wpe_power(d._h, None, ld, ldf, G, 0, 6, ip, 6 * bins, bins, None) == E
    assert Lc.crlot_wpe_power(d._h, xp, ld, ldf, G, -1, 6, ip, 6 * bins, bins, None) == E
    assert Lc.crlot_wpe_power(d._h, xp, ld - 2, ldf, G, 0, 6, ip, 6 * bins, bins, None) == E      # too small
    assert Lc.crlot_wpe_power(d._h, xp, ld + 1, ldf, G, 0, 6, ip, 6 * bins, bins, None) == E      # odd
    assert Lc.crlot_wpe_power(d._h, xp, ld, ldf, G, 0, 6, ip, 6 * bins, bins - 1, None) == E
    assert Lc.crlot_wpe_power(d._h, xp, ld, ldf, G, 0, 6, xp, 6 * bins, bins, None) == E          # overlap
    assert Lc.crlot_wpe_power(d._h, xp, ld, ldf, 0, 0, 6, ip, 6 * bins, bins, None) == 0          # nothing to do
    assert Lc.crlot_wpe_power(d._h, xp, ld, ldf, G, 3, 3, ip, 6 * bins, bins, None) == 0
    assert Lc.crlot_wpe_accumulate(d._h, xp, ld, ldf, ip, 6 * bins, bins, G, 0, 6, 0, None, None) == E   # carry 0 needs an output
    assert Lc.crlot_wpe_accumulate(d._h, xp, ld, ldf, ip, 6 * bins, bins, G, 0, 6, 2, sp, None) == E
    assert Lc.crlot_wpe_accumulate(d._h, xp, ld, ldf, ip, 6 * bins, bins, 1, 0, 6, 1, sp, None) == E
    assert Lc.crlot_wpe_accumulate(d._h, xp, ld, ldf, ip, 6 * bins, bins, G, 0, 6, 0, xp, None) == E     # overlaps an input
    assert Lc.crlot_wpe_accumulate(d._h, xp, ld, ldf, ip, 6 * bins, bins, G, 0, 6, 1, d.state().data_ptr(), None) == E
    assert Lc.crlot_wpe_solve(d._h, sp, G + 1, d.taps().data_ptr(), None) == E
    assert Lc.crlot_wpe_solve(d._h, sp, G, sp, None) == E                                        # taps overlap the state
    assert Lc.crlot_wpe_solve(d._h, None, 1, None, None) == E
    assert Lc.crlot_wpe_filter(d._h, xp, ld, ldf, None, G, 0, 6, xp, ld, ldf, None) == E
    assert Lc.crlot_wpe_filter(d._h, xp, ld, ldf, None, 1, 0, 6, sp, ld, ldf, None) == E          # the object's taps: G groups
    assert Lc.crlot_wpe_rls(d._h, xp, ld, ldf, 0, 6, xp, ld, ldf, None) == E
    assert Lc.crlot_wpe_rls(d._h, xp, ld, ldf, 0, 6, d.taps().data_ptr(), ld, ldf, None) == E     # overlaps the object's blocks
    assert Lc.crlot_wpe(d._h, xp, 10, sp, 10, G, 1000, None) == E                                # ld_x < T
    torch.cuda.synchronize()
    assert d.frames == 0 and bool(torch.all(d.state() == 0))
    # the per-hop entry's checks
    s_in, s_out = pkg.Stream(plan, G * M), pkg.Stream(plan, G * M)
    hop = torch.zeros((G * M, H), device="cuda")
    other_plan = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True, boundary_mode=pkg.DROP)
    with pytest.raises(ValueError):
        d.hop(s_in, pkg.Stream(plan, G), hop)               # channel counts
    with pytest.raises(ValueError):
        d.hop(s_in, pkg.Stream(other_plan, G * M), hop)     # another plan
    em = C.c_int32(7)
    assert Lc.crlot_stream_wpe_hop(s_in._h, s_in._h, d._h, hop.data_ptr(), hop.data_ptr(), C.byref(em), None) == E
    assert em.value == 0
    whole = pkg.Stream(plan, G * M)
    whole.push_hop(hop)
    with pytest.raises(RuntimeError):
        d.hop(whole, s_out, hop)                            # a stream in whole-hop mode
    d.close()


# ------------------------------------------------------------------ 7. against float64 and behaviour
_scene = {}


def scene(torch, pkg, M):
    """The issue's scene at 512/128: the device's spectra of the microphone signals (G = 1) and
    of the early signals, and the float32 signals."""
    if M not in _scene:
        N, H = 512, 128
        x, e = W.scene(M, early=3 * H)
        plan = plan_of(pkg, N, H)
        T = x.shape[-1]
        Fs = (T - N) // H + 1
        xd = dev(torch, x.astype(np.float32))
        Y = plan.stft(xd).view(1, M, Fs, N // 2 + 1)
        E = plan.stft(dev(torch, e.astype(np.float32)))
        torch.cuda.synchronize()
        _scene[M] = (xd, Y, Y.cpu().numpy(), E.cpu().numpy()[None])
    return _scene[M]


def rel(a, b):
    return float(np.abs(np.asarray(a, np.complex128) - b).max() / np.abs(b).max())


def test_offline_against_the_float64_model_on_the_scene(pkg, torch_cuda):
    torch = torch_cuda
    N, H, M, K, D = 512, 128, 2, 10, 3
    xd, Y, Yn, En = scene(torch, pkg, M)
    L = M * K
    d = pkg.Dereverberator(plan_of(pkg, N, H), M, taps=K, delay=D, iterations=3)
    st = d.accumulate(Y, d.power(Y))
    Z = Y
    for _ in range(3):
        s = d.accumulate(Y, d.power(Z))
        taps = torch.zeros((1, L, M, N // 2 + 1), dtype=torch.complex64, device="cuda")
        d.solve(s, taps)
        Z = d.filter(Y, taps)
    torch.cuda.synchronize()
    Zm = W.model_offline(Yn, K, D, 3)
    R, _ = W.model_stats(Yn, Yn, K, D)
    before, model_db, dev_db = W.error_db(Yn, En), W.error_db(Zm, En), W.error_db(Z.cpu().numpy(), En)
    e_state = rel(W.cov_full(st.cpu().numpy()[..., :L * L, :], L), R)
    e_out = rel(Z.cpu().numpy(), Zm)
    print(f"offline: before {before:.2f} dB, model {model_db:.2f} dB, device {dev_db:.2f} dB; "
          f"state {e_state:.2e}, output {e_out:.2e}")
    assert model_db < before - 3.0
    assert abs(dev_db - model_db) <= 1.0
    assert e_state <= 4 * MEASURED["offline_state"] and e_out <= 4 * MEASURED["offline_out"]
    # the composite entry on the signals is the synthesis of that same estimate
    y = d.dereverb(xd[None])
    want = plan_of(pkg, N, H).istft_ola(Z.view(M, Y.shape[2], N // 2 + 1))
    torch.cuda.synchronize()
    assert same(y.cpu().numpy()[0], want.cpu().numpy())
    d.close()


def test_rls_against_the_float64_model_on_the_scene(pkg, torch_cuda):
    torch = torch_cuda
    N, H, M, K, D, alpha = 512, 128, 2, 10, 3, 0.999
    _, Y, Yn, En = scene(torch, pkg, M)
    L, Fs = M * K, Y.shape[2]
    d = pkg.Dereverberator(plan_of(pkg, N, H), M, taps=K, delay=D, alpha=alpha)
    out = d.rls(Y)
    torch.cuda.synchronize()
    om, Qm, _ = W.model_rls(Yn, K, D, alpha)
    half = slice(Fs // 2, None)
    before, model_db, dev_db = W.error_db(Yn, En, half), W.error_db(om, En, half), W.error_db(out.cpu().numpy(), En, half)
    e_out, e_cov = rel(out.cpu().numpy(), om), rel(W.cov_full(d.inv_cov().cpu().numpy(), L), Qm)
    print(f"rls: before {before:.2f} dB, model {model_db:.2f} dB, device {dev_db:.2f} dB; output {e_out:.2e}, Q {e_cov:.2e}")
    assert model_db < before - 2.0
    assert abs(dev_db - model_db) <= 1.0
    assert e_out <= 4 * MEASURED["rls_out"] and e_cov <= 4 * MEASURED["rls_cov"]
    d.close()
