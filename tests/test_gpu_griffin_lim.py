"""GPU tests of Griffin-Lim (include/crlot_dsp.h, "Griffin-Lim"): crlot_gl_project
against the numpy float32 restatement of its contract, bit for bit;
crlot_griffin_lim equal to the loop over crlot_istft_ola / crlot_stft /
crlot_gl_project, bit for bit, at the fused shapes (one k_gl_iter per iteration,
whatever the pairing setting) and at the staged ones; output bits independent of
chunking, batch, leading dimensions, the alignment of y and slicing; convergence on
the device by the same two conditions as the float64 recurrence and in agreement
with it; memory containment; errors and empties.

The convergence tests run on plans whose norm table is the least-squares one
(tests/griffin_lim_reference.py, "The norm table").
"""
import functools

import numpy as np
import pytest

import griffin_lim_reference as GL

pytestmark = pytest.mark.gpu

S_FIX, F_FIX, N_ITER = 3, GL.F_SIGNAL, 3
FUSED = [(256, 128), (512, 128), (1024, 256), (1024, 1024)]
STAGED = [(1024, 384), (960, 240), (2048, 512), (4096, 1024)]

# The largest relative gap |SC_device - SC_f64| / SC_f64 seen on MI355X between the
# library's float32 recurrence and griffin_lim_f64 over test_convergence_on_device's
# cases was SC_GAP_MEASURED; the bar is 4 x that.
SC_GAP_MEASURED = 9.12e-07
SC_GAP_BAR = 4.0 * SC_GAP_MEASURED

_plans = {}


def plan_for(pkg, n, h, pairing=True, ls=False):
    key = (n, h, pairing, ls)
    if key not in _plans:
        p = pkg.Plan(frame_size=n, hop_size=h, frame_pairing=pairing)
        if ls:
            p.upload_tables(norm=GL.ls_norm32(n, h))
        _plans[key] = p
    return _plans[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def fixture_np(n, h, S=S_FIX):
    """(mag (S, F, bins) float32, init (S, F, bins) complex64) of S seeded test signals."""
    mag = np.stack([GL.target_mag(GL.make_signal(n, h, seed), n, h) for seed in range(S)])
    init = GL.random_phase_init(mag.shape, seed=n + h)
    mag.setflags(write=False)
    init.setflags(write=False)
    return mag, init


def fixture(torch, n, h, S=S_FIX):
    mag, init = fixture_np(n, h, S)
    return torch.from_numpy(mag.copy()).cuda(), torch.from_numpy(init.copy()).cuda()


def first_spectrum(torch, plan, mag, init):
    return torch.complex(mag, torch.zeros_like(mag)) if init is None else plan.gl_project(init, mag)


def compose(torch, plan, mag, n_iter, momentum, init=None):
    """The definition: the loop a user writes on the three public entries."""
    y = plan.istft_ola(first_spectrum(torch, plan, mag, init))
    tprev = None
    for _ in range(n_iter):
        X = plan.stft(y)
        y = plan.istft_ola(plan.gl_project(X, mag, tprev if momentum > 0 else None, momentum))
        tprev = X
    torch.cuda.synchronize()
    return y


# ------------------------------------------------------------------ 1. the projection
def project_inputs(N, S=3, F=5):
    bins = N // 2 + 1
    rng = np.random.default_rng(N)
    X = (rng.standard_normal((S, F, bins)) + 1j * rng.standard_normal((S, F, bins))).astype(np.complex64)
    T = (rng.standard_normal((S, F, bins)) + 1j * rng.standard_normal((S, F, bins))).astype(np.complex64)
    mag = np.abs(rng.standard_normal((S, F, bins))).astype(np.float32)
    X[0, 0, 3:9] = 0
    T[0, 1, 3:9] = 0
    X[0, 2, 5] = np.nan + 1j
    X[0, 2, 6] = 1 + 1j * np.inf
    T[0, 2, 7] = -np.inf
    X[0, 2, 8] = 1e-31 + 1e-31j          # below the sanitize threshold
    mag[0, 3, 4] = np.nan
    mag[0, 3, 5] = np.inf
    X[1, :, 10] *= np.float32(1e-12)     # a quiet column
    T[1, :, 10] *= np.float32(1e-12)
    X[1, 2] *= np.float32(1e12)          # a loud frame
    T[1, 2] *= np.float32(1e12)
    mag[2, 1] = -mag[2, 1]               # negative magnitudes are used as they are
    mag[2, 3] = 0                        # a zero row
    X.imag[2, :, 0] = 0.5                # bins 0 and N/2: imaginary parts are ignored
    T.imag[2, :, -1] = -0.5
    return X, T, mag


@pytest.mark.parametrize("N", [256, 1024, 960])
def test_gl_project_matches_float32_restatement(pkg, torch_cuda, N):
    torch = torch_cuda
    S, F, bins = 3, 5, N // 2 + 1
    plan = plan_for(pkg, N, N // 4)
    X, T, mag = project_inputs(N, S, F)
    dX, dT, dm = (torch.from_numpy(a).cuda() for a in (X, T, mag))
    for momentum in (0.0, 0.5, 0.99):
        for Tn, Td in ((None, None), (T, dT)):
            want = GL.project32(X, mag, Tn, momentum)
            assert np.all(np.isfinite(want.view(np.float32)))
            got = plan.gl_project(dX, dm, Td, momentum)
            torch.cuda.synchronize()
            assert plan.last_launch()["kernels"] == ["k_gl_project"]
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (momentum, Tn is not None)
    # padded leading dimensions on every operand, NaN in the padding
    want = GL.project32(X, mag, T, 0.99)

    def padded(src, pf, pb, dtype_complex):
        shape = (S, F + pf, bins + pb) + ((2,) if dtype_complex else ())
        big = torch.full(shape, float("nan"), device="cuda")
        big = torch.view_as_complex(big) if dtype_complex else big
        view = big[:, :F, :bins]
        view.copy_(src)
        return big, view

    _, pX = padded(dX, 2, 3, True)
    _, pT = padded(dT, 1, 5, True)
    _, pm = padded(dm, 3, 7, False)
    big_out, pout = padded(torch.zeros_like(dX), 2, 1, True)
    got = plan.gl_project(pX, pm, pT, 0.99, out=pout)
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert bool(torch.isnan(torch.view_as_real(big_out[:, F:])).all())
    assert bool(torch.isnan(torch.view_as_real(big_out[:, :, bins:])).all())
    # in place
    work = dX.clone()
    assert plan.gl_project(work, dm, dT, 0.99, out=work) is work
    torch.cuda.synchronize()
    assert np.array_equal(bits(work.cpu().numpy()), bits(want))
    # any other overlap of out with an input is refused
    with pytest.raises(ValueError):
        plan.gl_project(dX, dm, dT, 0.99, out=dT)
    flat = torch.view_as_complex(torch.zeros((S * F * bins + bins, 2), device="cuda"))
    with pytest.raises(ValueError):
        plan.gl_project(flat[:S * F * bins].view(S, F, bins), dm, None, 0.0, out=flat[bins:].view(S, F, bins))


# ------------------------------------------------------------------ 2. the composition
@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("n,h", FUSED)
def test_fused_shapes_are_the_pairing_off_composition(pkg, torch_cuda, n, h, momentum, with_init):
    torch = torch_cuda
    mag, init = fixture(torch, n, h)
    init = init if with_init else None
    off, on = plan_for(pkg, n, h, False), plan_for(pkg, n, h, True)
    want = compose(torch, off, mag, N_ITER, momentum, init)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.05
    for plan in (off, on):
        got = plan.griffin_lim(mag, N_ITER, momentum, init)
        torch.cuda.synchronize()
        rec = plan.last_launch()
        assert rec["kernels"] == ["k_gl_iter"], rec
        assert got.shape == (S_FIX, F_FIX * h)
        assert same_bits(torch, got, want), ("pairing", plan is on)
    # n_iter = 0 is istft_ola(S_0)
    y0 = off.istft_ola(first_spectrum(torch, off, mag, init))
    for plan in (off, on):
        got = plan.griffin_lim(mag, 0, momentum, init)
        torch.cuda.synchronize()
        assert "k_gl_iter" not in plan.last_launch()["kernels"]
        assert same_bits(torch, got, y0)


@pytest.mark.parametrize("pairing", [False, True])
@pytest.mark.parametrize("n,h", STAGED)
def test_staged_shapes_are_the_composition(pkg, torch_cuda, n, h, pairing):
    torch = torch_cuda
    mag, init0 = fixture(torch, n, h)
    plan = plan_for(pkg, n, h, pairing)
    for momentum in (0.0, 0.99):
        for init in (None, init0):
            want = compose(torch, plan, mag, N_ITER, momentum, init)
            assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.05
            got = plan.griffin_lim(mag, N_ITER, momentum, init)
            torch.cuda.synchronize()
            rec = plan.last_launch()
            assert "k_gl_project" in rec["kernels"] and "k_gl_iter" not in rec["kernels"], rec
            assert same_bits(torch, got, want), (momentum, init is not None)
    got = plan.griffin_lim(mag, 0, 0.99, init0)
    torch.cuda.synchronize()
    assert same_bits(torch, got, plan.istft_ola(first_spectrum(torch, plan, mag, init0)))


@pytest.mark.parametrize("pairing", [False, True])
@pytest.mark.parametrize("h", [128, 512])
def test_1024_with_momentum_is_routed_by_measurement(pkg, torch_cuda, h, pairing):
    """N = 1024 at H = 128 and 512: one k_gl_iter per iteration without momentum;
    with momentum the staged iteration (the walk measured slower), equal to
    the composition under the plan's own pairing setting."""
    torch = torch_cuda
    n = 1024
    mag, init = fixture(torch, n, h)
    plan, off = plan_for(pkg, n, h, pairing), plan_for(pkg, n, h, False)
    got = plan.griffin_lim(mag, N_ITER, 0.0, init)
    torch.cuda.synchronize()
    assert plan.last_launch()["kernels"] == ["k_gl_iter"]
    assert same_bits(torch, got, compose(torch, off, mag, N_ITER, 0.0, init))
    got = plan.griffin_lim(mag, N_ITER, 0.99, init)
    torch.cuda.synchronize()
    rec = plan.last_launch()
    assert "k_gl_project" in rec["kernels"] and "k_gl_iter" not in rec["kernels"], rec
    assert same_bits(torch, got, compose(torch, plan, mag, N_ITER, 0.99, init))


# ------------------------------------------------------------------ 3. chunking, batch, layout
@pytest.mark.parametrize("n,h", [(512, 128), (1024, 256), (960, 240)])
def test_bits_do_not_depend_on_chunks_batch_or_layout(pkg, torch_cuda, n, h):
    torch = torch_cuda
    bins, L = n // 2 + 1, F_FIX * h
    mag, init = fixture(torch, n, h)
    plan = plan_for(pkg, n, h)
    fused = (n, h) in FUSED
    for momentum in (0.0, 0.99):
        want = plan.griffin_lim(mag, N_ITER, momentum, init)
        torch.cuda.synchronize()
        if fused:  # the chunk seams move, the bits do not
            seen = set()
            try:
                for knob in (1, 2, 3, 7):
                    plan.set_chunks(knob)
                    got = plan.griffin_lim(mag, N_ITER, momentum, init)
                    torch.cuda.synchronize()
                    rec = plan.last_launch()
                    m = -(-F_FIX // knob)
                    assert rec["kernels"] == ["k_gl_iter"] and rec["n_chunks"] == -(-F_FIX // m), rec
                    seen.add(rec["n_chunks"])
                    assert same_bits(torch, got, want), knob
            finally:
                plan.set_chunks(0)
            assert len(seen) == 4
        # one stream alone against its place in the batch
        one = plan.griffin_lim(mag[0:1], N_ITER, momentum, init[0:1])
        assert same_bits(torch, one, want[0:1])
        mid = plan.griffin_lim(mag[1], N_ITER, momentum, init[1])
        assert mid.shape == (L,) and same_bits(torch, mid, want[1])
        # padded leading dimensions of mag, init and y
        big_m = torch.full((S_FIX, F_FIX + 2, bins + 5), float("nan"), device="cuda")
        big_i = torch.view_as_complex(torch.full((S_FIX, F_FIX + 1, bins + 3, 2), float("nan"), device="cuda"))
        big_y = torch.full((S_FIX, L + 10), -7.25, device="cuda")
        pm, pi = big_m[:, :F_FIX, :bins], big_i[:, :F_FIX, :bins]
        pm.copy_(mag)
        pi.copy_(init)
        got = plan.griffin_lim(pm, N_ITER, momentum, pi, y=big_y)
        torch.cuda.synchronize()
        assert got is big_y and same_bits(torch, big_y[:, :L], want)
        assert bool((big_y[:, L:] == -7.25).all())
        # y rows that are 4-byte aligned only (odd offset, odd leading dimension)
        flat = torch.full((S_FIX * (L + 3) + 8,), -7.25, device="cuda")
        odd = flat[1:1 + S_FIX * (L + 3)].view(S_FIX, L + 3)
        assert odd.data_ptr() % 8 == 4
        got = plan.griffin_lim(mag, N_ITER, momentum, init, y=odd)
        torch.cuda.synchronize()
        assert same_bits(torch, odd[:, :L], want)
        assert bool((odd[:, L:] == -7.25).all()) and float(flat[0]) == -7.25 and bool((flat[-7:] == -7.25).all())


@pytest.mark.parametrize("n,h,pairing,n_iter", [(256, 128, True, 0), (512, 128, True, 0), (1024, 256, True, 0),
                                                (1024, 256, True, N_ITER), (2048, 512, False, N_ITER),
                                                (4096, 1024, False, 0), (960, 240, True, N_ITER)])
def test_one_stream_with_an_odd_leading_dimension(pkg, torch_cuda, n, h, pairing, n_iter):
    """The C entry with n_streams = 1, 8-byte aligned y and an odd ld_y (the Python
    binding always passes F H there): ld_y is not read, the bits are the batch's."""
    torch = torch_cuda
    bins, L = n // 2 + 1, F_FIX * h
    mag, init = fixture(torch, n, h)
    plan, lib = plan_for(pkg, n, h, pairing), pkg.lib()
    want = plan.griffin_lim(mag, n_iter, 0.99, init)
    y = torch.full((L + 16,), -7.25, device="cuda")
    assert y.data_ptr() % 8 == 0
    rc = lib.crlot_griffin_lim(plan._h, mag[0].data_ptr(), F_FIX * bins, bins, init[0].data_ptr(), 2 * F_FIX * bins,
                               2 * bins, y.data_ptr(), L + 3, 1, F_FIX, n_iter, 0.99, plan._cur_stream())
    assert rc == 0, lib.crlot_last_error()
    torch.cuda.synchronize()
    assert same_bits(torch, y[:L], want[0]) and bool((y[L:] == -7.25).all())


# ------------------------------------------------------------------ 4. slices
def test_griffin_lim_in_two_slices(pkg, torch_cuda):
    """4096 / 1024, F = 24, momentum 0.99, frame pairs (no staged frames): per stream
    two y rows of 24 576 floats and three spectra of 24 x 4098 floats, 1 376 832
    bytes; 268 435 456 // 1 376 832 = 194 streams per slice, so S = 200 runs as
    slices of 194 and 6 streams.  Equal to the unsliced composition per stream."""
    torch = torch_cuda
    n, h, S, F = 4096, 1024, 200, F_FIX
    bins = n // 2 + 1
    assert (1 << 28) // ((2 * F * h + 3 * F * (n + 2)) * 4) == 194
    plan = plan_for(pkg, n, h)
    g = torch.Generator(device="cuda").manual_seed(5)
    mag3, init3 = fixture(torch, n, h)
    mag = mag3[torch.arange(S, device="cuda") % S_FIX] * (0.5 + torch.rand((S, 1, 1), device="cuda", generator=g))
    init = init3[torch.arange(S, device="cuda") % S_FIX].contiguous()
    got = plan.griffin_lim(mag, 2, 0.99, init)
    torch.cuda.synchronize()
    rec = plan.last_launch()
    k = rec["kernels"].index("k_gl_project")
    assert rec["grid"][k] == 6 * F * -(-bins // 256), rec  # the last slice's 6 streams
    assert got.shape == (S, F * h) and bool(torch.isfinite(got).all())
    for s0 in (0, 96, 192, 198):  # composed in small batches: both slices and their seam
        want = compose(torch, plan, mag[s0:s0 + 2], 2, 0.99, init[s0:s0 + 2])
        assert same_bits(torch, got[s0:s0 + 2], want), s0


# ------------------------------------------------------------------ 5. convergence on the device
@functools.lru_cache(maxsize=None)
def f64_sc(n, h, seed, n_iter, momentum):
    mag, init = fixture_np(n, h, 2)
    y = GL.griffin_lim_f64(mag[seed], n, h, n_iter, momentum, init[seed], ls=True)
    return GL.spectral_convergence(y, mag[seed], n, h)


@pytest.mark.parametrize("n,h", [(256, 128), (1024, 256)])
def test_convergence_on_device(pkg, torch_cuda, n, h):
    torch = torch_cuda
    S = 2
    mag_np, _ = fixture_np(n, h, S)
    mag, init = fixture(torch, n, h, S)
    plan = plan_for(pkg, n, h, ls=True)
    worst_gap = 0.0
    for momentum in (0.0, 0.99):
        sc = {}
        for n_iter in (0, 1, 8, 32):
            y = plan.griffin_lim(mag, n_iter, momentum, init)
            torch.cuda.synchronize()
            y = y.cpu().numpy()
            assert np.all(np.isfinite(y))
            sc[n_iter] = [GL.spectral_convergence(y[s], mag_np[s], n, h) for s in range(S)]
        for s in range(S):
            dev = [sc[k][s] for k in (0, 1, 8, 32)]
            ref = [f64_sc(n, h, s, k, momentum) for k in (0, 1, 8, 32)]
            gaps = [abs(d - r) / r for d, r in zip(dev, ref)]
            worst_gap = max(worst_gap, max(gaps))
            print(f"{n}/{h} momentum {momentum} stream {s}: SC device " + " ".join(f"{v:.5f}" for v in dev) +
                  " | float64 " + " ".join(f"{v:.5f}" for v in ref) + f" | largest gap {max(gaps):.3g}")
            if momentum == 0.0:  # Griffin and Lim: never increases
                assert dev[0] >= dev[1] >= dev[2] >= dev[3], dev
            else:
                assert dev[3] <= 0.25 * dev[0], dev
            for k, gap in zip((0, 1, 8, 32), gaps):
                assert gap <= SC_GAP_BAR, (momentum, s, k, gap)
    print(f"{n}/{h}: largest relative SC gap {worst_gap:.3g} (bar {SC_GAP_BAR:.3g})")


# ------------------------------------------------------------------ 6. containment
@pytest.mark.parametrize("n,h", [(512, 128), (960, 240)])
def test_containment(pkg, torch_cuda, n, h):
    """All operands in one flat allocation: NaN guards in front of, between and
    behind the magnitude and init rows, sentinel guards of N + H floats or more
    around every y row."""
    torch = torch_cuda
    S, F, bins, row = S_FIX, F_FIX, n // 2 + 1, n + 2
    L, G = F * h, n + h + 6
    plan, lib = plan_for(pkg, n, h), pkg.lib()
    mag_np, init_np = fixture_np(n, h)
    mag, init = fixture(torch, n, h)
    tight = plan.griffin_lim(mag, N_ITER, 0.99, init)
    torch.cuda.synchronize()
    tight = tight.cpu().numpy()

    ldf_m, ldf_i = bins + 5, row + 6
    ld_m, ld_i, ld_y = F * ldf_m + G, F * ldf_i + G, L + G
    m_off = G
    i_off = m_off + S * ld_m + G
    i_off += i_off & 1  # (spectra: 8-byte aligned)
    y_off = i_off + S * ld_i + G
    y_off += y_off & 1
    total = y_off + S * ld_y + G
    SENT = np.float32(-7.25)
    flat = np.full(total, np.nan, np.float32)
    flat[y_off - G:] = SENT
    is_y = np.zeros(total, bool)
    init_f = np.ascontiguousarray(init_np).view(np.float32)  # (S, F, row)
    for s in range(S):
        for k in range(F):
            o = m_off + s * ld_m + k * ldf_m
            flat[o:o + bins] = mag_np[s, k]
            o = i_off + s * ld_i + k * ldf_i
            flat[o:o + row] = init_f[s, k]
        is_y[y_off + s * ld_y:y_off + s * ld_y + L] = True
    before = flat.copy()
    buf = torch.from_numpy(flat).cuda()
    base = buf.data_ptr()
    assert (base + 4 * i_off) % 8 == 0
    rc = lib.crlot_griffin_lim(plan._h, base + 4 * m_off, ld_m, ldf_m, base + 4 * i_off, ld_i, ldf_i, base + 4 * y_off,
                               ld_y, S, F, N_ITER, 0.99, plan._cur_stream())
    assert rc == 0, lib.crlot_last_error()
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert np.array_equal(bits(after[~is_y]), bits(before[~is_y]))  # guards and inputs keep their bits
    got = np.stack([after[y_off + s * ld_y:][:L] for s in range(S)])
    assert np.all(np.isfinite(got))
    assert np.array_equal(bits(got), bits(tight))


# ------------------------------------------------------------------ 7. errors and empties
def test_errors(pkg, torch_cuda):
    torch = torch_cuda
    n, h = 512, 128
    mag, init = fixture(torch, n, h)
    lib = pkg.lib()
    gained = pkg.Plan(frame_size=n, hop_size=h)
    gained.set_spectral_gain(np.ones(n // 2 + 1, np.float32))
    with pytest.raises(ValueError, match="gain or a stored mask"):
        gained.griffin_lim(mag, 2, 0.5)
    gained.set_spectral_gain(None)
    gained.griffin_lim(mag, 2, 0.5)
    gained.set_spectral_mask(torch.ones((F_FIX, n // 2 + 1), device="cuda"))
    with pytest.raises(ValueError, match="gain or a stored mask"):
        gained.griffin_lim(mag, 2, 0.5)
    gained.set_spectral_mask(None)
    with pytest.raises(NotImplementedError):
        pkg.Plan(frame_size=n, hop_size=h, boundary_mode=pkg.DROP).griffin_lim(mag, 2, 0.5)
    plan = plan_for(pkg, n, h)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            plan.griffin_lim(mag, 2, bad)
        with pytest.raises(ValueError):
            plan.gl_project(init, mag, None, bad)
    with pytest.raises(ValueError):
        plan.griffin_lim(mag, -1, 0.5)
    # the C entries check for themselves
    y = torch.full((S_FIX, F_FIX * h), -7.25, device="cuda")
    bins, s = n // 2 + 1, plan._cur_stream()

    def call(S=S_FIX, F=F_FIX, n_iter=2, momentum=0.5):
        return lib.crlot_griffin_lim(plan._h, mag.data_ptr(), F_FIX * bins, bins, None, 0, 0, y.data_ptr(), F_FIX * h, S,
                                     F, n_iter, momentum, s)

    for momentum in (1.0, -0.1, float("nan")):
        assert call(momentum=momentum) == pkg.EINVAL
    assert call(n_iter=-1) == pkg.EINVAL and call(n_iter=65537) == pkg.EINVAL
    # F = 0 or S = 0: nothing written
    assert call(F=0) == 0 and call(S=0) == 0
    spec = torch.view_as_real(init)
    assert lib.crlot_gl_project(plan._h, spec.data_ptr(), None, mag.data_ptr(), y.data_ptr(), 0, F_FIX, 0.5,
                                F_FIX * 2 * bins, 2 * bins, 0, 0, F_FIX * bins, bins, F_FIX * 2 * bins, 2 * bins, s) == 0
    torch.cuda.synchronize()
    assert bool((y == -7.25).all())
    assert plan.griffin_lim(torch.zeros((2, 0, bins), device="cuda"), 3, 0.5).shape == (2, 0)


@pytest.mark.parametrize("n,h", [(512, 128), (960, 240)])
def test_zero_magnitudes_give_silence(pkg, torch_cuda, n, h):
    torch = torch_cuda
    mag, init = fixture(torch, n, h)
    mag = mag.clone()
    mag[1] = 0
    plan = plan_for(pkg, n, h)
    for init_ in (None, init):
        y = plan.griffin_lim(mag, N_ITER, 0.99, init_)
        torch.cuda.synchronize()
        assert bool((y[1] == 0).all()) and float(y[0].abs().max()) > 0.05 and bool(torch.isfinite(y).all())
