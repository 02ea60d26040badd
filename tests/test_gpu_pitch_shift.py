"""GPU tests of crlot_pitch_shift (include/crlot_dsp.h, "resample / pitch shift"):
by definition resample(time_stretch(x, U / D)) cropped or zero-filled to T, bit
for bit, whatever the slicing; a tone moves by the ratio and keeps its length."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_plans = {}


def plan_for(pkg, n, h):
    if (n, h) not in _plans:
        _plans[(n, h)] = pkg.Plan(frame_size=n, hop_size=h)
    return _plans[(n, h)]


def composed(torch, plan, r, x):
    """resample(time_stretch(x)) through the two public entries, fixed to T samples."""
    S, T = x.shape
    z = plan.time_stretch(x, r.up / r.down)
    w = r.resample(z)
    want = torch.zeros((S, T), device="cuda")
    m = min(w.shape[1], T)
    want[:, :m] = w[:, :m]
    torch.cuda.synchronize()
    return want, z.shape[1], w.shape[1]


@pytest.mark.parametrize("n,h", [(1024, 256), (960, 240), (4096, 1024)])
def test_pitch_shift_is_the_composition(pkg, torch_cuda, n, h):
    torch = torch_cuda
    S, T = 3, 20000
    plan = plan_for(pkg, n, h)
    x = torch.from_numpy(np.random.default_rng(n).standard_normal((S, T)).astype(np.float32)).cuda()
    for up, down in ((89, 84), (84, 89), (2, 1)):
        r = pkg.Resampler(up, down)
        want, Ls, L = composed(torch, plan, r, x)
        assert Ls == plan.stretch_output_length(T, up / down) and L == r.output_length(Ls)
        got = torch.full((S, T + 5), float("nan"), device="cuda")  # (a padded output: the gaps stay untouched)
        plan.pitch_shift(x, r, y=got[:, :T])
        torch.cuda.synchronize()
        rec = plan.last_launch()
        assert rec["kernels"][-1] == "k_resample_phase" and "k_phase_voc" in rec["kernels"][:-1], rec
        assert bool(torch.isnan(got[:, T:]).all())
        out = got[:, :T].contiguous()
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.1
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (up, down)
        if L < T:  # fix_length's tail is +0
            assert bool((out[:, L:].view(torch.int32) == 0).all())
        one = plan.pitch_shift(x[1], r)  # a stream alone, 1-d
        torch.cuda.synchronize()
        assert one.shape == (T,) and torch.equal(one.view(torch.int32), want[1].view(torch.int32))
        r.close()


def test_pitch_shift_with_a_stored_mask(pkg, torch_cuda):
    torch = torch_cuda
    n, h, S, T = 1024, 256, 3, 20000
    plan = plan_for(pkg, n, h)
    r = pkg.Resampler(84, 89)
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn((S, T), device="cuda", generator=g)
    Fp = pkg.stretch_frame_count(plan.frame_count(T), 84 / 89)
    plan.set_spectral_mask(torch.rand((S, Fp, n // 2 + 1), device="cuda", generator=g))
    try:
        want, _, _ = composed(torch, plan, r, x)
        got = plan.pitch_shift(x, r)
        torch.cuda.synchronize()
        plan.set_spectral_mask(torch.ones((Fp - 1, n // 2 + 1), device="cuda"))  # too few rows for F'
        with pytest.raises(ValueError):
            plan.pitch_shift(x, r)
    finally:
        plan.set_spectral_mask(None)
    unmasked = plan.pitch_shift(x, r)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(got, unmasked)


def test_pitch_shift_in_two_slices(pkg, torch_cuda):
    """test_time_stretch_in_two_slices' shape: 4096 / 1024, S = 64, T = 131 072, ratio
    1 / 2 (rate 0.5): F = 128, F' = 256, z = 262 144 samples.  Per stream
    (128 + 256) x 4098 x 4 + 262 144 x 4 = 7 343 104 bytes; 2^28 // 7 343 104 = 36
    streams per slice: slices of 36 and 28.  Each half of the batch alone is one
    slice."""
    torch = torch_cuda
    n, h, S, T = 4096, 1024, 64, 131072
    plan = plan_for(pkg, n, h)
    r = pkg.Resampler(1, 2)
    x = torch.randn((S, T), device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    F = plan.frame_count(T)
    Fp = pkg.stretch_frame_count(F, 0.5)
    assert (F, Fp) == (128, 256) and (1 << 28) // (((F + Fp) * (n + 2) + Fp * h) * 4) == 36
    halves = torch.cat([plan.pitch_shift(x[:32], r), plan.pitch_shift(x[32:], r)])
    try:
        plan.set_chunks(2)  # (the vocoder's grid then tells the slice: 28 streams x 33 column blocks x 2 chunks)
        got = plan.pitch_shift(x, r)
        torch.cuda.synchronize()
        rec = plan.last_launch()
    finally:
        plan.set_chunks(0)
    assert got.shape == (S, T)
    assert torch.equal(got.view(torch.int32), halves.view(torch.int32))
    k = rec["kernels"].index("k_phase_voc")
    assert rec["grid"][k] == (28 * 33 * 2 + 3) // 4, rec
    assert rec["kernels"][-1] == "k_resample_phase"
    want, _, _ = composed(torch, plan, r, x[40:43])
    assert torch.equal(got[40:43].view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("semitones", (12, -12, 1))
def test_tone_moves_by_the_ratio(pkg, torch_cuda, semitones):
    """440 Hz at 44.1 kHz shifted by +12, -12 and +1 semitones peaks at 440 rho, rho
    the rational the binding builds (2, 1/2, 196/185), within one bin of the 4096-point
    spectrum test_sinusoid_keeps_its_pitch uses, and has length T."""
    torch = torch_cuda
    n, h, T, sr = 1024, 256, 32768, 44100.0
    plan = plan_for(pkg, n, h)
    num, den = pkg.rational_approx(2.0 ** (semitones / 12.0), 256)
    assert (num, den) == {12: (2, 1), -12: (1, 2), 1: (196, 185)}[semitones]
    x = np.sin(2 * np.pi * 440.0 / sr * np.arange(T)).astype(np.float32)
    y = plan.pitch_shift(torch.from_numpy(x).cuda(), semitones=semitones)
    torch.cuda.synchronize()
    assert y.shape == (T,)
    y = y.cpu().numpy()
    mid = y[T // 2 - 2048:T // 2 + 2048]
    spec = np.abs(np.fft.rfft(mid * np.hanning(4096)))
    want_bin = 440.0 * num / den / sr * 4096
    assert abs(int(np.argmax(spec)) - want_bin) <= 1.0, (int(np.argmax(spec)), want_bin)
    assert np.abs(mid).max() > 0.5
    assert plan.pitch_shift(torch.from_numpy(x).cuda(), semitones=semitones) is not None  # (the cached resampler)
    assert len(plan._pitch_resamplers) >= 1


def test_refusals(pkg, torch_cuda):
    torch = torch_cuda
    L = pkg.lib()
    plan = plan_for(pkg, 1024, 256)
    x = torch.zeros((2, 4096), device="cuda")
    y = torch.zeros((2, 4096), device="cuda")
    # a rate outside time stretch's [1/64, 64] cannot be built: the resampler's own limit is the same
    for up, down in ((65, 1), (1, 65)):
        with pytest.raises(ValueError):
            pkg.Resampler(up, down)
    edge = pkg.Resampler(64, 1, zeros=2)  # rate 64: allowed
    assert plan.pitch_shift(x, edge).shape == (2, 4096)
    torch.cuda.synchronize()
    # a resampler on another device (created without touching it)
    other = pkg.Resampler(89, 84, device=1)
    with pytest.raises(ValueError):
        plan.pitch_shift(x, other)
    assert L.crlot_pitch_shift(plan._h, other._h, x.data_ptr(), y.data_ptr(), 2, 4096, 4096, 4096, None) == pkg.EINVAL
    r = pkg.Resampler(89, 84)

    def call(px, py, nst, t, ld_x, ld_y):
        return L.crlot_pitch_shift(plan._h, r._h, px, py, nst, t, ld_x, ld_y, None)

    assert call(x.data_ptr(), y.data_ptr(), 2, 4096, 4096, 4096) == pkg.OK
    assert call(x.data_ptr(), y.data_ptr(), 2, 4096, 4095, 4096) == pkg.EINVAL  # ld_x < T
    assert call(x.data_ptr(), y.data_ptr(), 2, 4096, 4096, 4095) == pkg.EINVAL  # ld_y < T
    assert call(x.data_ptr(), x.data_ptr(), 2, 4096, 4096, 4096) == pkg.EINVAL  # overlap
    assert call(None, None, 2, 4096, 4096, 4096) == pkg.EINVAL
    guard = torch.full((2, 4096), 7.0, device="cuda")
    assert call(x.data_ptr(), guard.data_ptr(), 0, 4096, 4096, 4096) == pkg.OK
    assert call(x.data_ptr(), guard.data_ptr(), 2, 0, 4096, 4096) == pkg.OK
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    # a signal too short for a frame has no stretch: all of fix_length's zeros
    short = plan.pitch_shift(torch.ones((2, 100), device="cuda"), r)
    torch.cuda.synchronize()
    assert short.shape == (2, 100)
    if plan.frame_count(100) == 0:
        assert bool((short.view(torch.int32) == 0).all())
