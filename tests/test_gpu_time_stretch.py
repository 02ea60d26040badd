"""GPU tests of the phase vocoder and the time stretch (include/crlot_dsp.h, "time
stretch"): crlot_phase_vocoder against the float64 torchaudio recurrence, held to
4 x the error of the float32 / uint32 emulation of its contract on the same case
(tests/phase_vocoder_reference.py); a long recurrence whose tail must be as good
as its head; output bits independent of chunking, batch position and leading
dimensions; memory containment; crlot_time_stretch equal to
istft_ola(phase_vocoder(stft(x))) bit for bit, sliced or not; and a sinusoid that
keeps its pitch.

The vocoder's inputs are synthetic float32 spectra, so it is tested apart from
crlot_stft.  Own-scale error: |out - reference| / max(|X[i_t]|, |X[i_t + 1]|) per
element; an element whose two sources are both zero must be exactly 0.
"""
import functools

import numpy as np
import pytest

import phase_vocoder_reference as PV

pytestmark = pytest.mark.gpu

FACTOR = 4.0  # device atan2f / sin / cos may be a few ulp looser than numpy's


@functools.lru_cache(maxsize=None)
def spectra(N, F, S):
    X = PV.spectra(N, F, S)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def emulation_worst(N, F, S, rate):
    X = spectra(N, F, S)
    rel, _ = PV.own_scale_error(PV.emulate(X, rate), X, rate)
    return float(rel.max())


_plans = {}


def plan_for(pkg, n, h=None, pairing=True):
    key = (n, h or n // 4, pairing)
    if key not in _plans:
        _plans[key] = pkg.Plan(frame_size=n, hop_size=key[1], frame_pairing=pairing)
    return _plans[key]


def vocode(torch, plan, X, rate):
    out = plan.phase_vocoder(torch.from_numpy(np.array(X, np.complex64)).cuda(), rate)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("N,F,rate", [(n, 40, r) for n in (256, 1024, 960) for r in PV.RATES] + [(4096, 9, 1.3)])
def test_accuracy_vs_float64(pkg, torch_cuda, N, F, rate):
    S = 3
    X = spectra(N, F, S)
    out = vocode(torch_cuda, plan_for(pkg, N), X, rate)
    assert out.shape == (S, PV.frame_count(F, rate), N // 2 + 1)
    rel, dead = PV.own_scale_error(out, X, rate)
    emu = emulation_worst(N, F, S, rate)
    print(f"N={N} F={F} rate={rate}: device worst {rel.max():.3g}, emulation worst {emu:.3g}")
    assert np.all(np.isfinite(out.view(np.float32)))
    assert np.all(out[dead] == 0)                 # silence (both sources zero) stays exact
    assert np.all(out.imag[..., 0] == 0) and np.all(out.imag[..., -1] == 0)
    assert not np.any(np.signbit(out.imag[..., 0])) and not np.any(np.signbit(out.imag[..., -1]))
    # the quiet column and the loud frame are held to their own scale like the rest
    assert rel.max() <= FACTOR * emu


@pytest.mark.parametrize("rate", (0.75, 2.0))
def test_long_recurrence(pkg, torch_cuda, rate):
    """20 000 frames: the integer accumulator keeps the tail as good as the head."""
    N, F, S = 256, 20000, 1
    X = spectra(N, F, S)
    out = vocode(torch_cuda, plan_for(pkg, N), X, rate)
    rel, dead = PV.own_scale_error(out, X, rate)
    bar = FACTOR * emulation_worst(N, F, S, rate)
    Fp = out.shape[1]
    seg = {"head": rel[:, :50], "middle": rel[:, Fp // 2 - 25:Fp // 2 + 25], "tail": rel[:, -50:]}
    print(f"N={N} F={F} rate={rate}: device worst {rel.max():.3g} " +
          " ".join(f"{k} {v.max():.3g}" for k, v in seg.items()) + f", bar {bar:.3g}")
    assert np.all(out[dead] == 0)
    for name, v in seg.items():
        assert v.max() <= bar, name
    assert rel.max() <= bar


def test_identity_at_rate_one(pkg, torch_cuda):
    N, F, S = 256, 40, 3
    X = spectra(N, F, S)
    re, im = PV.sanitize(X)
    Xs = (re + 1j * im).astype(np.complex128)
    own = np.abs(Xs)

    def worst(out):
        err = np.abs(out.astype(np.complex128) - Xs)
        assert np.all(err[own == 0] == 0)
        return float((err[own > 0] / own[own > 0]).max())

    dev, emu = worst(vocode(torch_cuda, plan_for(pkg, N), X, 1.0)), worst(PV.emulate(X, 1.0))
    print(f"rate 1: device worst {dev:.3g}, emulation worst {emu:.3g}")
    assert dev <= FACTOR * emu


# ------------------------------------------------------------------ bits
def test_bits_do_not_depend_on_chunks(pkg, torch_cuda):
    torch = torch_cuda
    N, F, rate = 256, 2000, 1.3
    plan = plan_for(pkg, N)
    x = torch.from_numpy(np.array(spectra(N, F, 1))).cuda()
    Fp = PV.frame_count(F, rate)
    try:
        plan.set_chunks(0)
        want = plan.phase_vocoder(x, rate)
        torch.cuda.synchronize()
        assert plan.last_launch()["kernels"][-1] == "k_phase_voc"
        for n in (1, 3, 7):
            plan.set_chunks(n)
            got = plan.phase_vocoder(x, rate)
            torch.cuda.synchronize()
            rec = plan.last_launch()
            assert rec["kernels"] == (["k_phase_voc"] if n == 1 else ["k_phase_voc_sums", "k_phase_voc"]), rec
            assert rec["n_chunks"] == n
            assert got.shape == (1, Fp, N // 2 + 1)
            assert torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(want).view(torch.int32)), n
    finally:
        plan.set_chunks(0)


def test_bits_do_not_depend_on_batch_or_leading_dimensions(pkg, torch_cuda):
    torch = torch_cuda
    N, F, rate = 256, 300, 0.75
    bins = N // 2 + 1
    plan = plan_for(pkg, N)
    X5 = np.ascontiguousarray(spectra(N, F, 5))
    one = vocode(torch, plan, X5[2:3], rate)
    batch = vocode(torch, plan, X5, rate)
    assert np.array_equal(bits(batch[2:3]), bits(one))
    assert not np.array_equal(bits(batch[1:2]), bits(one))
    # padded leading dimensions on both sides
    Fp = PV.frame_count(F, rate)
    big_in = torch.view_as_complex(torch.full((5, F + 3, bins + 3, 2), float("nan"), device="cuda"))
    big_out = torch.view_as_complex(torch.full((5, Fp + 2, bins + 5, 2), float("nan"), device="cuda"))
    xin = big_in[:, :F, :bins]
    xin.copy_(torch.from_numpy(X5.copy()))
    got = plan.phase_vocoder(xin, rate, out=big_out[:, :Fp, :bins])
    torch.cuda.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(batch))
    assert bool(torch.isnan(torch.view_as_real(big_out[:, Fp:])).all())
    assert bool(torch.isnan(torch.view_as_real(big_out[:, :, bins:])).all())


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("F,rate,Fp", [(1, 0.5, 2), (2, 0.75, 3), (3, 3.7, 1), (2, 1.0, 2)])
def test_short_inputs(pkg, torch_cuda, F, rate, Fp):
    N, S = 256, 3
    X = np.ascontiguousarray(spectra(N, 40, S)[:, 6:6 + F])
    out = vocode(torch_cuda, plan_for(pkg, N), X, rate)
    assert out.shape == (S, Fp, N // 2 + 1)
    rel, _ = PV.own_scale_error(out, X, rate)
    emu, _ = PV.own_scale_error(PV.emulate(X, rate), X, rate)
    print(f"F={F} rate={rate}: device worst {rel.max():.3g}, emulation worst {emu.max():.3g}")
    assert rel.max() <= FACTOR * emu.max()
    if (F, rate) == (1, 0.5):  # the second frame: half the magnitude at phase 0, exactly
        re, im = PV.sanitize(X)
        assert np.array_equal(bits(out[:, 1].real), bits(PV._m(re, im)[:, 0] * np.float32(0.5)))
        assert np.all(out[:, 1].imag == 0)


def test_empty_calls_write_nothing(pkg, torch_cuda):
    torch = torch_cuda
    N = 256
    plan, L = plan_for(pkg, N), pkg.lib()
    row = N + 2
    src = torch.ones(3 * 4 * row, device="cuda")
    dst = torch.full((3 * 8 * row,), -7.25, device="cuda")
    s = plan._cur_stream()
    assert L.crlot_phase_vocoder(plan._h, src.data_ptr(), dst.data_ptr(), 3, 0, 1.3, 4 * row, row, 8 * row, row, s) == 0
    assert L.crlot_phase_vocoder(plan._h, src.data_ptr(), dst.data_ptr(), 0, 4, 1.3, 4 * row, row, 8 * row, row, s) == 0
    x = torch.ones(3 * 1000, device="cuda")
    assert L.crlot_time_stretch(plan._h, x.data_ptr(), dst.data_ptr(), 0, 1000, 1.3, 1000, 2000, s) == 0
    assert L.crlot_time_stretch(plan._h, x.data_ptr(), dst.data_ptr(), 3, 0, 1.3, 1000, 2000, s) == 0
    torch.cuda.synchronize()
    assert bool((dst == -7.25).all())
    assert plan.phase_vocoder(torch.zeros((3, 0, N // 2 + 1), dtype=torch.complex64, device="cuda"), 1.3).shape == \
        (3, 0, N // 2 + 1)
    # overlapping buffers and bad rates are refused
    assert L.crlot_phase_vocoder(plan._h, src.data_ptr(), src.data_ptr() + 8 * row, 3, 4, 1.0, 4 * row, row, 4 * row,
                                 row, s) == pkg.EINVAL
    assert L.crlot_phase_vocoder(plan._h, src.data_ptr(), dst.data_ptr(), 3, 4, 65.0, 4 * row, row, 8 * row, row,
                                 s) == pkg.EINVAL
    assert L.crlot_phase_vocoder(plan._h, src.data_ptr(), dst.data_ptr(), 3, 4, 1.0, 4 * row, row - 2, 8 * row, row,
                                 s) == pkg.EINVAL


# ------------------------------------------------------------------ containment
@pytest.mark.parametrize("N,rate", [(256, 0.75), (1024, 1.3), (960, 2.0)])
def test_containment(pkg, torch_cuda, N, rate):
    """All operands in one flat allocation: NaN guards in front of, between and
    behind the input rows (right behind frame F - 1, which the last output frames
    must not read), sentinel guards around the output rows."""
    torch = torch_cuda
    S, F = 3, 37
    plan, L = plan_for(pkg, N), pkg.lib()
    row, G = N + 2, N + 2 + 14
    ldf = row + 6
    Fp = PV.frame_count(F, rate)
    X = np.ascontiguousarray(spectra(N, 40, S)[:, :F])
    tight = vocode(torch, plan, X, rate)

    ld_in, ld_out = F * ldf + G, Fp * ldf + G
    in_off, out_off = G, G + S * ld_in + G
    total = out_off + S * ld_out + G
    SENT = np.float32(-7.25)
    flat = np.full(total, np.nan, np.float32)
    flat[out_off - G:] = SENT
    is_in_row = np.zeros(total, bool)
    is_out_row = np.zeros(total, bool)
    Xf = X.view(np.float32)  # (S, F, row)
    for s in range(S):
        for k in range(F):
            o = in_off + s * ld_in + k * ldf
            flat[o:o + row] = Xf[s, k]
            is_in_row[o:o + row] = True
        for k in range(Fp):
            o = out_off + s * ld_out + k * ldf
            is_out_row[o:o + row] = True
    before = flat.copy()
    buf = torch.from_numpy(flat).cuda()
    base = buf.data_ptr()
    rc = L.crlot_phase_vocoder(plan._h, base + 4 * in_off, base + 4 * out_off, S, F, rate, ld_in, ldf, ld_out, ldf,
                               plan._cur_stream())
    assert rc == 0, L.crlot_last_error()
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert np.array_equal(bits(after[~is_out_row]), bits(before[~is_out_row]))  # guards and inputs keep their bits
    got = np.stack([np.stack([after[out_off + s * ld_out + k * ldf:][:row] for k in range(Fp)]) for s in range(S)])
    assert np.all(np.isfinite(got))
    assert np.array_equal(bits(got), bits(tight.view(np.float32)))


# ------------------------------------------------------------------ composition
def composed(torch, plan, x, rate):
    y = plan.istft_ola(plan.phase_vocoder(plan.stft(x), rate))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("pairing", [True, False])
@pytest.mark.parametrize("n,h", [(1024, 256), (960, 240)])
def test_time_stretch_is_the_composition(pkg, torch_cuda, n, h, pairing):
    torch = torch_cuda
    S, T = 3, 10000
    plan = plan_for(pkg, n, h, pairing)
    x = torch.from_numpy(np.random.default_rng(n + pairing).standard_normal((S, T)).astype(np.float32)).cuda()
    F = plan.frame_count(T)
    for rate in (0.8, 1.25):
        Fp = pkg.stretch_frame_count(F, rate)
        want = composed(torch, plan, x, rate)
        got = plan.time_stretch(x, rate)
        torch.cuda.synchronize()
        assert "k_phase_voc" in plan.last_launch()["kernels"]
        assert got.shape == (S, Fp * h) and plan.stretch_output_length(T, rate) == Fp * h
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.1
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), rate
    # a stored mask applies to the stretched frames: F rows are too few when F' > F
    plan.set_spectral_mask(torch.ones((F, n // 2 + 1), device="cuda"))
    try:
        with pytest.raises(ValueError):
            plan.time_stretch(x, 0.8)
        plan.time_stretch(x, 1.25)  # F' <= F: covered
    finally:
        plan.set_spectral_mask(None)


def test_time_stretch_in_two_slices(pkg, torch_cuda):
    """A shape whose spectra exceed the workspace cap.  4096 / 1024, S = 64,
    T = 131 072, rate 0.5: F = 128, F' = 256; per stream (128 + 256) rows x 4098
    floats x 4 bytes = 6 294 528 bytes; 268 435 456 // 6 294 528 = 42 streams per
    slice, so slices of 42 and 22 streams.  With a per-stream mask, so that the
    second slice must read its own streams' rows."""
    torch = torch_cuda
    n, h, S, T, rate = 4096, 1024, 64, 131072, 0.5
    plan = plan_for(pkg, n, h)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((S, T), device="cuda", generator=g)
    F = plan.frame_count(T)
    Fp = pkg.stretch_frame_count(F, rate)
    assert (F, Fp) == (128, 256) and (1 << 28) // ((F + Fp) * (n + 2) * 4) == 42
    mask = torch.rand((S, Fp, n // 2 + 1), device="cuda", generator=g)
    plan.set_spectral_mask(mask)
    try:
        want = composed(torch, plan, x, rate)
        plan.set_chunks(2)  # (the vocoder's grid then tells the slice: 22 streams x 33 column blocks x 2 chunks)
        got = plan.time_stretch(x, rate)
        torch.cuda.synchronize()
        rec = plan.last_launch()
    finally:
        plan.set_chunks(0)
        plan.set_spectral_mask(None)
    assert got.shape == (S, Fp * h)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    k = rec["kernels"].index("k_phase_voc")
    assert rec["kernels"][k - 1] == "k_phase_voc_sums"
    assert rec["grid"][k] == (22 * 33 * 2 + 3) // 4, rec


# ------------------------------------------------------------------ what a user hears
@pytest.mark.parametrize("rate", (0.5, 2.0))
def test_sinusoid_keeps_its_pitch(pkg, torch_cuda, rate):
    torch = torch_cuda
    n, h, T, k0 = 1024, 256, 32768, 32
    plan = plan_for(pkg, n, h)
    x = np.sin(2 * np.pi * k0 / n * np.arange(T)).astype(np.float32)
    y = plan.time_stretch(torch.from_numpy(x).cuda(), rate)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    Fp = pkg.stretch_frame_count(plan.frame_count(T), rate)
    assert y.shape == (Fp * h,)
    mid = y[len(y) // 2 - 2048:len(y) // 2 + 2048]
    spec = np.abs(np.fft.rfft(mid * np.hanning(4096)))
    assert int(np.argmax(spec)) == k0 * 4          # bin 32 of 1024 is bin 128 of 4096
    assert np.abs(mid).max() > 0.5
