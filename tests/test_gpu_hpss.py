"""GPU tests of HPSS (include/crlot_dsp.h, "HPSS"): crlot_hpss_masks against the
numpy float32 restatement of its contract (tests/hpss_reference.py), bit for bit,
on synthetic spectra uploaded directly, so a failure points at the two median
kernels; mask bits independent of chunking, batch and leading dimensions; memory
containment; crlot_hpss equal to the four-call composition through the public
Python entries, bit for bit; the oboe fixture against the oracle; the two parts
summing to the round trip; two host threads on one plan; errors and empties.
"""
import functools
import os
import threading

import numpy as np
import pytest

import hpss_reference as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_L2, MAX_ABS = 1e-6, 4e-6  # the split entries' bar (tests/test_gpu_parity.py)
HOPS = {256: 64, 400: 160, 512: 128, 1024: 256, 4096: 1024}
INF = float("inf")

_plans = {}


def plan_for(pkg, n, h=None, pairing=True):
    h = h or HOPS[n]
    key = (n, h, pairing)
    if key not in _plans:
        _plans[key] = pkg.Plan(frame_size=n, hop_size=h, frame_pairing=pairing)
    return _plans[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ref_power(power):
    return H.HARD if power == INF else power


@functools.lru_cache(maxsize=None)
def case_np(N, S, F, wh, wp, power, margins, nasty=False):
    """(spectra, reference mask_h, reference mask_p), computed once per case."""
    Z = H.make_spectrum(N, S, F, nasty=nasty)
    mh, mp = H.masks32(Z, wh, wp, ref_power(power), margins[0], margins[1])
    for a in (Z, mh, mp):
        a.setflags(write=False)
    return Z, mh, mp


# ------------------------------------------------------------------ 1. the masks
# every value of every axis at least once: N (bins 129 / 201 / 513), S, F (below r, at
# w, one past it, several chunks), the window pairs, the powers, the margins
MASK_CASES = [
    (256, 1, 1, 31, 31, 2, (1.0, 1.0)),
    (256, 3, 7, 3, 63, 1, (2.0, 3.7)),
    (400, 1, 31, 63, 3, INF, (1.0, 1.0)),
    (400, 3, 32, 17, 31, 2, (2.0, 3.7)),
    (1024, 3, 70, 31, 31, 1, (1.0, 1.0)),
    (1024, 1, 70, 17, 31, INF, (2.0, 3.7)),
    (1024, 3, 32, 63, 3, 2, (1.0, 1.0)),
    (256, 3, 70, 3, 63, 2, (2.0, 3.7)),
    (400, 3, 70, 1, 1, 1, (2.0, 3.7)),
]


@pytest.mark.parametrize("N,S,F,wh,wp,power,margins", MASK_CASES)
def test_masks_match_float32_restatement(pkg, torch_cuda, N, S, F, wh, wp, power, margins):
    torch = torch_cuda
    plan = plan_for(pkg, N)
    Z, want_h, want_p = case_np(N, S, F, wh, wp, power, margins)
    assert np.all(np.isfinite(want_h)) and np.all(np.isfinite(want_p))
    mh, mp = plan.hpss_masks(torch.from_numpy(Z.copy()).cuda(), (wh, wp), power, margins)
    torch.cuda.synchronize()
    assert plan.last_launch()["kernels"] == ["k_hpss_freq", "k_hpss_time"]
    assert np.array_equal(bits(mh.cpu().numpy()), bits(want_h))
    assert np.array_equal(bits(mp.cpu().numpy()), bits(want_p))


def test_unit_windows_give_half_everywhere(pkg, torch_cuda):
    torch = torch_cuda
    plan = plan_for(pkg, 1024)
    Z = H.make_spectrum(1024, 2, 9, nasty=True)
    for power in (1, 2):
        mh, mp = plan.hpss_masks(torch.from_numpy(Z).cuda(), 1, power, 1.0)
        assert bool((mh == 0.5).all()) and bool((mp == 0.5).all())


@pytest.mark.parametrize("power,margins", [(2, (1.0, 1.0)), (1, (2.0, 3.7)), (INF, (1.0, 1.0))])
def test_sanitize_zeros_and_ties(pkg, torch_cuda, power, margins):
    """Zero rows, columns and bands, NaN / Inf / 1e-35 components and a block of exact
    ties: sanitize, Z < FLT_MIN under both zero rules, and the hard masks' tie rule."""
    torch = torch_cuda
    N, S, F = 256, 2, 40
    plan = plan_for(pkg, N)
    Z, want_h, want_p = case_np(N, S, F, 5, 7, power, margins, True)
    m = H.magnitude32(Z)
    h, p = H.medians32(m, 5, 7)
    dead = (h == 0) & (p == 0)
    assert dead.sum() > 100                      # the Z < FLT_MIN branch is taken ...
    zero = np.float32(0.5 if margins == (1.0, 1.0) and power != INF else 0.0)
    assert np.all(want_h[dead] == zero) and np.all(want_p[dead] == zero)
    assert ((h == p) & (h > 0)).sum() > 100      # ... and so are exact ties
    mh, mp = plan.hpss_masks(torch.from_numpy(Z.copy()).cuda(), (5, 7), power, margins)
    assert np.array_equal(bits(mh.cpu().numpy()), bits(want_h))
    assert np.array_equal(bits(mp.cpu().numpy()), bits(want_p))


def test_bits_do_not_depend_on_chunks(pkg, torch_cuda):
    """F = 70 in 1, 2, 3 and 5 chunks (the last: 14 frames, fewer than r = 15): a
    halo that reflected at a chunk's end instead of the signal's would show here."""
    torch = torch_cuda
    N, S, F = 1024, 3, 70
    plan = plan_for(pkg, N)
    Z, want_h, want_p = case_np(N, S, F, 31, 31, 2, (1.0, 1.0))
    dZ = torch.from_numpy(Z.copy()).cuda()
    try:
        for chunks in (1, 2, 3, 5):
            plan.set_chunks(chunks)
            mh, mp = plan.hpss_masks(dZ)
            torch.cuda.synchronize()
            assert plan.last_launch()["n_chunks"] == chunks
            assert np.array_equal(bits(mh.cpu().numpy()), bits(want_h)), chunks
            assert np.array_equal(bits(mp.cpu().numpy()), bits(want_p)), chunks
    finally:
        plan.set_chunks(0)


def test_batch_independence_and_one_output(pkg, torch_cuda):
    torch = torch_cuda
    N, S, F = 400, 3, 32
    plan = plan_for(pkg, N)
    Z, want_h, want_p = case_np(N, S, F, 17, 31, 2, (2.0, 3.7))
    dZ = torch.from_numpy(Z.copy()).cuda()
    kw = dict(kernel_size=(17, 31), power=2, margin=(2.0, 3.7))
    mh, mp = plan.hpss_masks(dZ, **kw)
    for s in range(S):  # a stream alone (also as a 2-D tensor) = the stream inside the batch
        ah, ap = plan.hpss_masks(dZ[s], **kw)
        assert ah.shape == (F, N // 2 + 1)
        assert same_bits(torch, ah, mh[s]) and same_bits(torch, ap, mp[s])
    oh, none = plan.hpss_masks(dZ, mask_p=False, **kw)
    assert none is None and same_bits(torch, oh, mh)
    none, op = plan.hpss_masks(dZ, mask_h=False, **kw)
    assert none is None and same_bits(torch, op, mp)
    assert np.array_equal(bits(mh.cpu().numpy()), bits(want_h))


def test_containment_padded_leading_dimensions(pkg, torch_cuda):
    """Spectra with NaN between their rows and streams; masks with rows of bins + 3
    floats and two spare rows per stream in one sentinel-filled allocation with a
    guard region behind the last row: the masks equal the reference and every
    other float keeps its sentinel bits."""
    torch = torch_cuda
    N, S, F = 256, 3, 31
    bins = N // 2 + 1
    plan = plan_for(pkg, N)
    Z, want_h, want_p = case_np(N, S, F, 31, 31, 2, (1.0, 1.0))
    big = torch.full((S, F + 2, bins + 3), float("nan"), dtype=torch.complex64, device="cuda")
    big[:, 1:F + 1, :bins] = torch.from_numpy(Z.copy()).cuda()
    spec = big[:, 1:F + 1, :bins]
    SENT = 0x7FC0BEEF  # a NaN's bits
    guard = 4096
    rows = S * (F + 2) * (bins + 3)
    flat = torch.full((2 * (rows + guard),), SENT, dtype=torch.int32, device="cuda").view(torch.float32)
    views = []
    for i in range(2):
        base = i * (rows + guard)
        views.append(flat[base:base + rows].view(S, F + 2, bins + 3)[:, 1:F + 1, :bins])
    mh, mp = plan.hpss_masks(spec, mask_h=views[0], mask_p=views[1])
    torch.cuda.synchronize()
    assert mh.data_ptr() == views[0].data_ptr() and mp.data_ptr() == views[1].data_ptr()
    assert np.array_equal(bits(mh.cpu().numpy()), bits(want_h))
    assert np.array_equal(bits(mp.cpu().numpy()), bits(want_p))
    written = torch.zeros_like(flat, dtype=torch.bool)
    for i in range(2):
        base = i * (rows + guard)
        written[base:base + rows].view(S, F + 2, bins + 3)[:, 1:F + 1, :bins] = True
    untouched = flat.view(torch.int32)[~written]
    assert untouched.numel() == 2 * (rows + guard) - 2 * S * F * bins
    assert bool((untouched == SENT).all())


# ------------------------------------------------------------------ 2. crlot_hpss is the composition
def signal(torch, S, T, seed):
    """Noise, two tones and a click every 2000 samples, per stream."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    x = 0.1 * rng.standard_normal((S, T))
    for s in range(S):
        x[s] += 0.5 * np.sin(2 * np.pi * (0.01 + 0.003 * s) * t) + 0.3 * np.sin(2 * np.pi * 0.031 * t)
        x[s, 500 + 37 * s::2000] += 1.0
    return torch.from_numpy(x.astype(np.float32)).cuda()


def compose(torch, plan, x, want_h=True, want_p=True, **kw):
    """The definition: the calls a user writes on the public entries."""
    X = plan.stft(x)
    Mh, Mp = plan.hpss_masks(X, mask_h=None if want_h else False, mask_p=None if want_p else False, **kw)
    out = []
    try:
        for M in (Mh, Mp):
            if M is None:
                out.append(None)
                continue
            plan.set_spectral_mask(M)
            out.append(plan.istft_ola(X))
    finally:
        plan.set_spectral_mask(None)
    torch.cuda.synchronize()
    return out[0], out[1]


@pytest.mark.parametrize("n,h,pairing", [(1024, 256, True), (1024, 256, False), (512, 128, True), (512, 128, False),
                                         (400, 160, True), (1024, 300, True)])
def test_hpss_is_the_composition(pkg, torch_cuda, n, h, pairing):
    torch = torch_cuda
    S, T = 3, 70 * h + 123  # T not a multiple of H
    plan = plan_for(pkg, n, h, pairing)
    x = signal(torch, S, T, n + h)
    F = plan.frame_count(T)
    for kw in (dict(), dict(kernel_size=(17, 5), power=1, margin=(2.0, 3.7)), dict(power=INF)):
        want_h, want_p = compose(torch, plan, x, **kw)
        got_h, got_p = plan.hpss(x, **kw)
        torch.cuda.synchronize()
        rec = plan.last_launch()["kernels"]
        assert "k_hpss_freq" in rec and rec.index("k_hpss_time") == rec.index("k_hpss_freq") + 1
        assert got_h.shape == (S, F * h) and got_p.shape == (S, F * h)
        assert bool(torch.isfinite(got_h).all()) and float(got_h.abs().max()) > 0.05
        assert same_bits(torch, got_h, want_h) and same_bits(torch, got_p, want_p), kw
    # one output skipped: the other unchanged
    only_h, none = plan.hpss(x, y_p=False)
    assert none is None and same_bits(torch, only_h, compose(torch, plan, x)[0])
    none, only_p = plan.hpss(x, y_h=False)
    assert none is None and same_bits(torch, only_p, compose(torch, plan, x)[1])
    # a stream alone = the stream in the batch; padded output rows
    a_h, a_p = plan.hpss(x[1])
    w_h, w_p = compose(torch, plan, x)
    assert same_bits(torch, a_h, w_h[1]) and same_bits(torch, a_p, w_p[1])
    pad = torch.full((2, S, F * h + 6), 7.0, device="cuda")
    plan.hpss(x, y_h=pad[0, :, :F * h], y_p=pad[1, :, :F * h])
    assert same_bits(torch, pad[0, :, :F * h], w_h) and same_bits(torch, pad[1, :, :F * h], w_p)
    assert bool((pad[:, :, F * h:] == 7.0).all())


def test_hpss_with_a_spectral_gain(pkg, torch_cuda):
    torch = torch_cuda
    n, h, S, T = 1024, 256, 2, 40 * 256
    plan = pkg.Plan(frame_size=n, hop_size=h)
    x = signal(torch, S, T, 5)
    plain = compose(torch, plan, x)
    plan.set_spectral_gain(np.linspace(0.25, 2.0, n // 2 + 1).astype(np.float32))
    torch.cuda.synchronize()
    want_h, want_p = compose(torch, plan, x)
    got_h, got_p = plan.hpss(x)
    torch.cuda.synchronize()
    assert same_bits(torch, got_h, want_h) and same_bits(torch, got_p, want_p)
    assert not same_bits(torch, got_h, plain[0])  # (the gain did ride)
    plan.close()


def test_hpss_in_two_slices(pkg, torch_cuda):
    """4096 / 1024, S = 64, T = 131 072: F = 128; per stream 128 rows x (4098 spectrum
    + 3 x 2049 medians and masks) floats x 4 bytes = 5 245 440 bytes; 268 435 456 //
    5 245 440 = 51 streams per slice, so slices of 51 and 13 streams."""
    torch = torch_cuda
    n, h, S, T = 4096, 1024, 64, 131072
    plan = plan_for(pkg, n, h)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn((S, T), device="cuda", generator=g)
    x[:, 777::9000] += 20.0
    F = plan.frame_count(T)
    assert F == 128 and (1 << 28) // (F * (n + 2 + 3 * (n // 2 + 1)) * 4) == 51
    want_h, want_p = compose(torch, plan, x)
    got_h, got_p = plan.hpss(x)
    torch.cuda.synchronize()
    rec = plan.last_launch()
    assert same_bits(torch, got_h, want_h) and same_bits(torch, got_p, want_p)
    # the last slice: 13 streams x 2 tiles of 64 frames x at most 2049 // 96 = 21 bin segments
    # (a slice of 51 streams would give a multiple of 102, which needs 51 segments)
    grid = rec["grid"][rec["kernels"].index("k_hpss_freq")]
    assert grid % (13 * 2) == 0 and grid // (13 * 2) <= 21 and grid % (51 * 2) != 0, rec


# ------------------------------------------------------------------ 3. against the oracle
def test_oboe_with_clicks_vs_oracle(pkg, oracle, torch_cuda):
    """The first 2 s of the oboe fixture with a click every 0.25 s, 1024 / 256, pairing
    off: the device masks equal the reference applied to the device spectra bit for
    bit; y_h and y_p meet the split entries' bar against the oracle's masked round
    trip under those masks; the tone goes to y_h and the clicks to y_p."""
    torch = torch_cuda
    n, h = 1024, 256
    x, sr = pkg.load_wav_mono(os.path.join(ROOT, "tests", "golden", "oboe.wav"))
    x = np.ascontiguousarray(x[:2 * sr], np.float32)
    clicks = np.arange(sr // 8, x.size, sr // 4)
    x[clicks] += np.float32(0.8)
    plan = plan_for(pkg, n, h, pairing=False)
    dx = torch.from_numpy(x).cuda()
    X = plan.stft(dx)
    mh, mp = plan.hpss_masks(X)
    y_h, y_p = plan.hpss(dx)
    torch.cuda.synchronize()
    want_h, want_p = H.masks32(X.cpu().numpy())
    assert np.array_equal(bits(mh.cpu().numpy()), bits(want_h))
    assert np.array_equal(bits(mp.cpu().numpy()), bits(want_p))
    xmax = float(np.max(np.abs(x)))
    for y, m, what in ((y_h, want_h, "harmonic"), (y_p, want_p, "percussive")):
        ref = oracle.roundtrip_mask(x, n, h, mask=m)
        got = y.cpu().numpy()
        assert got.shape == ref.shape and np.all(np.isfinite(got))
        d = got.astype(np.float64) - ref
        rel = np.linalg.norm(d) / np.linalg.norm(ref)
        print(f"{what}: rel-L2 {rel:.3e}, max-abs {np.max(np.abs(d)) / xmax:.3e} of max|x|")
        assert rel <= REL_L2 and np.max(np.abs(d)) <= MAX_ABS * xmax, what
    yh, yp = y_h.cpu().numpy(), y_p.cpu().numpy()
    # what a user hears: between the clicks the tone is in y_h, at the clicks y_p stands out
    at = clicks[(clicks > n) & (clicks < yh.size - n)]
    quiet = np.ones(yh.size, bool)
    for c in clicks:
        quiet[max(0, c - n):c + n] = False
    quiet[:n] = quiet[-n:] = False
    rms = lambda v: float(np.sqrt(np.mean(np.square(v, dtype=np.float64))))  # noqa: E731
    print(f"between clicks: rms y_h {rms(yh[quiet]):.3e}, y_p {rms(yp[quiet]):.3e}; at clicks: mean |y_p| "
          f"{float(np.mean(np.abs(yp[at]))):.3e}, |y_h| {float(np.mean(np.abs(yh[at]))):.3e}")
    assert rms(yh[quiet]) > rms(yp[quiet])
    assert float(np.mean(np.abs(yp[at]))) > 2 * rms(yp[quiet])


def test_parts_sum_to_the_round_trip(pkg, torch_cuda):
    """Power 1, margins 1: the masks sum to 1 within rounding, the inversion is
    linear and two outputs are summed, so y_h + y_p is within twice the split
    entries' bar of crlot_roundtrip(x), per stream."""
    torch = torch_cuda
    n, h, S, T = 1024, 256, 3, 64 * 256
    plan = plan_for(pkg, n, h)
    x = signal(torch, S, T, 9)
    y_h, y_p = plan.hpss(x, power=1)
    rt = plan.roundtrip(x)
    torch.cuda.synchronize()
    F = plan.frame_count(T)
    got = (y_h.double() + y_p.double()).cpu().numpy()
    ref = rt[:, :F * h].double().cpu().numpy()
    for s in range(S):
        d = got[s] - ref[s]
        xmax = float(x[s].abs().max())
        rel = np.linalg.norm(d) / np.linalg.norm(ref[s])
        print(f"stream {s}: rel-L2 {rel:.3e}, max-abs {np.max(np.abs(d)) / xmax:.3e} of max|x|")
        assert rel <= 2 * REL_L2 and np.max(np.abs(d)) <= 2 * MAX_ABS * xmax


# ------------------------------------------------------------------ 4. threads
def test_two_host_threads_one_plan(pkg, torch_cuda):
    """Two host threads, one plan, two HIP streams, different inputs: both reproduce
    their single-threaded bits (nothing is stored in the plan; scratch is per stream)."""
    torch = torch_cuda
    n, h, S, T = 1024, 256, 8, 48 * 256
    plan = plan_for(pkg, n, h)
    xs = [signal(torch, S, T, 21), signal(torch, S, T, 22)]
    kws = [dict(), dict(kernel_size=(17, 31), power=1, margin=(1.0, 2.0))]
    serial = [plan.hpss(x, **kw) for x, kw in zip(xs, kws)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    results, errors = [[], []], []
    barrier = threading.Barrier(2)

    def work(i):
        try:
            barrier.wait(timeout=30)
            with torch.cuda.stream(streams[i]):
                for _ in range(4):
                    results[i].append(plan.hpss(xs[i], **kws[i]))
            streams[i].synchronize()
        except Exception as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((i, repr(e)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        assert len(results[i]) == 4
        for y_h, y_p in results[i]:
            assert same_bits(torch, y_h, serial[i][0]) and same_bits(torch, y_p, serial[i][1]), i
    assert plan._mask is None


# ------------------------------------------------------------------ 5. errors and empties
def test_errors_and_empties(pkg, torch_cuda):
    torch = torch_cuda
    n, h, S, F = 256, 64, 2, 9
    bins = n // 2 + 1
    plan = plan_for(pkg, n, h)
    L = pkg.lib()
    d = pkg._hpss_desc()
    import ctypes as C
    spec = torch.zeros((S, F, bins), dtype=torch.complex64, device="cuda")
    m = torch.full((2, S, F, bins), 3.0, device="cuda")
    row = 2 * bins

    def masks(sp=None, mh=None, mp=None, ns=S, nf=F, ld_s=F * row, ldf_s=row, ld_m=F * bins, ldf_m=bins):
        sp = spec.data_ptr() if sp is None else sp
        mh = m[0].data_ptr() if mh is None else mh
        mp = m[1].data_ptr() if mp is None else mp
        return L.crlot_hpss_masks(plan._h, C.byref(d), sp, mh, mp, ns, nf, ld_s, ldf_s, ld_m, ldf_m, ld_m, ldf_m, None)

    assert masks() == 0
    assert masks(ldf_s=row - 2) == pkg.EINVAL and masks(ld_s=(F - 1) * row) == pkg.EINVAL   # short leading dimensions
    assert masks(ldf_m=bins - 1) == pkg.EINVAL and masks(ld_m=(F - 1) * bins) == pkg.EINVAL
    assert masks(ldf_s=row + 1) == pkg.EINVAL and masks(sp=spec.data_ptr() + 4) == pkg.EINVAL  # float pairs
    assert masks(ns=-1) == pkg.EINVAL and masks(nf=-1) == pkg.EINVAL
    assert masks(mh=spec.data_ptr()) == pkg.EINVAL                   # an output on the input
    assert masks(mp=m[0].data_ptr() + 4 * bins) == pkg.EINVAL        # the outputs on each other
    assert masks(mh=0, mp=0) == pkg.EINVAL
    m.fill_(3.0)
    assert masks(ns=0) == 0 and masks(nf=0) == 0
    torch.cuda.synchronize()
    assert bool((m == 3.0).all())
    with pytest.raises(ValueError):
        plan.hpss_masks(spec, mask_h=m[0], mask_p=m[0])              # the Python front sees the overlap first

    T = F * h + n - h
    x = torch.zeros((S, T), device="cuda")
    y = torch.full((2, S, plan.frame_count(T) * h), 3.0, device="cuda")

    def hpss(xp=None, yh=None, yp=None, ns=S, t=T, ld_x=T, ld_y=None):
        ld_y = y.shape[2] if ld_y is None else ld_y
        xp = x.data_ptr() if xp is None else xp
        yh = y[0].data_ptr() if yh is None else yh
        yp = y[1].data_ptr() if yp is None else yp
        return L.crlot_hpss(plan._h, C.byref(d), xp, yh, yp, ns, t, ld_x, ld_y, ld_y, None)

    assert hpss() == 0
    y.fill_(3.0)
    assert hpss(ns=0) == 0                                 # empty: nothing written
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    assert hpss(ld_x=T - 1) == pkg.EINVAL and hpss(ld_y=y.shape[2] - 1) == pkg.EINVAL
    assert hpss(yh=x.data_ptr()) == pkg.EINVAL and hpss(yp=y[0].data_ptr() + 8) == pkg.EINVAL
    assert hpss(yh=0, yp=0) == pkg.EINVAL and hpss(ns=-1) == pkg.EINVAL
    # a plan with a stored mask: refused by the library, and by the Python front before it
    plan.set_spectral_mask(torch.ones((F + 8, bins), device="cuda"))
    try:
        assert hpss() == pkg.EINVAL and b"stored mask" in L.crlot_last_error()
        with pytest.raises(ValueError):
            plan.hpss(x)
    finally:
        plan.set_spectral_mask(None)
    assert hpss() == 0
    torch.cuda.synchronize()
