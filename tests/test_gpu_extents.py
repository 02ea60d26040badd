"""Far offsets and long streams: the extent guards of abi.cpp, pinned on both sides.

test_full_size_* stops at 1024 x 480 000, whose last stream starts 1.96e9 bytes
into x: nothing else addresses x or y beyond 2^31 bytes, 2^32 bytes or 2^31
elements, and no test sits next to a limit of the guards that choose the kernel.

Far rows (test_far_rows): few streams with a huge leading dimension, T = 9N + 37
samples touched per row.  ld = 2^30 + 2 floats with S = 3 puts rows 1 and 2 beyond
2^32 bytes and row 2 beyond 2^31 elements; ld = 2^31 + 2 with S = 2 exercises any
32-bit narrowing of ld itself.  Each row has 64 KiB of NaN (x) or sentinel (y)
on either side; only those windows are filled and scanned.  The result is
bit-equal to the same rows as a small tight batch where both calls run the same
kernels, within test_gpu_parity's bar where the guards send the far call
elsewhere (N = 960 / 480: ld >= 2^27 leaves K_pair15 and, at N = 480, the
pair-15 spectral walkers, whose buffer descriptor spans two streams).

Long streams (test_long_*): one stream (two at N = 480) at three lengths per
guard expression -- the largest T every term of the guard admits, a T where only
the output-length term fails (ZERO_PAD: F H reaches the limit before T does), and
T equal to the limit.  Kernels are asserted on each side; the output is finite
over its whole length; head, middle and tail slices meet the parity bar against
the oracle (tests/extent_reference.py); the tail frames' spectra meet
assert_spec_close; and the below-limit and at-limit results, which come from
different kernels, agree within the parity bar over their whole common length,
compared on the device in float64, piece by piece.

The guard n_streams * (T / H + 1) < 2^29 needs 2^36 samples and is out of reach.
"""
import numpy as np
import pytest

import extent_reference as ER
import test_gpu_containment as TC
from test_gpu_parity import MAX_ABS, REL_L2, assert_close, host
from test_gpu_stft import assert_spec_close

pytestmark = pytest.mark.gpu

GIB = 1 << 30
GUARD = 16384  # floats: 64 KiB on each side of each row

# ------------------------------------------------------------------ far rows
GEOMETRIES = {"ld=2^30+2 S=3": ((1 << 30) + 2, 3), "ld=2^31+2 S=2": ((1 << 31) + 2, 2)}

FAR_SHAPES = ["1024/256", "512/128", "4096/1024", "256/128", "1024/256 unpaired", "960/240", "480/120", "882/441",
              "1920/480", "1024/300 staged"]
FAR_ENTRIES = ["roundtrip", "mask_shared", "stft", "istft_ola"]

# The far call's kernels where they are not the tight call's (TC.ROUTES / TC.TIGHT_ROUTES):
#   roundtrip_impl: K_pair15 needs ld_x, ld_y < 2^27 at N = 960 and 480 -> the per-frame K_fused_any alone;
#   pair15_spec_fits: at N = 480 ld < 2^27 -> stft, istft_ola and the masked round trip run staged
#   (dense spectra, so one rfft launch and no k_spec_step copy unless a mask is set).
# Every other shape keeps its walker: K_pair at 1024/256 must stay.
FAR_ROUTES = {
    "960/240": {"roundtrip": ["k_fused_any"]},
    "480/120": {"roundtrip": ["k_fused_any"],
                "mask": ["k_frames_w", "k_fft_any", "k_spec_step", "k_fft_any", "k_gather"],
                "stft": ["k_frames_w", "k_fft_any"],
                "istft_ola": ["k_fft_any", "k_gather"]},
}


@pytest.fixture(scope="module")
def far(torch_cuda):
    """x and y, 8 GiB each, shared by the far-row tests (never filled or scanned whole)."""
    torch = torch_cuda
    width = TC.even(9 * 4096 + 37 + 4096)
    size = max((S - 1) * ld for ld, S in GEOMETRIES.values()) + 2 * GUARD + width
    need = 2 * 4 * size + 2 * GIB
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"far rows need {need / GIB:.1f} GiB of device memory, {free / GIB:.1f} GiB are free")
    bufs = {"x": torch.empty(size, dtype=torch.float32, device="cuda"),
            "yi": torch.empty(size, dtype=torch.int32, device="cuda")}
    yield bufs
    bufs.clear()
    torch.cuda.empty_cache()


def far_route(shape, entry, S):
    key = TC.route_key(entry)
    if key in FAR_ROUTES.get(shape, {}):
        return FAR_ROUTES[shape][key]
    return TC.expected_route(TC.ROUTES, shape, entry, S, tight=True)


@pytest.mark.parametrize("entry", FAR_ENTRIES)
@pytest.mark.parametrize("shape", FAR_SHAPES)
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_far_rows(pkg, torch_cuda, far, geometry, shape, entry):
    torch = torch_cuda
    ld, S = GEOMETRIES[geometry]
    plan, n, h = TC.make_plan(pkg, shape, entry)
    T = 9 * n + 37
    F = plan.frame_count(T)
    L = F * h
    data = TC.make_data(torch, plan, entry, S, T, n, seed=n + h + S)
    # the tight call first: the same rows as a small batch
    arena, ops = TC.layout(entry, S, T, F, n, h, 0, False)
    arena.build(torch)
    t = {k: arena.view(i) for k, i in ops.items()}
    for k in ("x", "mask", "spec"):
        if k in t and not arena.ops[ops[k]][3]:
            t[k].copy_(data[k].reshape(t[k].shape))
    ref, ks_near = TC.run_entry(torch, plan, entry, t)
    assert ks_near == TC.expected_route(TC.ROUTES, shape, entry, S, tight=True), (shape, entry, ks_near)
    # the far call: x rows and y rows ld apart, windows of GUARD | row | GUARD
    win = 2 * GUARD + TC.even(max(T, L))
    xw = far["x"].as_strided((S, win), (ld, 1), 0)
    yw = far["yi"].as_strided((S, win), (ld, 1), 0)
    xw.fill_(float("nan"))
    yw.fill_(TC.SENTINEL)
    ft = dict(t)
    if "x" in t:
        ft["x"] = far["x"].as_strided((S, T), (ld, 1), GUARD)
        ft["x"].copy_(data["x"])
    if "y" in t:
        ft["y"] = far["yi"].view(torch.float32).as_strided((S, L), (ld, 1), GUARD)
    if "spec" in t and arena.ops[ops["spec"]][3]:
        ft["spec"] = torch.full_like(t["spec"], float("nan"))
    x_before = xw.view(torch.int32).clone()
    got, ks_far = TC.run_entry(torch, plan, entry, ft)
    assert ks_far == far_route(shape, entry, S), (geometry, shape, entry, ks_far)
    # guards: nothing but the output rows changed in y's windows, nothing at all in x's
    y_after = yw.clone()
    if "y" in t:
        y_after[:, GUARD:GUARD + L] = TC.SENTINEL
    bad = torch.nonzero(y_after != TC.SENTINEL)
    assert bad.numel() == 0, f"{geometry} {shape} {entry}: y guard overwritten at (row, window offset) {bad[:4].tolist()}"
    assert torch.equal(xw.view(torch.int32), x_before), f"{geometry} {shape} {entry}: x changed"
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), (geometry, shape, entry, k)
        if ks_far == ks_near:
            assert torch.equal(got[k].contiguous().view(torch.int32), ref[k].contiguous().view(torch.int32)), \
                f"{geometry} {shape} {entry}: {k} differs from the tight batch"
        else:
            g, r = host(got[k]).reshape(S, -1), host(ref[k]).reshape(S, -1)
            for s in range(S):
                assert_close(g[s], r[s], float(np.max(np.abs(r[s]))), f"{geometry} {shape} {entry} {k} stream {s}",
                             float(np.linalg.norm(r[s].astype(np.float64))))


# ------------------------------------------------------------------ long streams at the guards
LIM27, LIM29 = 1 << 27, 1 << 29  # 134217728, 536870912

# Lengths on either side of a guard.  F = ceil(T / H) (ZERO_PAD), out_len = F H.
#   "out":  T < lim && out_len < lim                 crlot_roundtrip at the 2^27 family
#   "outn": T < lim && out_len + k N < lim           k = 1: masked round trip, istft_ola at the 2^27 family
#                                                    k = 2: round trip, masked, istft_ola at the 2^29 family
#   "t":    T < lim                                  crlot_stft
# a: the largest T every term admits = Fmax H with Fmax = floor((lim - k N - 1) / H);
# b: a + 2 (one more frame: only the out_len term fails; + 2 keeps single rows 8-byte wide);
# c: lim.
LENGTHS = {
    # (960, 240): Fmax = floor((2^27 - 1) / 240) = 559240 -> 559240 * 240; k = 1: floor((2^27 - 961) / 240) = 559236
    (960, 240): {"out": (134217600, 134217602, LIM27), "outn": (134216640, 134216642, LIM27)},
    # (480, 120): floor((2^27 - 1) / 120) = 1118481; floor((2^27 - 481) / 120) = 1118477
    (480, 120): {"out": (134217720, 134217722, LIM27), "outn": (134217240, 134217242, LIM27)},
    # (882, 441): floor((2^27 - 1) / 441) = 304348; floor((2^27 - 883) / 441) = 304346
    (882, 441): {"out": (134217468, 134217470, LIM27), "outn": (134216586, 134216588, LIM27)},
    # (1920, 480): floor((2^27 - 1) / 480) = 279620; floor((2^27 - 1921) / 480) = 279616
    (1920, 480): {"out": (134217600, 134217602, LIM27), "outn": (134215680, 134215682, LIM27)},
    # (1024, 512): floor((2^29 - 2049) / 512) = 1048571
    (1024, 512): {"outn": (536868352, 536868354, LIM29)},
    # (4096, 2048): floor((2^29 - 8193) / 2048) = 262139
    (4096, 2048): {"outn": (536860672, 536860674, LIM29)},
}
for (_n, _h), _d in LENGTHS.items():  # the arithmetic above, checked
    _lim, _k = (LIM27, 1) if (_n, _h) in ((960, 240), (480, 120), (882, 441), (1920, 480)) else (LIM29, 2)
    for _name, (_a, _b, _c) in _d.items():
        _extra = 0 if _name == "out" else _k * _n
        assert _a < _lim and -(-_a // _h) * _h + _extra < _lim and _a % _h == 0
        assert -(-(_a + _h) // _h) * _h + _extra >= _lim  # a is the largest such multiple of H ...
        assert _b < _lim and -(-_b // _h) * _h + _extra >= _lim and _c == _lim  # ... and any T beyond it fails

# kernels below the limit (walkers) and at it (fallbacks)
WALK = {
    (960, 240): {"roundtrip": ["k_pair15", "k_fused_any"]},
    (480, 120): {"roundtrip": ["k_pair15", "k_fused_any"]},
    (882, 441): {"roundtrip": ["k_pairn", "k_fused_any"]},
    (1920, 480): {"roundtrip": ["k_pair30", "k_fused_any"]},
    (1024, 512): {"roundtrip": ["k_pair_hot", "k_pair_fix"]},
    (4096, 2048): {"roundtrip": ["k_pair4k_hot", "k_pair4k"]},
}
for _v in WALK.values():
    _v.update({"mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"]})
ANY_FALLBACK = {"roundtrip": ["k_fused_any"], "stft": ["k_frames_w", "k_fft_any"],
                "istft_ola": ["k_fft_any", "k_gather"],
                # masked, spectra through HBM: the stft half still runs the walker while T < 2^27 ("mask_b")
                "mask_b": ["k_pair_stft", "k_spec_step", "k_fft_any", "k_gather"],
                "mask": ["k_frames_w", "k_fft_any", "k_spec_step", "k_fft_any", "k_gather"]}
POW2_FALLBACK = {"roundtrip": ["k_synth", "k_gather"], "stft": ["k_stft"], "istft_ola": ["k_istft"],
                 "mask_b": ["k_stft_masked"], "mask": ["k_stft_masked"]}
LONG_SHAPES = list(LENGTHS)


def fallback(n, h):
    return POW2_FALLBACK if n in (1024, 4096) else ANY_FALLBACK


def long_setup(pkg, torch, n, h, need_gib):
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need_gib * GIB:
        pytest.skip(f"{n}/{h} long streams need {need_gib} GiB of device memory, {free / GIB:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats()
    S = 2 if n == 480 else 1  # N = 480: one buffer descriptor spans two streams
    lim = LIM27 if n not in (1024, 4096) else LIM29
    g = torch.Generator(device="cuda").manual_seed(n * 7 + h)
    x = (torch.rand((S, lim), generator=g, device="cuda") * 2 - 1) * 0.5
    return pkg.Plan(frame_size=n, hop_size=h), S, lim, x


def report_peak(torch, what):
    print(f"[extents] {what}: peak device memory {torch.cuda.max_memory_allocated() / GIB:.2f} GiB")


def prefix(torch, x, T):
    """x[:, :T] as a tensor of its own: a row stride of T, as a caller's batch of that length has."""
    return x if T == x.shape[1] else x[:, :T].contiguous()


def check_slices(oracle, x, y, T, n, h, what, mask=None):
    """Head, middle and tail slices of every stream against the oracle."""
    ring = oracle.ring_len(n, h)
    span = ER.min_span(n, h, ring)
    for s in range(x.shape[0]):
        def run(xs, k0):
            if mask is None:
                return oracle.roundtrip(xs, n, h)
            rows = host(mask[k0:k0 + oracle.frame_count(xs.size, n, h)])
            return oracle.roundtrip_mask(xs, n, h, mask=rows)
        for sl, lo, hi, ref in ER.roundtrip_slices(run, lambda a, b: host(x[s, a:b]), T, n, h, ring, span):
            xs = host(x[s, sl.a:sl.b]).astype(np.float64)
            assert_close(host(y[s, lo:hi]), ref, 0.5, f"{what} stream {s} {sl.name} slice [{lo}, {hi})",
                         float(np.linalg.norm(xs)))


def assert_agree(torch, a, b, length, what, scale=0.5, piece=1 << 24):
    """a[..., :length] and b[..., :length] within the parity bar, per piece, on the
    device in float64: a corrupted stretch anywhere fails its own piece."""
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    for s in range(a.shape[0]):
        for p0 in range(0, length, piece):
            p1 = min(length, p0 + piece)
            u, v = a[s, p0:p1].double(), b[s, p0:p1].double()
            d = u - v
            rel = float(d.norm() / v.norm().clamp_min(1e-30))
            mx = float(d.abs().max())
            assert rel <= REL_L2 and mx <= MAX_ABS * scale, \
                f"{what}: stream {s} piece [{p0}, {p1}): rel-L2 {rel:.3e}, max-abs {mx:.3e}"


def finite(torch, t):
    return bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all())


@pytest.mark.parametrize("n,h", LONG_SHAPES)
def test_long_roundtrip(pkg, oracle, torch_cuda, n, h):
    torch = torch_cuda
    plan, S, lim, x = long_setup(pkg, torch, n, h, 14)
    Ta, Tb, Tc = LENGTHS[(n, h)]["out" if lim == LIM27 else "outn"]
    want = {Ta: WALK[(n, h)]["roundtrip"], Tb: fallback(n, h)["roundtrip"], Tc: fallback(n, h)["roundtrip"]}
    ys = {}
    for T in (Ta, Tb, Tc):
        xp = prefix(torch, x, T)
        y = plan.roundtrip(xp)
        torch.cuda.synchronize()
        assert plan.last_launch()["kernels"] == want[T], (n, h, T, plan.last_launch())
        assert y.shape == (S, plan.output_length(T)) and finite(torch, y), (n, h, T)
        check_slices(oracle, xp, y, T, n, h, f"{n}/{h} roundtrip T={T}")
        ys[T] = y
        del xp
    for T in (Tb, Tc):  # different kernels, the same prefix of x: every sample whose frames lie inside Ta
        assert_agree(torch, ys[Ta], ys[T], Ta - n, f"{n}/{h} roundtrip T={Ta} vs T={T}")
    report_peak(torch, f"roundtrip {n}/{h}")
    del x, ys, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,h", LONG_SHAPES)
def test_long_masked_roundtrip(pkg, oracle, torch_cuda, n, h):
    torch = torch_cuda
    plan, S, lim, x = long_setup(pkg, torch, n, h, 30)
    Ta, Tb, Tc = LENGTHS[(n, h)]["outn"]
    fb = fallback(n, h)
    want = {Ta: WALK[(n, h)]["mask"], Tb: fb["mask_b"], Tc: fb["mask"]}
    g = torch.Generator(device="cuda").manual_seed(n + h)
    mask = torch.rand((plan.frame_count(Tc), n // 2 + 1), generator=g, device="cuda") * 0.75 + 0.25
    plan.set_spectral_mask(mask)  # one row per frame, shared by the streams
    ys = {}
    try:
        for T in (Ta, Tb, Tc):
            xp = prefix(torch, x, T)
            y = plan.roundtrip(xp)
            torch.cuda.synchronize()
            assert plan.last_launch()["kernels"] == want[T], (n, h, T, plan.last_launch())
            assert y.shape == (S, plan.output_length(T)) and finite(torch, y), (n, h, T)
            check_slices(oracle, xp, y, T, n, h, f"{n}/{h} masked T={T}", mask=mask)
            ys[T] = y
            del xp
    finally:
        plan.set_spectral_mask(None)
    for T in (Tb, Tc):
        assert_agree(torch, ys[Ta], ys[T], Ta - n, f"{n}/{h} masked T={Ta} vs T={T}")
    report_peak(torch, f"masked roundtrip {n}/{h}")
    del x, ys, y, mask
    torch.cuda.empty_cache()


def check_tail_spectra(oracle, x, spec, T, n, h, what, count=8):
    F = spec.shape[1]
    for s in range(x.shape[0]):
        k0, ref = ER.stft_rows(lambda xs: oracle.roundtrip_mask(xs, n, h, want_spec=True)[1],
                               lambda a, b: host(x[s, a:b]), T, n, h, (F - count) * h, count)
        assert k0 == F - count and ref.shape[0] == count
        assert_spec_close(host(spec[s, k0:]), ref, f"{what} stream {s} tail frames")
        k0, ref = ER.stft_rows(lambda xs: oracle.roundtrip_mask(xs, n, h, want_spec=True)[1],
                               lambda a, b: host(x[s, a:b]), T, n, h, (F // 2) * h, count)
        assert_spec_close(host(spec[s, k0:k0 + count]), ref, f"{what} stream {s} middle frames")


@pytest.mark.parametrize("n,h", LONG_SHAPES)
def test_long_stft(pkg, oracle, torch_cuda, n, h):
    torch = torch_cuda
    plan, S, lim, x = long_setup(pkg, torch, n, h, 24)
    Ta, Tc = lim - 1, lim  # crlot_stft's guard has the one term T < lim
    want = {Ta: WALK[(n, h)]["stft"], Tc: fallback(n, h)["stft"]}
    specs = {}
    for T in (Ta, Tc):
        xp = prefix(torch, x, T)
        spec = plan.stft(xp)
        torch.cuda.synchronize()
        assert plan.last_launch()["kernels"] == want[T], (n, h, T, plan.last_launch())
        assert spec.shape == (S, plan.frame_count(T), n // 2 + 1) and finite(torch, spec), (n, h, T)
        check_tail_spectra(oracle, xp, spec, T, n, h, f"{n}/{h} stft T={T}")
        specs[T] = spec
        del xp
    # frames that lie inside Ta: the same samples, different kernels; spectra scale with N / 2 * max|x|
    common = (Ta - n) // h + 1
    ra, rc = torch.view_as_real(specs[Ta]), torch.view_as_real(specs[Tc])
    scale = float(rc[:, :64].abs().max())
    assert_agree(torch, ra, rc, common * (n // 2 + 1) * 2, f"{n}/{h} stft T={Ta} vs T={Tc}", scale=scale)
    report_peak(torch, f"stft {n}/{h}")
    del x, specs, spec, ra, rc
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,h", LONG_SHAPES)
def test_long_istft_of_stft(pkg, oracle, torch_cuda, n, h):
    torch = torch_cuda
    plan, S, lim, x = long_setup(pkg, torch, n, h, 30)
    Ta, Tb, Tc = LENGTHS[(n, h)]["outn"]
    w, fb = WALK[(n, h)], fallback(n, h)
    want = {Ta: (w["stft"], w["istft_ola"]), Tb: (w["stft"], fb["istft_ola"]), Tc: (fb["stft"], fb["istft_ola"])}
    ys = {}
    for T in (Ta, Tb, Tc):
        xp = prefix(torch, x, T)
        spec = plan.stft(xp)
        ks = plan.last_launch()["kernels"]
        y = plan.istft_ola(spec)
        torch.cuda.synchronize()
        assert (ks, plan.last_launch()["kernels"]) == want[T], (n, h, T, ks, plan.last_launch())
        assert y.shape == (S, plan.output_length(T)) and finite(torch, y), (n, h, T)
        check_slices(oracle, xp, y, T, n, h, f"{n}/{h} istft(stft) T={T}")
        ys[T] = y
        del xp, spec
    for T in (Tb, Tc):
        assert_agree(torch, ys[Ta], ys[T], Ta - n, f"{n}/{h} istft(stft) T={Ta} vs T={T}")
    report_peak(torch, f"istft(stft) {n}/{h}")
    del x, ys, y
    torch.cuda.empty_cache()
