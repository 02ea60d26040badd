"""GPU tests of the fused spectrogram features (crlot_spectrogram, feat.hip),
pinned to the project's own crlot_stft: the value contract of
include/crlot_dsp.h ("spectrogram features") restated.

1 per bin: bit for bit float32(float32(re re) + float32(im im)) of Plan.stft under
  the same pairing setting, and np.sqrt of it; also with NaN / Inf / denormal /
  huge samples;
2 routing: k_pair_feat / k_feat where crlot_stft runs k_pair_stft (N = 1024) /
  k_stft (N <= 1024), the staged k_feat_step elsewhere;
3 bands: within (width + 2) 2^-24 sum |w||v| of the float64 sum over the span, and
  bit for bit the documented summation order restated in numpy float32 (the
  check that the walkers and the staged form agree: no public switch forces the
  staged form at a walker's shape);
4 determinism over chunking, batch, leading dimensions and streams;
5 log modes within 4 float32 ulps of the float64 log of the LIN output;
6 edges.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import bits, dev, host
from test_gpu_stft import special

pytestmark = pytest.mark.gpu

PAIR = [(1024, 256), (1024, 512), (1024, 128)]
WAVE = [(512, 128), (256, 128), (1024, 300)]
STAGED = [(2048, 512), (960, 240)]
SHAPES = PAIR + WAVE + STAGED
MODES = [0, 1, 2]  # ZERO_PAD, DROP, FRAMEQUEUE (centre, reflect)
S = 3


def make_plan(pkg, n, h, mode=0, pairing=True):
    kw = dict(center=True, pad_mode=pkg.PAD_REFLECT) if mode == 2 else {}
    plan = pkg.Plan(frame_size=n, hop_size=h, boundary_mode=mode, **kw)
    plan.set_frame_pairing(pairing)
    return plan


def streams(oracle, n, s=S, T=None):
    return oracle.synth_streams(s, 9 * n + 77 if T is None else T, config_id=71)


def power_of(spec):
    """float32(float32(re re) + float32(im im)) of a complex64 array."""
    f = np.ascontiguousarray(spec, np.complex64).view(np.float32).reshape(spec.shape + (2,))
    re, im = f[..., 0], f[..., 1]
    with np.errstate(over="ignore", invalid="ignore"):
        return (re * re) + (im * im)  # float32 arrays: every product and the sum round to float32


def hand_bank(bins):
    """130 rows (more than two rounds of 64): a width-1 band on bin N/2 and on bin 0,
    an all-zero row, a dense row over every bin, negative weights, and random spans."""
    rng = np.random.default_rng(5)
    W = np.zeros((130, bins), np.float32)
    W[0, bins - 1] = 1.25
    W[1, 0] = 0.75
    # row 2: all zero
    W[3, :] = rng.uniform(0.1, 1.0, bins).astype(np.float32)
    W[4, 5:40] = -rng.uniform(0.1, 1.0, 35).astype(np.float32)
    for j in range(5, 130):
        lo = int(rng.integers(0, bins - 1))
        hi = int(rng.integers(lo + 1, min(bins, lo + 70) + 1))
        W[j, lo:hi] = rng.uniform(-1.0, 1.0, hi - lo).astype(np.float32)
        if hi - lo > 4:
            W[j, lo + 2] = 0.0  # an interior zero stays inside the span
    return W


def banks(pkg, n):
    bins = n // 2 + 1
    return {"mel80_htk": pkg.mel_filterbank(80, n, 16000.0),
            "mel40_slaney_norm": pkg.mel_filterbank(40, n, 16000.0, 20.0, 7600.0, pkg.MEL_SLANEY, True),
            "hand130": hand_bank(bins)}


def spans_of(W):
    lo, hi = np.zeros(len(W), int), np.zeros(len(W), int)
    for j, w in enumerate(W):
        nz = np.flatnonzero(w)
        if nz.size:
            lo[j], hi[j] = nz[0], nz[-1] + 1
    return lo, hi


def bands_restated(W, V):
    """The documented summation order in numpy float32: part g = span offset mod 8
    adds fl(w v) in ascending offset from +0; ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7))."""
    lo, hi = spans_of(W)
    out = np.zeros(V.shape[:-1] + (len(W),), np.float32)
    for j in range(len(W)):
        t = W[j, lo[j]:hi[j]] * V[..., lo[j]:hi[j]]  # float32 products
        s = []
        for g in range(8):
            acc = np.zeros(V.shape[:-1], np.float32)
            for i in range(g, hi[j] - lo[j], 8):
                acc = acc + t[..., i]
            s.append(acc)
        out[..., j] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))
    return out


# ------------------------------------------------------------------ 1: per bin, bit exact
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,h", SHAPES)
def test_per_bin_bit_exact_vs_stft(pkg, oracle, torch_cuda, n, h, mode):
    torch = torch_cuda
    x0 = streams(oracle, n)
    for pairing in (True, False):
        plan = make_plan(pkg, n, h, mode, pairing)
        fp = pkg.Features(plan, kind=pkg.FEAT_POWER)
        fm = pkg.Features(plan, kind=pkg.FEAT_MAGNITUDE)
        assert fp.n_out == n // 2 + 1 and fp.widest_band == 0
        for what, x in (("plain", x0), ("special", special(x0))):
            xd = dev(torch, x)
            ref = power_of(host(plan.stft(xd)))
            p = host(fp.spectrogram(xd))
            m = host(fm.spectrogram(xd))
            assert p.shape == ref.shape == (S, plan.frame_count(x.shape[1]), n // 2 + 1)
            assert np.array_equal(bits(p), bits(ref)), (n, h, mode, pairing, what, "power")
            with np.errstate(invalid="ignore"):
                assert np.array_equal(bits(m), bits(np.sqrt(ref))), (n, h, mode, pairing, what, "magnitude")
            if what == "special":
                assert not np.any(np.isnan(p))  # (the forward's input is sanitized; a huge sample overflows to +Inf)
        fp.close()
        fm.close()
        plan.close()


# ------------------------------------------------------------------ 2: routing
def test_routing(pkg, oracle, torch_cuda):
    """The walkers run exactly where crlot_stft itself runs k_pair_stft at N = 1024 or
    k_stft at N <= 1024 (so the spectrum is crlot_stft's bit for bit); every other
    route of crlot_stft -- N = 2048, the mixed-radix sizes, and N = 512 with pairing
    on, whose stft is k_pair512_stft -- takes the staged form."""
    torch = torch_cuda

    def kernels(n, h, pairing):
        plan = make_plan(pkg, n, h, 0, pairing)
        xd = dev(torch, streams(oracle, n))
        plan.stft(xd)
        stft_k = plan.last_launch()["kernels"]
        f = pkg.Features(plan)
        f.spectrogram(xd)
        return stft_k, plan.last_launch()["kernels"]

    for n, h in PAIR:
        assert kernels(n, h, True) == (["k_pair_stft"], ["k_pair_feat"])
        assert kernels(n, h, False) == (["k_stft"], ["k_feat"])
    for n, h in WAVE:
        assert kernels(n, h, False) == (["k_stft"], ["k_feat"])
    for n, h in [(256, 128), (1024, 300)]:
        assert kernels(n, h, True) == (["k_stft"], ["k_feat"])
    stft_k, feat_k = kernels(512, 128, True)  # (no frame-pair feature walker at N = 512)
    assert stft_k == ["k_pair_stft"] and feat_k == ["k_pair_stft", "k_feat_step"]
    for n, h in STAGED:
        for pairing in (True, False):
            stft_k, feat_k = kernels(n, h, pairing)
            assert feat_k == stft_k + ["k_feat_step"], (n, h, pairing, feat_k)


# ------------------------------------------------------------------ 3: bands
# (n, h, pairing): every shape under the default pairing, and with pairing off the shapes
# whose default route is not the per-wave walker -- k_feat<4> at (512, 128), whose stft
# under pairing is k_pair512_stft (the staged form), and k_feat<8> at the three pair hops
BAND_CASES = [(n, h, True) for n, h in SHAPES] + [(n, h, False) for n, h in [(512, 128)] + PAIR]


def expected_route(n, h, pairing):
    if (n, h) in PAIR:
        return "k_pair_feat" if pairing else "k_feat"
    if (n, h) in WAVE and not (pairing and n == 512):
        return "k_feat"
    return "k_feat_step"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,h,pairing", BAND_CASES)
def test_bands_vs_float64_and_restated_order(pkg, oracle, torch_cuda, n, h, pairing, mode):
    torch = torch_cuda
    plan = make_plan(pkg, n, h, mode, pairing)
    xd = dev(torch, streams(oracle, n))
    per_bin = {kind: host(pkg.Features(plan, kind=kind).spectrogram(xd))
               for kind in (pkg.FEAT_POWER, pkg.FEAT_MAGNITUDE)}
    assert np.all(np.isfinite(per_bin[pkg.FEAT_POWER]))
    for name, W in banks(pkg, n).items():
        lo, hi = spans_of(W)
        for kind in ((pkg.FEAT_POWER, pkg.FEAT_MAGNITUDE) if name == "mel80_htk" else (pkg.FEAT_POWER,)):
            f = pkg.Features(plan, kind=kind, weights=W)
            assert f.n_out == len(W) and f.widest_band == int(np.max(hi - lo))
            out = host(f.spectrogram(xd))
            route = expected_route(n, h, pairing)
            launched = plan.last_launch()["kernels"]
            assert launched == [route] if route != "k_feat_step" else launched[-1] == route, (launched, route)
            v = per_bin[kind]
            assert out.shape == v.shape[:2] + (len(W),)
            w64, v64 = W.astype(np.float64), v.astype(np.float64)
            ref = v64 @ w64.T                       # (zeros outside the span add nothing)
            mag = np.abs(v64) @ np.abs(w64).T
            bound = (hi - lo + 2)[None, None, :] * 2.0 ** -24 * mag
            err = np.abs(out.astype(np.float64) - ref)
            assert np.all(err <= bound), (name, kind, float(np.max(err / np.maximum(bound, 1e-300))))
            if name == "hand130":
                assert np.array_equal(bits(out[..., 2]), np.zeros(out.shape[:2], np.uint32))  # all-zero row: +0
            assert np.array_equal(bits(out), bits(bands_restated(W, v))), (name, kind)
            f.close()
    plan.close()


# ------------------------------------------------------------------ 4: determinism
@pytest.mark.parametrize("n,h,pairing", [(1024, 256, True), (1024, 256, False), (1024, 300, True), (512, 128, False),
                                         (512, 128, True), (2048, 512, True)])
def test_determinism(pkg, oracle, torch_cuda, n, h, pairing):
    torch = torch_cuda
    plan = make_plan(pkg, n, h, 0, pairing)
    x = streams(oracle, n)
    xd = dev(torch, x)
    W = banks(pkg, n)["mel80_htk"]
    for f in (pkg.Features(plan), pkg.Features(plan, weights=W, log=pkg.FEAT_DB, floor=1e-10)):
        base = host(f.spectrogram(xd))
        route = expected_route(n, h, pairing)
        launched = plan.last_launch()["kernels"]
        assert launched == [route] if route != "k_feat_step" else launched[-1] == route, (launched, route)
        walker = route != "k_feat_step"
        # chunking (the walkers; n_chunks as crlot_stft reports it under the same knob)
        seen = set()
        for c in (1, 2, 3, 7):
            plan.set_chunks(c)
            out = host(f.spectrogram(xd))
            nc = plan.last_launch()["n_chunks"]
            plan.stft(xd)
            assert nc == plan.last_launch()["n_chunks"], (c, nc)
            seen.add(nc)
            assert np.array_equal(bits(out), bits(base)), ("chunks", c)
        plan.set_chunks(0)
        if walker:
            assert len(seen) == 4, seen
        # one stream against row 0 of three
        one = host(f.spectrogram(xd[:1].contiguous()))
        assert np.array_equal(bits(one[0]), bits(base[0]))
        assert np.array_equal(bits(host(f.spectrogram(xd[0]))), bits(base[0]))  # 1-D input
        # padded leading dimensions; the padding keeps its sentinel
        F, no = base.shape[1], base.shape[2]
        big = torch.full((S, F + 2, no + 5), -7.0, dtype=torch.float32, device=xd.device)
        f.spectrogram(xd, out=big[:, :F, :no])
        bigh = host(big)
        assert np.array_equal(bits(bigh[:, :F, :no]), bits(base))
        assert np.all(bigh[:, F:, :] == -7.0) and np.all(bigh[:, :, no:] == -7.0)
        # a non-default HIP stream
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            out = f.spectrogram(xd)
            assert plan.last_launch()["kernels"][-1] == route
        st.synchronize()
        assert np.array_equal(bits(host(out)), bits(base))
        # run to run
        assert np.array_equal(bits(host(f.spectrogram(xd))), bits(base))


# ------------------------------------------------------------------ 5: log modes
def ulps(out, ref64):
    ref32 = ref64.astype(np.float32)
    return np.abs(out.astype(np.float64) - ref64) / np.spacing(np.abs(ref32)).astype(np.float64)


@pytest.mark.parametrize("n,h", [(1024, 256), (1024, 300), (2048, 512)])
def test_log_modes(pkg, oracle, torch_cuda, n, h):
    """LN / LOG10 / DB against the float64 log of max(LIN output, floor): 4 float32 ulps of
    the reference value (logf / log10f are documented at 1-2 ulp; DB adds one rounding)."""
    torch = torch_cuda
    plan = make_plan(pkg, n, h)
    x = streams(oracle, n)
    x[2] = 0.0  # a silent stream: exactly log(floor)
    xd = dev(torch, x)
    floor = 1e-10
    fl32 = np.float64(np.float32(floor))
    worst = 0.0
    for W in (None, banks(pkg, n)["mel80_htk"]):
        lin = host(pkg.Features(plan, weights=W).spectrogram(xd)).astype(np.float64)
        assert np.all(lin[2] == 0.0)
        m = np.maximum(lin, fl32)
        for mode, ref in ((pkg.FEAT_LN, np.log(m)), (pkg.FEAT_LOG10, np.log10(m)), (pkg.FEAT_DB, 10.0 * np.log10(m))):
            out = host(pkg.Features(plan, weights=W, log=mode, floor=floor).spectrogram(xd))
            u = ulps(out, ref)
            worst = max(worst, float(np.max(u)))
            print(f"log mode {mode} bands {W is not None} N={n} H={h}: max {float(np.max(u)):.3f} ulp")
            assert np.all(u <= 4.0), (mode, float(np.max(u)))
            assert np.all(ulps(out[2], ref[2]) <= 4.0)
    print(f"largest ulp distance N={n} H={h}: {worst:.3f}")
    with pytest.raises(ValueError):
        pkg.Features(plan, log=pkg.FEAT_DB, floor=0.0)       # below FLT_MIN
    with pytest.raises(ValueError):
        pkg.Features(plan, log=pkg.FEAT_LN, floor=float("inf"))
    with pytest.raises(ValueError):
        pkg.Features(plan, log=7)
    with pytest.raises(ValueError):
        pkg.Features(plan, kind=2)


# ------------------------------------------------------------------ 6: edges
def test_edges(pkg, oracle, torch_cuda):
    torch = torch_cuda
    n, h = 1024, 256
    plan = make_plan(pkg, n, h)
    bins = n // 2 + 1
    W = banks(pkg, n)["mel80_htk"]
    fb, fw = pkg.Features(plan), pkg.Features(plan, weights=W)
    # an odd frame count: the pair walker's lone last frame
    x = streams(oracle, n)
    xd = dev(torch, x)
    assert plan.frame_count(x.shape[1]) % 2 == 1
    out = host(fb.spectrogram(xd))
    assert plan.last_launch()["kernels"] == ["k_pair_feat"]
    assert np.array_equal(bits(out), bits(power_of(host(plan.stft(xd)))))
    outw = host(fw.spectrogram(xd))
    assert np.array_equal(bits(outw), bits(bands_restated(W, out)))
    # one stream, one frame
    x1 = dev(torch, streams(oracle, n, 1, 100))
    assert plan.frame_count(100) == 1
    o1 = host(fb.spectrogram(x1))
    assert o1.shape == (1, 1, bins) and np.array_equal(bits(o1), bits(power_of(host(plan.stft(x1)))))
    assert np.array_equal(bits(host(fw.spectrogram(x1))), bits(bands_restated(W, o1)))
    # T = 0
    assert tuple(fb.spectrogram(torch.zeros((S, 0), dtype=torch.float32, device=xd.device)).shape) == (S, 0, bins)
    # DROP with T = N - 1: no frame, CRLOT_OK, output untouched
    drop = make_plan(pkg, n, h, 1)
    fd = pkg.Features(drop)
    assert drop.frame_count(n - 1) == 0
    sent = torch.full((S, 2 * bins), -3.0, dtype=torch.float32, device=xd.device)
    L = pkg.lib()
    rc = L.crlot_spectrogram(fd._h, xd.data_ptr(), sent.data_ptr(), S, n - 1, x.shape[1], 2 * bins, bins, None)
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.all(sent == -3.0))
    assert drop.last_launch()["n_kernels"] == 0
    # ld_frame < n_out: CRLOT_EINVAL from the C entry, ValueError from the binding
    rc = L.crlot_spectrogram(fb._h, xd.data_ptr(), sent.data_ptr(), 1, 100, 100, bins, bins - 1, None)
    assert rc == pkg.EINVAL and b"ld_frame" in L.crlot_last_error()
    F = plan.frame_count(x.shape[1])
    flat = torch.zeros(S * F * bins, dtype=torch.float32, device=xd.device)
    with pytest.raises(ValueError):
        fb.spectrogram(xd, out=flat.as_strided((S, F, bins), (F * bins, bins - 1, 1)))
    with pytest.raises(ValueError):
        fb.spectrogram(xd, out=torch.zeros((S, F, bins + 1), dtype=torch.float32, device=xd.device))
    # a non-finite weight, a weight matrix without its n_bands and the reverse
    for bad in (np.nan, np.inf):
        Wb = W.copy()
        Wb[3, 17] = bad
        with pytest.raises(ValueError):
            pkg.Features(plan, weights=Wb)
    with pytest.raises(ValueError):
        pkg.Features(plan, weights=np.zeros((513, bins), np.float32))  # n_bands > 512
    h_ = C.c_void_p()
    d = pkg.FeaturesDesc(0, 4, 0, 0.0)
    assert L.crlot_features_create(plan._h, C.byref(d), None, C.byref(h_)) == pkg.EINVAL
    d = pkg.FeaturesDesc(0, 0, 0, 0.0)
    assert L.crlot_features_create(plan._h, C.byref(d), W.ctypes.data, C.byref(h_)) == pkg.EINVAL
    # two objects on one plan used alternately, and one destroyed before the plan
    a, b = pkg.Features(plan, weights=W), pkg.Features(plan, kind=pkg.FEAT_MAGNITUDE)
    ra, rb = host(a.spectrogram(xd)), host(b.spectrogram(xd))
    for _ in range(2):
        assert np.array_equal(bits(host(a.spectrogram(xd))), bits(ra))
        assert np.array_equal(bits(host(b.spectrogram(xd))), bits(rb))
    assert np.array_equal(bits(ra), bits(outw))
    a.close()
    assert np.array_equal(bits(host(b.spectrogram(xd))), bits(rb))
    for f in (b, fb, fw, fd):
        f.close()
    torch.cuda.synchronize()
    plan.close()
    drop.close()
