"""GPU tests of crlot_resample (include/crlot_dsp.h, "resample / pitch shift").

Accuracy is checked against the float64 dot product with the library's own
float32 table (tests/resample_reference.py): |y - ref| <= gamma_K sum|h x| + 2^-149,
gamma_K = K 2^-24 / (1 - K 2^-24), the bound of a K-step fmaf chain (derived, not
measured).  Everything else is bit for bit: the two routes, the tiling, the
batch, the leading dimensions, the base alignment, the run."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import resample_reference as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 3
SHAPES = [(160, 147, 16, "hann"), (147, 160, 16, "kaiser"), (2, 1, 16, "hann"), (1, 2, 16, "hann"),
          (3, 1, 6, "hann"), (1, 3, 6, "kaiser"), (7, 5, 4, "hann"), (89, 84, 16, "hann"),
          (1, 64, 4, "hann"),       # K = 540: the any route, table in LDS
          (1021, 1024, 6, "hann")]  # U beyond one workgroup: the any route, table through L2
IDS = [f"{u}-{d}-z{z}-{w}" for u, d, z, w in SHAPES]

_resamplers = {}


def resampler(pkg, shape):
    if shape not in _resamplers:
        u, d, z, w = shape
        _resamplers[shape] = pkg.Resampler(u, d, zeros=z, window=w)
    r = _resamplers[shape]
    r.set_route("auto")
    r.set_tile(0)
    return r


@functools.lru_cache(maxsize=None)
def signal(T, n=S, seed=0):
    """White noise; from 200 samples on also a silent stretch, one sample at 1e12 and
    a run at 1e-12."""
    x = np.random.default_rng(1000 * seed + T).standard_normal((n, T)).astype(np.float32)
    if T >= 200:
        x[:, 50:90] = 0.0
        x[:, 120] = 1e12
        x[:, 140:170] = 1e-12
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(shape, T):
    u, d, z, w = shape
    U, D, W, K, _ = RR.geometry(u, d, z)
    tab = _resamplers[shape].table()
    return RR.resample(signal(T), U, D, W, tab)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def run(torch, r, x):
    y = r.resample(x)
    torch.cuda.synchronize()
    return y


def routes(r):
    return ("phase", "any") if r.info["phase_ok"] else ("any",)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_accuracy_vs_float64(pkg, torch_cuda, shape):
    torch = torch_cuda
    r = resampler(pkg, shape)
    K = r.taps
    worst = 0.0
    for T in (0, 1, 2, K - 1, 1000, 1777):
        x = torch.from_numpy(np.array(signal(T))).cuda()
        y = run(torch, r, x)
        L = r.output_length(T)
        assert y.shape == (S, L) and L == RR.output_length(T, r.up, r.down)
        if T == 0:
            continue
        ref, scale = reference(shape, T)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        bound = RR.fma_bound(K) * scale + 2.0 ** -149
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (shape, T, float((err / bound).max()))
        assert bool(torch.isfinite(y).all())
        name = r.last_launch()["name"]
        assert name == ("k_resample_phase" if r.info["phase_ok"] else "k_resample_any")
    print(f"{shape}: worst error {worst:.3f} of the fma-chain bound")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits_do_not_depend_on_route_tile_batch_or_layout(pkg, torch_cuda, shape):
    torch = torch_cuda
    r = resampler(pkg, shape)
    T = 1777
    L = r.output_length(T)
    x = torch.from_numpy(np.array(signal(T))).cuda()
    want = bits(run(torch, r, x))
    assert np.array_equal(bits(run(torch, r, x)), want)  # two calls in a row
    for route in routes(r):
        r.set_route(route)
        for tile in (1, 3, 0):
            r.set_tile(tile)
            got = bits(run(torch, r, x))
            rec = r.last_launch()
            assert rec["name"] == "k_resample_" + route, rec
            if tile:
                assert 1 <= rec["tile_outputs"] <= tile * r.up, rec  # (several seams at this length)
                assert rec["grid"] == S * -(-L // rec["tile_outputs"]), rec
                assert tile != 1 or rec["grid"] > S, rec
            assert np.array_equal(got, want), (route, tile)
    r.set_route("auto")
    r.set_tile(0)
    # a stream alone against the same stream in a batch of 5 at another position
    big = torch.from_numpy(np.array(signal(T, 5, seed=1))).cuda()
    big[3] = x[1]
    assert np.array_equal(bits(run(torch, r, big))[3], want[1])
    assert np.array_equal(bits(run(torch, r, x[1:2]))[0], want[1])
    # padded leading dimensions, and base pointers one float off the allocation
    xp = torch.full((S, T + 13), float("nan"), device="cuda")
    xp[:, :T] = x
    yp = torch.zeros((S, L + 7), device="cuda")
    r.resample(xp[:, :T], yp[:, :L])
    torch.cuda.synchronize()
    assert np.array_equal(bits(yp[:, :L].contiguous()), want)
    xo = torch.empty(S * T + 1, device="cuda")[1:].view(S, T)
    xo.copy_(x)
    yo = torch.empty(S * L + 1, device="cuda")[1:].view(S, L)
    assert xo.data_ptr() % 8 != x.data_ptr() % 8
    r.resample(xo, yo)
    torch.cuda.synchronize()
    assert np.array_equal(bits(yo), want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bad_samples_are_zeros(pkg, torch_cuda, shape):
    """NaN, +-Inf and 1e-35 give the bits of the same input with zeros in their place."""
    torch = torch_cuda
    r = resampler(pkg, shape)
    T = 1000
    clean = np.array(signal(T))
    dirty = clean.copy()
    for k, v in ((0, np.nan), (7, np.inf), (333, -np.inf), (334, 1e-35), (600, -1e-35), (T - 1, np.nan)):
        clean[:, k] = 0.0
        dirty[:, k] = v
    for route in routes(r):
        r.set_route(route)
        a = run(torch, r, torch.from_numpy(clean).cuda())
        b = run(torch, r, torch.from_numpy(dirty).cuda())
        assert bool(torch.isfinite(b).all())
        assert np.array_equal(bits(a), bits(b)), route


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_containment(pkg, torch_cuda, shape):
    """NaN guard bands before, after and between the output rows stay untouched; NaN
    behind each input row never reaches an output."""
    torch = torch_cuda
    r = resampler(pkg, shape)
    nan = float("nan")
    for T in (1, r.taps - 1, 1777):
        L = r.output_length(T)
        ld_x, ld_y, G = T + 64, L + 37, 256
        xb = torch.full((S, ld_x), nan, device="cuda")
        xb[:, :T] = torch.from_numpy(np.array(signal(T))).cuda()
        for route in routes(r):
            r.set_route(route)
            for tile in (0, 1):
                r.set_tile(tile)
                buf = torch.full((G + S * ld_y + G,), nan, device="cuda")
                rows = buf[G:G + S * ld_y].view(S, ld_y)
                r.resample(xb[:, :T], rows[:, :L])
                torch.cuda.synchronize()
                assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + S * ld_y:]).all())
                assert bool(torch.isnan(rows[:, L:]).all())
                assert bool(torch.isfinite(rows[:, :L]).all()), (T, route, tile)
                if T > 1:
                    ref, scale = reference(shape, T)
                    err = np.abs(rows[:, :L].cpu().numpy().astype(np.float64) - ref)
                    assert np.all(err <= RR.fma_bound(r.taps) * scale + 2.0 ** -149)


def test_oboe_44k1_to_48k(pkg, torch_cuda):
    """The reference demo's case: oboe.wav from 44.1 kHz to 48 kHz."""
    torch = torch_cuda
    x, sr = pkg.load_wav_mono(os.path.join(ROOT, "tests", "golden", "oboe.wav"))
    assert sr == 44100 and x.dtype == np.float32
    r = pkg.Resampler(48000, 44100)
    assert (r.up, r.down, r.taps) == (160, 147, 34)
    y = run(torch, r, torch.from_numpy(x).cuda())
    L = r.output_length(len(x))
    assert y.shape == (L,) and L == -(-len(x) * 160 // 147)
    ref, scale = RR.resample(x, 160, 147, r.half_width, r.table())
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    bound = RR.fma_bound(r.taps) * scale + 2.0 ** -149
    print(f"oboe: worst error {float((err / bound).max()):.3f} of the fma-chain bound")
    assert np.all(err <= bound)
    assert float(np.abs(ref).max()) > 0.05 and r.last_launch()["name"] == "k_resample_phase"


def test_argument_checks(pkg, torch_cuda):
    torch = torch_cuda
    L = pkg.lib()
    r = resampler(pkg, SHAPES[0])
    T = 1000
    Lo = r.output_length(T)
    x = torch.zeros((2, T), device="cuda")
    y = torch.zeros((2, Lo), device="cuda")

    def call(px, py, n, t, ld_x, ld_y):
        return L.crlot_resample(r._h, px, py, n, t, ld_x, ld_y, None)

    assert call(x.data_ptr(), y.data_ptr(), 2, T, T, Lo) == pkg.OK
    assert call(x.data_ptr(), y.data_ptr(), 2, T, T - 1, Lo) == pkg.EINVAL   # ld_x < T
    assert call(x.data_ptr(), y.data_ptr(), 1, T, T - 1, Lo) == pkg.EINVAL   # ... for one stream too
    assert call(x.data_ptr(), y.data_ptr(), 2, T, T, Lo - 1) == pkg.EINVAL   # ld_y < L
    assert call(x.data_ptr(), y.data_ptr(), 1, T, T, 0) == pkg.OK            # one stream: ld_y unused
    assert call(x.data_ptr(), x.data_ptr(), 1, T, T, Lo) == pkg.EINVAL       # the same buffer
    assert call(x.data_ptr(), x.data_ptr() + 4 * (T - 1), 1, T, T, Lo) == pkg.EINVAL  # one float shared
    assert call(y.data_ptr() + 4 * Lo, y.data_ptr(), 1, T, T, Lo) == pkg.OK  # adjacent
    # empty calls write nothing
    guard = torch.full((2, Lo), 7.0, device="cuda")
    assert call(x.data_ptr(), guard.data_ptr(), 0, T, T, Lo) == pkg.OK
    assert call(x.data_ptr(), guard.data_ptr(), 2, 0, T, Lo) == pkg.OK
    torch.cuda.synchronize()
    assert bool((guard == 7.0).all())
    # the route knob: the phase kernel on a shape it cannot take
    long = resampler(pkg, SHAPES[8])
    with pytest.raises(NotImplementedError):
        long.set_route("phase")
    for route in routes(r):
        r.set_route(route)
        run(torch, r, x)
        assert r.last_launch()["name"] == "k_resample_" + route
        assert r.last_launch()["kernel"] == {"phase": 37, "any": 38}[route]
    r.set_route("auto")
