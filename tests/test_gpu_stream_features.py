"""Per-hop spectrogram features on the streaming path: crlot_stream_features_hop
(csrc/stream_feat.hip, the kHopFeat cut of stream_common.h) through
pkg.Stream.features_hop.

Yardsticks: the path's own stft_hop (the spectrum must be its row bit for bit),
the value contract of include/crlot_dsp.h restated in numpy by test_gpu_features
(power_of, np.sqrt, bands_restated, the float64 band sum, the float64 log), the
batched crlot_spectrogram on the same DROP, pairing-off plan, and push_hop_masked
for the analyse -> mask -> synthesise loop.

Shapes, channel count and inputs are test_gpu_stream_spectral's (every (E, S)
family of the register-resident body, both regimes of the any-shape body, a partly
filled last workgroup, NaN / Inf / sub-threshold / huge samples on channel 1).  The
huge sample overflows |X|^2 to +Inf on the frames that hold it, so band sums there
are +Inf or NaN; "bit for bit" below means: NaNs in the same places (the payload of
a NaN an invalid operation produces differs between the GPU and the host, and the
contract does not pin it) and every other value equal in all 32 bits.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_features import bands_restated, banks, power_of, spans_of, ulps
from test_gpu_parity import bits, host
from test_gpu_stream_spectral import ANY_SIZE, C_, RESIDENT, TOLERANCE, by_shape, case, cbits  # noqa: F401 (case: fixture)

pytestmark = pytest.mark.gpu

SHAPES = RESIDENT + ANY_SIZE
SENT = -7.0
CSENT = 7.0 + 3.0j
FLOOR = 1e-10


def same_bits(a, b):
    """NaNs in the same places, every other value equal in all 32 bits (module docstring)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def hop_of(c, q, channels=C_, interleaved=False):
    x = c.xd[:channels, q * c.h:(q + 1) * c.h]
    return x.t().contiguous() if interleaved else x.contiguous()


def run_feat(pkg, torch, c, f, with_spec=True, interleaved=False, channels=C_, pad=0, st=None):
    """features_hop over the whole signal on one object.  Checks hop by hop that
    emitted follows the DROP frame count and that a hop which emits nothing leaves the
    sentinel-filled out (and spec) untouched; the guard floats of padded rows keep the
    sentinel.  Returns (rows (channels, F, n_out), spectra (channels, F, bins) or None)."""
    st = st or pkg.Stream(c.plan, channels, interleaved=interleaved)
    rows, specs = [], []
    for q in range(c.hops):
        k = c.frame_of(q)
        big = torch.full((channels, f.n_out + pad), SENT, dtype=torch.float32, device="cuda")
        spec = torch.full((channels, c.bins), CSENT, dtype=torch.complex64, device="cuda") if with_spec else None
        out, em = st.features_hop(f, hop_of(c, q, channels, interleaved), out=big[:, :f.n_out], spec=spec)
        assert em == (1 if k >= 0 else 0), q
        assert out.data_ptr() == big.data_ptr()
        if em:
            rows.append(big)
            specs.append(spec)
        else:
            assert bool(torch.all(big == SENT)), q
            assert spec is None or bool(torch.all(spec == CSENT)), q
    assert len(rows) == c.F
    big = host(torch.stack(rows, dim=1))
    assert np.all(big[..., f.n_out:] == SENT)
    return big[..., :f.n_out].copy(), (host(torch.stack(specs, dim=1)) if with_spec else None)


def big_bank(bins):
    """Dense rows whose spans and weights exceed kFeatLdsBytes (8064): never staged in LDS."""
    rows = max(8, 8064 // (4 * bins) + 2)
    return np.random.default_rng(11).uniform(0.1, 1.0, (rows, bins)).astype(np.float32)


_store = {}


def per_bin(pkg, torch, c, kind):
    """(rows, spectra) of the per-bin LIN features of a case, with the spectrum: computed once."""
    key = (c.n, c.h, "bin", kind)
    if key not in _store:
        _store[key] = run_feat(pkg, torch, c, pkg.Features(c.plan, kind=kind))
    return _store[key]


def band_lin(pkg, torch, c, name, W, kind):
    key = (c.n, c.h, name, kind)
    if key not in _store:
        _store[key] = run_feat(pkg, torch, c, pkg.Features(c.plan, kind=kind, weights=W), with_spec=False)[0]
    return _store[key]


# ------------------------------------------------------------------ 1. per bin
@by_shape(SHAPES)
def test_per_bin_and_spectrum(pkg, torch_cuda, case):
    """The spectrum rows are a twin object's stft_hop rows, POWER is power_of(own
    spectrum), MAGNITUDE np.sqrt of it, all bit for bit; no NaN in POWER."""
    torch, c = torch_cuda, case
    p, spec = per_bin(pkg, torch, c, pkg.FEAT_POWER)
    m, spec_m = per_bin(pkg, torch, c, pkg.FEAT_MAGNITUDE)
    assert p.shape == m.shape == (C_, c.F, c.bins) and spec.shape == (C_, c.F, c.bins)
    twin = pkg.Stream(c.plan, C_)
    rows = []
    for q in range(c.hops):
        s, em = twin.stft_hop(hop_of(c, q))
        if em:
            rows.append(s.clone())
    want = host(torch.stack(rows, dim=1))
    assert np.array_equal(cbits(spec), cbits(want))
    assert np.array_equal(cbits(spec_m), cbits(want))
    ref = power_of(spec)
    assert not np.any(np.isnan(p))
    assert np.any(np.isinf(p[1])) and np.all(np.isfinite(p[0]))  # (the huge sample of channel 1)
    assert np.array_equal(bits(p), bits(ref))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(m), bits(np.sqrt(ref)))


# ------------------------------------------------------------------ 2. bands, LIN
@by_shape(SHAPES)
def test_bands_lin(pkg, torch_cuda, case):
    """Rows equal bands_restated(W, per-bin rows) bit for bit and lie within
    (width + 2) 2^-24 sum |w||v| of the float64 sum (where that sum is finite), for
    the three banks of test_gpu_features and one too large to be staged in LDS."""
    torch, c = torch_cuda, case
    todo = [(name, W, pkg.FEAT_POWER) for name, W in banks(pkg, c.n).items()]
    todo.append(("mel80_htk", todo[0][1], pkg.FEAT_MAGNITUDE))
    todo.append(("big", big_bank(c.bins), pkg.FEAT_POWER))
    assert todo[0][0] == "mel80_htk" and len(todo[2][1]) == 130
    for name, W, kind in todo:
        v = per_bin(pkg, torch, c, kind)[0]
        out = band_lin(pkg, torch, c, name, W, kind)
        lo, hi = spans_of(W)
        assert out.shape == (C_, c.F, len(W)), name
        if name == "big":
            assert 16 * len(W) + 4 * int(np.sum(hi - lo)) > 8064
        assert same_bits(out, bands_restated(W, v)), (name, kind)
        w64, v64 = W.astype(np.float64), v.astype(np.float64)
        fin = np.all(np.isfinite(v64), axis=-1)  # frames without the overflowed sample
        assert np.all(fin[0]) and np.any(fin[1]) and not np.all(fin[1])
        ref = v64[fin] @ w64.T
        bound = (hi - lo + 2)[None, :] * 2.0 ** -24 * (np.abs(v64[fin]) @ np.abs(w64).T)
        err = np.abs(out[fin].astype(np.float64) - ref)
        print(f"{c.n}/{c.h} {name} kind {kind}: max err / bound "
              f"{float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
        assert np.all(err <= bound), (name, kind, float(np.max(err / np.maximum(bound, 1e-300))))
        if name == "hand130":
            assert np.array_equal(bits(out[..., 2]), np.zeros(out.shape[:2], np.uint32))  # all-zero row: +0


# ------------------------------------------------------------------ 3. the batched entry
@by_shape([s for s in SHAPES if s not in TOLERANCE])
def test_equals_batched_spectrogram(pkg, torch_cuda, case):
    """The stacked rows are Features(plan).spectrogram(x)'s on the same plan: per bin,
    mel80_htk LIN and mel80_htk DB."""
    torch, c = torch_cuda, case
    W = banks(pkg, c.n)["mel80_htk"]
    fdb = pkg.Features(c.plan, weights=W, log=pkg.FEAT_DB, floor=FLOOR)
    got = {"bin": per_bin(pkg, torch, c, pkg.FEAT_POWER)[0],
           "lin": band_lin(pkg, torch, c, "mel80_htk", W, pkg.FEAT_POWER),
           "db": run_feat(pkg, torch, c, fdb, with_spec=False)[0]}
    want = {"bin": pkg.Features(c.plan), "lin": pkg.Features(c.plan, weights=W), "db": fdb}
    for what in got:
        ref = host(want[what].spectrogram(c.xd))
        assert ref.shape == got[what].shape == (C_, c.F, want[what].n_out), what
        assert same_bits(got[what], ref), what


# ------------------------------------------------------------------ 4. log modes
def nan_bank(bins):
    """Two rows; the first sums +Inf and -Inf on a frame whose |X|^2 overflowed: NaN."""
    W = np.zeros((2, bins), np.float32)
    W[0, 3:11] = 1.0
    W[0, 5] = -1.0
    W[1, 2:9] = 0.5
    return W


@by_shape([(512, 128), (2048, 512), (960, 240), (1024, 300)])
def test_log_modes(pkg, torch_cuda, case):
    """LN / LOG10 / DB within 4 float32 ulps of the float64 log of max(LIN output,
    floor) (the project's bar, test_gpu_features.test_log_modes); +Inf logs as +Inf, a
    NaN value as the floor."""
    torch, c = torch_cuda, case
    fl64 = np.float64(np.float32(FLOOR))
    cases = [("bin", None), ("mel80_htk", banks(pkg, c.n)["mel80_htk"]), ("nan", nan_bank(c.bins))]
    for name, W in cases:
        lin = (per_bin(pkg, torch, c, pkg.FEAT_POWER)[0] if W is None
               else band_lin(pkg, torch, c, name, W, pkg.FEAT_POWER)).astype(np.float64)
        nan, inf = np.isnan(lin), np.isposinf(lin)
        assert np.any(nan) == (name == "nan") and np.any(inf)
        with np.errstate(invalid="ignore"):
            m = np.where(nan, fl64, np.maximum(lin, fl64))
        fin = np.isfinite(m)
        for mode, ref in ((pkg.FEAT_LN, np.log(m)), (pkg.FEAT_LOG10, np.log10(m)), (pkg.FEAT_DB, 10.0 * np.log10(m))):
            f = pkg.Features(c.plan, weights=W, log=mode, floor=FLOOR)
            out = run_feat(pkg, torch, c, f, with_spec=False)[0]
            assert not np.any(np.isnan(out)), (name, mode)
            assert np.array_equal(np.isposinf(out), inf), (name, mode)
            u = ulps(out[fin], ref[fin])
            print(f"{c.n}/{c.h} {name} log mode {mode}: max {float(np.max(u)):.3f} ulp")
            assert np.all(u <= 4.0), (name, mode, float(np.max(u)))


# ------------------------------------------------------------------ 5. invariance
@by_shape(SHAPES)
def test_invariance(pkg, torch_cuda, case):
    """The same bits with and without a spectrum, for both PCM layouts, into padded
    rows (the guard floats keep their sentinel: run_feat), with one channel instead
    of five, and on a replay after reset()."""
    torch, c = torch_cuda, case
    W = banks(pkg, c.n)["mel80_htk"]
    for f, base in ((pkg.Features(c.plan), per_bin(pkg, torch, c, pkg.FEAT_POWER)[0]),
                    (pkg.Features(c.plan, weights=W), band_lin(pkg, torch, c, "mel80_htk", W, pkg.FEAT_POWER))):
        # (the stored rows: per bin with a spectrum, bands without)
        flip = run_feat(pkg, torch, c, f, with_spec=f.n_out != c.bins)[0]
        assert same_bits(flip, base), "spectrum given or not"
        assert same_bits(run_feat(pkg, torch, c, f, interleaved=True)[0], base), "interleaved PCM"
        assert same_bits(run_feat(pkg, torch, c, f, with_spec=False, pad=5)[0], base), "padded rows"
        one = run_feat(pkg, torch, c, f, channels=1)[0]
        assert one.shape[0] == 1 and same_bits(one[0], base[0]), "one channel"
        st = pkg.Stream(c.plan, C_)
        first = run_feat(pkg, torch, c, f, st=st)
        st.reset()
        again = run_feat(pkg, torch, c, f, st=st)
        assert same_bits(first[0], base) and same_bits(again[0], base), "reset and replay"
        assert np.array_equal(cbits(first[1]), cbits(again[1]))


# ------------------------------------------------------------------ 6. analyse -> mask -> synthesise
@by_shape(SHAPES)
def test_mask_loop_equals_push_hop_masked(pkg, torch_cuda, case):
    """features_hop(spec=...) -> a mask from the features -> istft_hop(spec, mask) gives,
    hop for hop and bit for bit, push_hop_masked with the same masks on a twin object.

    The mask is a Wiener-like gain p / (p + 1) of the per-bin power (0.5 where p
    overflowed) times a fixed de-emphasis ramp.  The ramp is there for a reason that
    has nothing to do with the feature entry: push_hop_masked and istft_hop o stft_hop
    (both older than it) agree bit for bit only while a block is not the residue of a
    total cancellation (the size of the effect fits the self-paired bin
    k = N/4, where the whole hop forms X[P-k] by its mirror formula and the split path
    reads the one stored X[k] for both, about 1e-16 |Z| apart; not confirmed further).
    On channel 1's frames with the 3e30 sample a mask with
    mask[k] == mask[P-k] -- a constant 0.5 here, and equally a row of ones -- cancels
    everything above that, and the blocks (1e12 against 3e30) then differ; measured with
    stft_hop in place of features_hop: 47 to 384 samples of channel 1 at 256/128,
    512/128, 2048/512, 1024/300 and 4096/1024, relative to the block's peak 1e-18 to
    1e-10, every other channel equal.  With the ramp (as with the gain ramp of
    test_gpu_stream_spectral's identity test) nothing cancels.  The symmetric mask is
    still run against a twin that takes the split path through stft_hop: the feature
    entry is a drop-in for the analysis half on every channel."""
    torch, c = torch_cuda, case
    f = pkg.Features(c.plan)
    split, whole, twin = pkg.Stream(c.plan, C_), pkg.Stream(c.plan, C_), pkg.Stream(c.plan, C_)
    sym = pkg.Stream(c.plan, C_)
    ones = torch.ones((C_, c.bins), dtype=torch.float32, device="cuda")
    ramp = torch.linspace(1.0, 0.25, c.bins, device="cuda")
    blocks = 0
    for q in range(c.hops):
        hop = hop_of(c, q)
        spec = torch.zeros((C_, c.bins), dtype=torch.complex64, device="cuda")
        feat, em = split.features_hop(f, hop, spec=spec)
        spec_t, et = twin.stft_hop(hop)
        _, es = sym.features_hop(f, hop, out=feat, spec=spec)
        assert em == et == es
        if not em:
            _, ew = whole.push_hop_masked(hop, ones)
            assert ew == 0, q
            continue
        wiener = torch.nan_to_num(feat / (feat + 1.0), nan=0.5).contiguous()  # in [0, 1], symmetric where p overflowed
        mask = (wiener * ramp).contiguous()
        blk = split.istft_hop(spec, mask)
        out, ew = whole.push_hop_masked(hop, mask)
        assert ew == c.h, q
        assert torch.equal(blk.view(torch.int32), out.view(torch.int32)), q
        assert torch.equal(sym.istft_hop(spec, wiener).view(torch.int32),
                           twin.istft_hop(spec_t, wiener).view(torch.int32)), q
        blocks += 1
    assert blocks == c.F


# ------------------------------------------------------------------ 7. modes and validation
@by_shape([(512, 128), (960, 240)])
def test_modes_and_validation(pkg, torch_cuda, case):
    torch, c = torch_cuda, case
    L = pkg.lib()
    f = pkg.Features(c.plan)
    p, spec = per_bin(pkg, torch, c, pkg.FEAT_POWER)
    # mixed with stft_hop on one object: one hop counter
    st = pkg.Stream(c.plan, C_)
    for q in range(c.hops):
        k = c.frame_of(q)
        if q % 2:
            out, em = st.features_hop(f, hop_of(c, q))
            if em:
                assert np.array_equal(bits(host(out)), bits(p[:, k])), q
        else:
            s, em = st.stft_hop(hop_of(c, q))
            if em:
                assert np.array_equal(cbits(host(s)), cbits(spec[:, k])), q
        assert em == (1 if k >= 0 else 0), q
    st.reset()
    # refused calls: CRLOT_EINVAL, nothing launched, no mode fixed, no counter moved
    other = pkg.Plan(frame_size=c.n, hop_size=c.h, boundary_mode=pkg.DROP, frame_pairing=False)
    fo = pkg.Features(other)
    hop = hop_of(c, 0)
    out = torch.full((C_, c.bins), SENT, dtype=torch.float32, device="cuda")
    sp = torch.full((C_, c.bins + 1), CSENT, dtype=torch.complex64, device="cuda")
    em = ctypes.c_int32(5)
    hp, op, spp, ld = hop.data_ptr(), out.data_ptr(), sp.data_ptr(), 2 * (c.bins + 1)

    def einval(rc, word=None):
        assert rc == pkg.EINVAL and em.value == 0, rc
        if word:
            assert word in L.crlot_last_error(), L.crlot_last_error()
        with pytest.raises(ValueError):
            pkg._check(rc)

    call = L.crlot_stream_features_hop
    einval(call(st._h, fo._h, hp, op, c.bins, None, 0, ctypes.byref(em), None), b"plan")
    einval(call(st._h, f._h, hp, op, c.bins - 1, None, 0, ctypes.byref(em), None), b"ld_feat")
    einval(call(st._h, f._h, hp, op, 0, None, 0, ctypes.byref(em), None), b"ld_feat")
    einval(call(st._h, f._h, hp, op, c.bins, spp + 4, ld, ctypes.byref(em), None), b"aligned")
    for bad_ld in (c.n + 3, c.n, 0):
        einval(call(st._h, f._h, hp, op, c.bins, spp, bad_ld, ctypes.byref(em), None), b"ld_spec")
    einval(call(None, f._h, hp, op, c.bins, None, 0, ctypes.byref(em), None))
    einval(call(st._h, None, hp, op, c.bins, None, 0, ctypes.byref(em), None))
    einval(call(st._h, f._h, None, op, c.bins, None, 0, ctypes.byref(em), None))
    einval(call(st._h, f._h, hp, None, c.bins, None, 0, ctypes.byref(em), None))
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENT)) and bool(torch.all(sp == CSENT))
    # the binding's own checks, before the C call
    for bad in (out.double(), out.cpu(), out[:, :-1], out[:-1], out.t().contiguous().t(),
                torch.zeros((C_, 2 * c.bins), device="cuda")[:, ::2], host(out)):
        with pytest.raises(ValueError):
            st.features_hop(f, hop, out=bad)
    with pytest.raises(ValueError):
        st.features_hop(fo, hop)
    with pytest.raises(ValueError):
        st.features_hop(f, hop, spec=sp[:, :c.bins].real)
    with pytest.raises(ValueError):
        st.features_hop(f, hop.double())
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENT))
    # (none of the refused calls fixed the split mode: a whole-hop call is still the object's first)
    # a whole-mode object refuses the entry until reset
    _, e0 = st.push_hop(hop)
    assert e0 == (c.h if c.frame_of(0) >= 0 else 0)
    with pytest.raises(RuntimeError, match="crlot_stream_reset"):
        st.features_hop(f, hop, out=out)
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENT))
    st.reset()
    # ld_spec is ignored without a spectrum
    assert call(st._h, f._h, hp, op, c.bins, None, 3, ctypes.byref(em), None) == 0
    st.reset()
    rows = run_feat(pkg, torch, c, f, st=st)[0]
    assert np.array_equal(bits(rows), bits(p))
    with pytest.raises(RuntimeError, match="crlot_stream_reset"):
        st.push_hop(hop)
    st.close()
    fo.close()
    other.close()
