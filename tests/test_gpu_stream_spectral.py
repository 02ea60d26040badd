"""The spectral step on the per-hop streaming path: crlot_stream_stft_hop,
crlot_stream_istft_hop and crlot_stream_push_hop_masked (csrc/stream_spec.hip)
through pkg.Stream.

Yardsticks: the batched entries on a per-frame plan (boundary_mode=DROP,
frame_pairing=False) -- Plan.stft, Plan.istft_ola and Plan.roundtrip with the
same gain and mask -- the per-hop path's own push_hop, and the oracle's masked
loop (or_roundtrip_mask).

Bit identity with the batched entries holds where the batched kernel runs the
transform the hop kernel runs.  Two shapes have a weaker batched yardstick
(TOLERANCE below), known from which kernels the library dispatches, and are held
to the FFT tolerance (assert_close / assert_spec_close) there:
  4096/1024  the hop path transforms with the mixed-radix wave FFT (fft_any.h), the
             batched entries with the workgroup Stockham kernels;
  1024/300   N % H != 0 sends the hop path to the mixed-radix kernel as well, while
             the batched entries at N = 1024 keep the one-wave Stockham transform
             (test_stream_any_shape compares bits only for non-power-of-two N for
             the same reason).
The identities inside the per-hop path (masked == istft(stft), ones / no mask ==
push_hop, reset replays) are bit-exact at every shape.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import assert_close, bits, dev, host
from test_gpu_stft import assert_spec_close, finite_scale

pytestmark = pytest.mark.gpu

C_ = 5  # the last workgroup (4 or 8 waves) is partly filled
RESIDENT = [(256, 128), (512, 128), (1024, 256), (1024, 1024), (2048, 512)]
ANY_SIZE = [(960, 240), (882, 441), (480, 120), (1024, 300), (4096, 1024)]
SHAPES = RESIDENT + ANY_SIZE
TOLERANCE = {(4096, 1024), (1024, 300)}  # batched yardstick within the FFT tolerance (module docstring)


def frames_after(hops, n, h):
    """Frames a DROP Framer has produced after `hops` hops of h samples."""
    t = hops * h
    return (t - n) // h + 1 if t >= n else 0


def cbits(z):
    """Bit pattern of complex64 data."""
    return np.ascontiguousarray(z, np.complex64).view(np.uint32)


class Case:
    """Inputs of one shape, the plan and the batched yardsticks: built once, read-only."""

    def __init__(self, pkg, oracle, torch, n, h):
        self.n, self.h = n, h
        self.bins = n // 2 + 1
        self.hops = 3 * -(-n // h) + 2
        self.T = self.hops * h
        self.F = frames_after(self.hops, n, h)
        x = oracle.synth_streams(C_, self.T, config_id=n + h)
        # channel 1: a NaN burst, +-Inf, a sub-threshold stretch and one huge sample, all inside the first 2N samples
        x[1, n // 8:n // 8 + 5] = np.nan
        x[1, n // 2] = np.inf
        x[1, n // 2 + 7] = -np.inf
        x[1, n:n + n // 4] = 1e-35
        x[1, n + n // 2 + 3] = 3e30
        self.x = x
        self.xd = dev(torch, x)
        rng = np.random.default_rng(1000 * n + h)
        m = rng.uniform(-1.5, 1.5, (C_, self.F, self.bins)).astype(np.float32)
        m[..., ::17] = 0.0
        self.mask = m                      # per channel and frame
        self.mask_shared = m[0].copy()     # one row per frame
        self.maskd = dev(torch, m)
        self.mask_shared_d = dev(torch, self.mask_shared)
        self.gain = np.linspace(1.0, 0.25, self.bins).astype(np.float32)
        self.plan = pkg.Plan(frame_size=n, hop_size=h, boundary_mode=pkg.DROP, frame_pairing=False)
        self.spec = self.plan.stft(self.xd)  # (C, F, bins) complex64, before the gain
        self.exact = (n, h) not in TOLERANCE

    def hop(self, torch, q, interleaved=False):
        hop = self.xd[:, q * self.h:(q + 1) * self.h]
        return hop.t().contiguous() if interleaved else hop.contiguous()

    def frame_of(self, q):
        """Frame completed by hop q, or -1."""
        a, b = frames_after(q + 1, self.n, self.h), frames_after(q, self.n, self.h)
        return a - 1 if a > b else -1

    def batched(self, torch, call, gain=False, mask=None):
        """A batched entry on the plan with the step set, then cleared."""
        self.plan.set_spectral_gain(self.gain if gain else None)
        self.plan.set_spectral_mask(mask)
        try:
            y = host(call())
        finally:
            self.plan.set_spectral_mask(None)
            self.plan.set_spectral_gain(None)
        return y


_cases = {}


@pytest.fixture
def case(request, pkg, oracle, torch_cuda):
    key = request.param
    if key not in _cases:
        _cases[key] = Case(pkg, oracle, torch_cuda, *key)
    return _cases[key]


def by_shape(shapes=SHAPES):
    return pytest.mark.parametrize("case", shapes, indirect=True, ids=[f"{n}-{h}" for n, h in shapes])


def planar(o, interleaved):
    o = host(o)
    return (o.T if interleaved else o).copy()


def run_masked(pkg, torch, c, mask_rows, interleaved=False, st=None):
    """push_hop_masked over the whole signal; mask_rows(k) -> the row tensor of frame k (or None).
    Returns the blocks, (C, F*H)."""
    st = st or pkg.Stream(c.plan, C_, interleaved=interleaved)
    outs = []
    for q in range(c.hops):
        k = c.frame_of(q)
        out, em = st.push_hop_masked(c.hop(torch, q, interleaved), mask_rows(max(k, 0)))
        assert em == (c.h if k >= 0 else 0), q
        if em:
            outs.append(planar(out, interleaved))
    return np.concatenate(outs, axis=1)


def run_plain(pkg, torch, c, interleaved=False):
    st = pkg.Stream(c.plan, C_, interleaved=interleaved)
    outs = []
    for q in range(c.hops):
        out, em = st.push_hop(c.hop(torch, q, interleaved))
        if em:
            outs.append(planar(out, interleaved))
    return np.concatenate(outs, axis=1)


# ------------------------------------------------------------------ 1. stft_hop rows
@by_shape()
def test_stft_hop_rows_equal_batched_stft(pkg, torch_cuda, case):
    """emitted follows the DROP frame count hop by hop, a hop that emits nothing
    leaves d_spec untouched, and the rows are Plan.stft's (bit for bit; TOLERANCE
    shapes within the FFT tolerance, module docstring)."""
    torch, c = torch_cuda, case
    st = pkg.Stream(c.plan, C_)
    rows = []
    for q in range(c.hops):
        k = c.frame_of(q)
        sentinel = torch.full((C_, c.bins), 7.0 + 3.0j, dtype=torch.complex64, device="cuda")
        spec, em = st.stft_hop(c.hop(torch, q), sentinel)
        assert em == (1 if k >= 0 else 0), q
        if em:
            rows.append(host(spec).copy())
        else:
            assert np.all(host(spec) == np.complex64(7.0 + 3.0j)), q
    got = np.stack(rows, axis=1)
    want = host(c.spec)
    assert got.shape == want.shape == (C_, c.F, c.bins)
    assert np.all(got[..., 0].imag == 0) and np.all(got[..., -1].imag == 0)  # DC / Nyquist
    if c.exact:
        assert np.array_equal(cbits(got), cbits(want))
    else:
        for s in range(C_):
            assert_spec_close(got[s], want[s], f"{c.n}/{c.h} channel {s}")


# ------------------------------------------------------------------ 2. istft_hop blocks
@by_shape()
@pytest.mark.parametrize("gain,masked", [(False, False), (True, False), (False, True), (True, True)])
def test_istft_hop_blocks_equal_batched_istft(pkg, torch_cuda, case, gain, masked):
    """istft_hop over Plan.stft's rows with (none, gain, mask, gain + mask): the blocks
    are Plan.istft_ola's with the same step on the plan."""
    torch, c = torch_cuda, case
    want = c.batched(torch, lambda: c.plan.istft_ola(c.spec), gain, c.maskd if masked else None)
    c.plan.set_spectral_gain(c.gain if gain else None)
    try:
        st = pkg.Stream(c.plan, C_)
        blocks = [host(st.istft_hop(c.spec[:, k], c.maskd[:, k] if masked else None)).copy() for k in range(c.F)]
    finally:
        c.plan.set_spectral_gain(None)
    got = np.concatenate(blocks, axis=1)
    assert got.shape == want.shape == (C_, c.F * c.h)
    if c.exact:
        assert np.array_equal(bits(got), bits(want))
    else:
        for s in range(C_):
            xmax, xnorm = finite_scale(c.x[s])
            assert_close(got[s], want[s], xmax, f"{c.n}/{c.h} channel {s}", xnorm)


# ------------------------------------------------------------------ 3. push_hop_masked
@by_shape()
@pytest.mark.parametrize("gain", [False, True])
def test_push_hop_masked_equals_batched_masked_roundtrip(pkg, oracle, torch_cuda, case, gain):
    """push_hop_masked == Plan.roundtrip with the same mask (and gain), and within the
    FFT tolerance of the oracle's masked loop."""
    torch, c = torch_cuda, case
    want = c.batched(torch, lambda: c.plan.roundtrip(c.xd), gain, c.maskd)
    c.plan.set_spectral_gain(c.gain if gain else None)
    try:
        got = run_masked(pkg, torch, c, lambda k: c.maskd[:, k])
    finally:
        c.plan.set_spectral_gain(None)
    assert got.shape == want.shape == (C_, c.F * c.h)
    if not gain:  # (the mask does something: these are not push_hop's blocks)
        assert not np.array_equal(bits(got), bits(run_plain(pkg, torch, c)))
    if c.exact:
        assert np.array_equal(bits(got), bits(want))
    for s in range(C_):
        xmax, xnorm = finite_scale(c.x[s])
        if not c.exact:
            assert_close(got[s], want[s], xmax, f"{c.n}/{c.h} vs batched, channel {s}", xnorm)
        ref = oracle.roundtrip_mask(c.x[s], c.n, c.h, bin_gain=c.gain if gain else None, mask=c.mask[s],
                                    mode=oracle.DROP)
        assert_close(got[s], ref, xmax, f"{c.n}/{c.h} vs oracle, channel {s}", xnorm)


@by_shape()
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("interleaved", [False, True])
def test_push_hop_masked_equals_istft_of_stft_hop_for_hop(pkg, torch_cuda, case, shared, interleaved):
    """One launch or two through spectra in HBM: the same bits, hop for hop, with a
    shared row and per-channel rows, both PCM layouts, the gain on."""
    torch, c = torch_cuda, case
    row = (lambda k: c.mask_shared_d[k]) if shared else (lambda k: c.maskd[:, k])
    c.plan.set_spectral_gain(c.gain)
    try:
        whole = pkg.Stream(c.plan, C_, interleaved=interleaved)
        split = pkg.Stream(c.plan, C_, interleaved=interleaved)
        emitted = 0
        for q in range(c.hops):
            k = c.frame_of(q)
            hop = c.hop(torch, q, interleaved)
            out, em = whole.push_hop_masked(hop, row(max(k, 0)))
            spec, es = split.stft_hop(hop)
            assert (em != 0) == (es != 0) == (k >= 0), q
            if es:
                blk = split.istft_hop(spec, row(k))
                assert blk.shape == out.shape
                assert np.array_equal(bits(host(blk)), bits(host(out))), q
                emitted += 1
        assert emitted == c.F
    finally:
        c.plan.set_spectral_gain(None)


# ------------------------------------------------------------------ 4. identity cases
@by_shape()
@pytest.mark.parametrize("interleaved", [False, True])
def test_ones_and_no_mask_are_push_hop(pkg, torch_cuda, case, interleaved):
    """A row of ones, no mask, and the two entries alternating on one object all
    give push_hop's bits."""
    torch, c = torch_cuda, case
    want = run_plain(pkg, torch, c, interleaved)
    ones = torch.ones((C_, c.bins), dtype=torch.float32, device="cuda")
    assert np.array_equal(bits(run_masked(pkg, torch, c, lambda k: ones, interleaved)), bits(want))
    assert np.array_equal(bits(run_masked(pkg, torch, c, lambda k: ones[0], interleaved)), bits(want))
    assert np.array_equal(bits(run_masked(pkg, torch, c, lambda k: None, interleaved)), bits(want))
    st = pkg.Stream(c.plan, C_, interleaved=interleaved)
    outs = []
    for q in range(c.hops):
        hop = c.hop(torch, q, interleaved)
        out, em = st.push_hop(hop) if q % 2 == 0 else st.push_hop_masked(hop, ones if q % 4 == 1 else None)
        if em:
            outs.append(planar(out, interleaved))
    assert np.array_equal(bits(np.concatenate(outs, axis=1)), bits(want))


# ------------------------------------------------------------------ 7. reset and mode
@by_shape([(512, 128), (1024, 1024), (960, 240), (1024, 300)])
def test_reset_replays_and_modes_do_not_mix(pkg, torch_cuda, case):
    torch, c = torch_cuda, case
    nrep = c.hops // 2 + 1  # past the first emitted block
    st = pkg.Stream(c.plan, C_)
    row = lambda k: c.maskd[:, k]

    def whole_pass():
        got = []
        for q in range(nrep):
            out, em = st.push_hop_masked(c.hop(torch, q), row(max(c.frame_of(q), 0)))
            got.append(host(out).copy() if em else None)
        return got

    def split_pass():
        got = []
        for q in range(nrep):
            spec, em = st.stft_hop(c.hop(torch, q))
            got.append((host(spec).copy(), host(st.istft_hop(spec, row(c.frame_of(q)))).copy()) if em else None)
        return got

    a = whole_pass()
    assert any(o is not None for o in a)
    # whole mode: the split entries are refused, the object keeps working
    with pytest.raises(RuntimeError, match="crlot_stream_reset"):
        st.stft_hop(c.hop(torch, 0))
    with pytest.raises(RuntimeError, match="crlot_stream_reset"):
        st.istft_hop(c.spec[:, 0])
    st.push_hop(c.hop(torch, nrep))
    st.reset()
    b = whole_pass()
    for q in range(nrep):
        assert (a[q] is None) == (b[q] is None), q
        if a[q] is not None:
            assert np.array_equal(bits(a[q]), bits(b[q])), q
    st.reset()
    s1 = split_pass()
    with pytest.raises(RuntimeError, match="crlot_stream_reset"):
        st.push_hop(c.hop(torch, 0))
    with pytest.raises(RuntimeError, match="crlot_stream_reset"):
        st.push_hop_masked(c.hop(torch, 0), None)
    st.reset()
    s2 = split_pass()
    for q in range(nrep):
        assert (s1[q] is None) == (s2[q] is None) == (a[q] is None), q
        if s1[q] is not None:
            assert np.array_equal(cbits(s1[q][0]), cbits(s2[q][0])), q
            assert np.array_equal(bits(s1[q][1]), bits(s2[q][1])), q
            assert np.array_equal(bits(s1[q][1]), bits(a[q])), q
    # the two halves keep their own counters: synthesis may lag the analysis
    st.reset()
    specs = []
    for q in range(nrep):
        spec, em = st.stft_hop(c.hop(torch, q))
        if em:
            specs.append(spec)
    blocks = [host(st.istft_hop(sp, row(k))).copy() for k, sp in enumerate(specs)]
    want = [o for o in a if o is not None]
    assert len(blocks) == len(want)
    for k in range(len(blocks)):
        assert np.array_equal(bits(blocks[k]), bits(want[k])), k


# ------------------------------------------------------------------ 8. validation
@by_shape([(512, 128), (960, 240)])
def test_validation(pkg, torch_cuda, case):
    """Bad layouts are CRLOT_EINVAL (ValueError) before anything is launched; a wrong
    mask dtype or shape is caught in Python, where the element type is still known."""
    torch, c = torch_cuda, case
    L = pkg.lib()
    n, h, bins = c.n, c.h, c.bins
    st = pkg.Stream(c.plan, C_)
    hop = c.hop(torch, 0)
    out = torch.empty_like(hop)
    spec = torch.zeros((C_, bins + 1), dtype=torch.complex64, device="cuda")
    mask = torch.ones((C_, bins), dtype=torch.float32, device="cuda")
    em = ctypes.c_int32()
    hp, op, sp, mp = hop.data_ptr(), out.data_ptr(), spec.data_ptr(), mask.data_ptr()
    ld = 2 * (bins + 1)

    def einval(rc):
        assert rc == pkg.EINVAL, rc
        with pytest.raises(ValueError):
            pkg._check(rc)

    for bad_ld in (n + 3, n + 1, n, 0, -2):  # odd, short
        einval(L.crlot_stream_stft_hop(st._h, hp, sp, bad_ld, ctypes.byref(em), None))
        einval(L.crlot_stream_istft_hop(st._h, sp, bad_ld, None, 0, op, None))
    einval(L.crlot_stream_stft_hop(st._h, hp, sp + 4, ld, ctypes.byref(em), None))  # misaligned
    einval(L.crlot_stream_istft_hop(st._h, sp + 4, ld, None, 0, op, None))
    for bad_ld in (1, n // 4, n // 2, -1):
        einval(L.crlot_stream_istft_hop(st._h, sp, ld, mp, bad_ld, op, None))
        einval(L.crlot_stream_push_hop_masked(st._h, hp, mp, bad_ld, op, ctypes.byref(em), None))
    einval(L.crlot_stream_stft_hop(st._h, None, sp, ld, ctypes.byref(em), None))  # null buffers
    einval(L.crlot_stream_stft_hop(st._h, hp, None, ld, ctypes.byref(em), None))
    einval(L.crlot_stream_istft_hop(st._h, None, ld, None, 0, op, None))
    einval(L.crlot_stream_istft_hop(st._h, sp, ld, None, 0, None, None))
    einval(L.crlot_stream_push_hop_masked(st._h, None, mp, bins, op, ctypes.byref(em), None))
    einval(L.crlot_stream_push_hop_masked(st._h, hp, mp, bins, None, ctypes.byref(em), None))
    einval(L.crlot_stream_stft_hop(None, hp, sp, ld, ctypes.byref(em), None))
    # none of the refused calls fixed a mode or moved a counter: the object still runs either way
    _, e0 = st.push_hop_masked(hop, mask)
    assert e0 == (h if c.frame_of(0) >= 0 else 0)
    st.reset()
    _, e1 = st.stft_hop(hop, spec[:, :bins])  # rows 2 (bins + 1) floats apart: a padded ld_spec
    assert e1 == (1 if c.frame_of(0) >= 0 else 0)
    st.reset()
    # Python-side checks
    for bad in (mask.double(), mask[:, :-1], mask[:-1], mask.t().contiguous().t(), mask.cpu(),
                torch.ones((2, C_, bins), device="cuda"), mask.to(torch.float16), host(mask)):
        with pytest.raises(ValueError):
            st.push_hop_masked(hop, bad)
        with pytest.raises(ValueError):
            st.istft_hop(spec[:, :bins], bad)
    for bad in (hop.double(), hop[:, :-1], hop.cpu(), hop.t()):
        with pytest.raises(ValueError):
            st.push_hop_masked(bad, mask)
        with pytest.raises(ValueError):
            st.stft_hop(bad)
    for bad in (spec[:, :bins].real, spec[:, :bins - 1], spec[:-1, :bins], spec.cpu()[:, :bins],
                torch.zeros((C_, bins), dtype=torch.complex128, device="cuda")):
        with pytest.raises(ValueError):
            st.istft_hop(bad)
        with pytest.raises(ValueError):
            st.stft_hop(hop, bad)
    st.close()
