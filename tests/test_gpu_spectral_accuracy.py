"""Frame-local accuracy of the forward spectra, against a float64 DFT.

DESIGN 4 bounds a time-domain block's error by its own frames and their pair
mates (tests/test_gpu_local_accuracy.py).  This file holds the frequency-domain
counterpart: every frame of a forward spectrum is judged against its OWN scale
ps[k] = max_b |X64[k, b]| -- with frame pairing on against the larger of its own
and its pair mate's (frames k and k ^ 1 of a call share one transform) -- and a
frame whose input is exact silence is exact zeros, whether or not its mate is
live (a pair with exactly one all-zero input frame is transformed frame by
frame: hop_live / hops_live_code / any_nonzero, csrc/fused_common.h).  The
whole-stream bars of tests/test_gpu_stft.py cannot see either: one loud frame
sets the scale of every other frame of its stream.

Reference: numpy float64 rfft of the float32 frame times the float32 window
(tests/f64_reference.py stft_f64); metric: spec_local_err / spec_frame_l2 /
silent_spec_is_zero in tests/spec_reference.py, which also re-exports the former's
names.  tests/test_spec_reference.py proves on the CPU that
the oracle (kiss_fftr in float32) meets all of it on these inputs with
spec_local_err(own) <= 2.93e-7 and per-frame rel-L2 <= 1.58e-7 (998/499, whose
half size 499 is prime: 1.12e-6 / 5.18e-7), and that the inputs hold the lone
silent frames (s2, 8), (gaps, 20), (gaps, 41): both parities.

Bars: the project's 4e-6 (peak-relative) and 1e-6 (rel-L2), >= 6x the oracle's own
error.  Where the complex transform length (N / 2 for a real transform) has a prime
factor > 7 -- 998/499, FFT-plan sizes 998 and 499 -- a generic O(R^2) butterfly's
summation error grows with R and its order of additions is the implementation's
own, so the bar is the larger of the project's and 4x the oracle's figure on the
same input and metric, computed here (spec_reference.spec_bars).

Inputs: spec_reference.make_spec_streams, six streams per shape -- plain; level
steps of 2^-24 and 2^12; exact leading silence with the onset in the pair mate,
and a silent gap; plain; tones (on-bin, off-bin + DC, Nyquist); two one-frame
gaps, one on an even and one on an odd frame.

  (a) crlot_stft at SPEC_SHAPES x pairing x {ZERO_PAD, DROP}: the bars, silent frames
      zero by value, DC / Nyquist imaginary parts zero, bits under chunkings 1, 3, F,
      the same on an even frame count, each stream alone against its bits in the batch;
      the launch record names the regime that ran.
  (b) crlot_spectrogram on the same inputs: POWER bit for bit fl(fl(re^2) + fl(im^2)) of
      (a)'s spectra where k_pair_feat's own regime branch switches, MAGNITUDE its sqrt,
      silent frames +0 and log(floor) through a dB filterbank, and the float64 bound.
  (c) Stream.stft_hop, the six streams as six channels, against the DROP rows (own bars).
  (d) FftPlan rows against numpy float64, six rows spanning 2^32 in level per batch.

The last frame of an odd frame count has no mate: the samples after it belong to
no frame (DROP keeps up to a hop of them).  (a) and (b) also run DROP streams whose
tail is 2^12 louder than the frames and whose stream 3 ends in a silent frame
(spec_reference.make_tail_streams).  This was a miss when the file was written:
every frame-pair forward kernel took that tail as the imaginary half of the last
transform -- the last frame's spec_local_err(own) 9.2e-6 .. 2.1e-4 with pairing on
(<= 1.8e-7 off), a silent last frame not zeros; they now put zeros there.

Observed on an MI355X, crlot_stft, worst spec_local_err / per-frame rel-L2 over the
six streams, both framings, both frame counts and the loud tail (pairing on against
the pair scales | pairing off against the frame's own | the oracle on the CPU, own):
    512/128   1.87e-7 / 1.15e-7 | 2.00e-7 / 1.22e-7 | 2.17e-7 / 1.30e-7
    1024/128  1.84e-7 / 1.26e-7 | 1.97e-7 / 1.22e-7 | 2.35e-7 / 1.29e-7
    1024/256  1.59e-7 / 1.19e-7 | 2.16e-7 / 1.22e-7 | 1.91e-7 / 1.29e-7
    1024/512  1.58e-7 / 1.17e-7 | 1.91e-7 / 1.24e-7 | 1.94e-7 / 1.29e-7
    2048/512  1.99e-7 / 1.19e-7 | 2.21e-7 / 1.34e-7 | 2.38e-7 / 1.37e-7
    4096/1024 1.67e-7 / 1.23e-7 | 2.09e-7 / 1.42e-7 | 2.62e-7 / 1.41e-7
    480/120   1.68e-7 / 1.17e-7 | 2.31e-7 / 1.23e-7 | 2.13e-7 / 1.29e-7
    960/240   1.73e-7 / 1.21e-7 | 1.99e-7 / 1.31e-7 | 2.16e-7 / 1.38e-7
    882/441   1.84e-7 / 1.34e-7 | 2.08e-7 / 1.35e-7 | 2.13e-7 / 1.42e-7
    1764/441  1.87e-7 / 1.42e-7 | 2.38e-7 / 1.43e-7 | 2.27e-7 / 1.58e-7
    1000/250  2.32e-7 / 1.62e-7 | 2.01e-7 / 1.32e-7 | 2.35e-7 / 1.40e-7
    1920/480  1.94e-7 / 1.29e-7 | 2.29e-7 / 1.31e-7 | 2.46e-7 / 1.38e-7
    256/128   2.18e-7 / 1.18e-7 | 2.18e-7 / 1.20e-7 | 2.93e-7 / 1.24e-7   (no pair kernel)
    1536/384  2.15e-7 / 1.29e-7 | 2.16e-7 / 1.29e-7 | 2.12e-7 / 1.33e-7   (no pair kernel)
    998/499   1.01e-6 / 5.26e-7 | 1.13e-6 / 5.26e-7 | 1.12e-6 / 5.18e-7   (no pair kernel; 499 prime)
stft_hop 1.95e-7 .. 2.21e-7 / 1.22e-7 .. 1.34e-7; spectrogram power within 0.06 of its
float64 bound; FftPlan rows <= 3.73e-7 / 1.48e-7 at the smooth sizes, 998 real
6.01e-7 / 4.18e-7 and 499 complex 9.08e-7 / 4.28e-7 (the oracle: 6.2e-7 / 4.2e-7).
"""
import numpy as np
import pytest

import spec_reference as R
from test_gpu_parity import bits, dev, host

pytestmark = pytest.mark.gpu

S = R.SPEC_S
PAIR_KERNELS = ("k_pair", "k_pn_", "k_p15_")   # the frame-pair families' launch-record names
HAS_PAIR_STFT = set(R.SHAPES)                  # 256/128, 1536/384 and 998/499 have no pair kernel
SHARED_WAVE = {(480, 120)}                     # two streams per wave with pairing on
MODE_IDS = ["zero_pad", "drop"]
_cache = {}


def cbits(X):
    return np.ascontiguousarray(X, np.complex64).view(np.uint32)


def refs_of(oracle, x, n, h, mode):
    """Per stream: the float64 spectra, the own and pair scales, and -- where the bar
    depends on it -- the oracle's own figures under both scales."""
    out = []
    for s in range(x.shape[0]):
        X64 = R.stft_f64(x[s], n, h, mode)
        ps = R.spec_peak(X64)
        r = {"X64": X64, "own": ps, "pair": R.spec_pair_peak(ps), "oracle": {False: (0.0, 0.0), True: (0.0, 0.0)}}
        if R.generic_butterfly(n // 2):
            _, Xo = oracle.roundtrip_mask(x[s], n, h, mode=mode, want_spec=True)
            r["oracle"] = {False: (R.spec_local_err(Xo, X64, ps), R.spec_frame_l2(Xo, X64)),
                           True: (R.spec_local_err(Xo, X64, r["pair"]), R.spec_frame_l2(Xo, X64, pair=True))}
        out.append(r)
    return out


def case(oracle, n, h, mode):
    """Inputs and float64 references of a shape and framing, computed once and shared
    (read-only): the whole streams (an odd frame count) and the streams without their
    last hop (an even one: the last frame has a mate)."""
    key = (n, h, mode)
    if key not in _cache:
        x = R.make_spec_streams(n, h)
        x.setflags(write=False)
        T = x.shape[1]
        F = R.frame_count(T, n, h, mode)
        assert F >= 45 and F % 2 == 1 and R.frame_count(T - h, n, h, mode) == F - 1
        _cache[key] = {"x": x, "T": T, "F": F, "full": refs_of(oracle, x, n, h, mode),
                       "even": refs_of(oracle, x[:, :T - h], n, h, mode)}
        if mode == R.DROP:   # a loud tail that belongs to no frame, after a last frame without a mate
            xt = R.make_tail_streams(n, h)
            xt.setflags(write=False)
            _cache[key].update({"x_tail": xt, "tail": refs_of(oracle, xt, n, h, mode)})
    return _cache[key]


def upload(torch, x):
    """Rows on an even pitch: T is odd at some shapes, and rows that are not 8-byte
    aligned leave the walkers this file is about."""
    rows, T = x.shape
    xd = torch.zeros((rows, T + (T & 1)), dtype=torch.float32, device="cuda")[:, :T]
    xd.copy_(dev(torch, np.array(x)))
    return xd


class Judge:
    """Applies the frame-local assertions to a producer's spectra, keeps the worst
    figures, and collects the misses so that one run reports every figure before it fails."""

    def __init__(self, n, pairing):
        self.n, self.pairing = n, pairing
        self.worst, self.worst_l2, self.misses = 0.0, 0.0, []

    def __call__(self, X, refs, what, streams=None):
        streams = range(len(refs)) if streams is None else streams
        assert X.shape[0] == len(streams), (what, X.shape)
        for i, s in enumerate(streams):
            r = refs[s]
            assert X[i].shape == r["X64"].shape, (what, X[i].shape, r["X64"].shape)
            if not np.all(np.isfinite(X[i].view(np.float32))):
                self.misses.append(f"{what} stream {s}: non-finite values")
                continue
            scale = r["pair"] if self.pairing else r["own"]
            err = R.spec_local_err(X[i], r["X64"], scale)
            l2 = R.spec_frame_l2(X[i], r["X64"], pair=self.pairing)
            bar, bar_l2 = R.spec_bars(self.n // 2, *r["oracle"][self.pairing])
            self.worst, self.worst_l2 = max(self.worst, err), max(self.worst_l2, l2)
            if err > bar:
                k = int(np.argmax(np.where(scale > 0, R.spec_frame_err(X[i], r["X64"]) / np.maximum(scale, 1e-300), 0)))
                self.misses.append(f"{what} stream {s}: spec_local_err {err:.3e} > {bar:.3e} (frame {k})")
            if l2 > bar_l2:
                self.misses.append(f"{what} stream {s}: per-frame rel-L2 {l2:.3e} > {bar_l2:.3e}")
            # a lone silent member is transformed alone, two silent members transform to zeros
            if not R.silent_spec_is_zero(X[i], r["own"]):
                sil = R.silent_frames(r["own"])
                mx = np.max(np.abs(X[i][sil]), axis=1)
                self.misses.append(f"{what} stream {s}: silent frames {sil[mx != 0].tolist()} not zero "
                                   f"(max |X| {mx.max():.3e})")
            if np.any(X[i][:, 0].imag != 0) or np.any(X[i][:, -1].imag != 0):
                self.misses.append(f"{what} stream {s}: DC / Nyquist imaginary part not zero")

    def report(self, label):
        print(f"\n{label}: spec_local_err({'pair' if self.pairing else 'own'}) {self.worst:.2e}  "
              f"per-frame rel-L2 {self.worst_l2:.2e}  misses {len(self.misses)}")
        for msg in self.misses:
            print("  MISS", msg)
        assert not self.misses, f"{label}: " + "; ".join(self.misses[:8])


# ------------------------------------------------------------------ (a) crlot_stft
@pytest.mark.parametrize("mode", [R.ZERO_PAD, R.DROP], ids=MODE_IDS)
@pytest.mark.parametrize("pairing", [True, False], ids=["paired", "per_frame"])
@pytest.mark.parametrize("n,h", R.SPEC_SHAPES)
def test_stft_frame_local_accuracy(pkg, oracle, torch_cuda, n, h, pairing, mode):
    torch = torch_cuda
    c = case(oracle, n, h, mode)
    x, T, F = c["x"], c["T"], c["F"]
    plan = pkg.Plan(frame_size=n, hop_size=h, boundary_mode=mode, frame_pairing=pairing)
    assert plan.frame_count(T) == F and plan.frame_count(T - h) == F - 1
    xd = upload(torch, x)
    judge = Judge(n, pairing)

    def launched(what):
        """The regime under test really ran: a frame-pair kernel with pairing on wherever
        the shape has one, none with pairing off."""
        ks = plan.last_launch()["kernels"]
        pair_ran = any(k.startswith(PAIR_KERNELS) for k in ks)
        assert ks and pair_ran == (pairing and (n, h) in HAS_PAIR_STFT), (what, ks)

    X = host(plan.stft(xd))
    launched("stft")
    assert X.shape == (S, F, n // 2 + 1)
    judge(X, c["full"], "stft")

    # the bits under every chunking
    for chunks in (1, 3, F):
        plan.set_chunks(chunks)
        Xc = host(plan.stft(xd))
        launched(f"stft {chunks} chunks")
        if not np.array_equal(cbits(Xc), cbits(X)):
            judge.misses.append(f"stft: bits change at {chunks} chunks")
            judge(Xc, c["full"], f"stft {chunks} chunks")   # (which frames, for the report)
    plan.set_chunks(0)

    # an even frame count: the last frame now has a mate
    Xe = host(plan.stft(xd[:, :T - h]))
    launched("stft even F")
    judge(Xe, c["even"], "stft even F")

    # DROP: the samples after the last frame belong to no frame.  2^12 louder than the
    # frames, they leave the last frame (odd F: no mate) at its own scale, and a silent
    # last frame zeros
    if mode == R.DROP:
        Xt = host(plan.stft(upload(torch, c["x_tail"])))
        launched("stft loud tail")
        judge(Xt, c["tail"], "stft loud tail")

    # each stream alone
    for s in range(S):
        X1 = host(plan.stft(upload(torch, x[s:s + 1])))
        launched(f"stft stream {s} alone")
        if pairing and (n, h) in SHARED_WAVE:
            # two streams share a wave here, and a lone silent member in one sends the other
            # to the per-frame regime as well (csrc/fused_common.h, pair_code<32>): a stream's
            # bits depend on its wave mate, so the stream alone is held to the bars instead
            judge(X1, c["full"], f"stft stream {s} alone", streams=[s])
        elif not np.array_equal(cbits(X1[0]), cbits(X[s])):
            judge.misses.append(f"stft: stream {s} alone differs from its bits in the batch")

    judge.report(f"stft {n}/{h} {MODE_IDS[mode]} pairing={'on' if pairing else 'off'}")


# ------------------------------------------------------------------ (b) crlot_spectrogram
FEAT_SHAPES = [(256, 128), (512, 128), (1024, 128), (1024, 256), (1024, 512), (1024, 300), (4096, 1024), (960, 240)]
PAIR_FEAT = {(1024, 128), (1024, 256), (1024, 512)}   # k_pair_feat<2/4/8> with pairing on


def power_of(spec):
    """float32(float32(re re) + float32(im im)) of a complex64 array."""
    f = np.ascontiguousarray(spec, np.complex64).view(np.float32).reshape(spec.shape + (2,))
    re, im = f[..., 0], f[..., 1]
    return (re * re) + (im * im)  # float32 arrays: every product and the sum round to float32


def ulps(out, ref64):
    return np.abs(out.astype(np.float64) - ref64) / np.spacing(np.abs(np.float32(ref64))).astype(np.float64)


@pytest.mark.parametrize("mode", [R.ZERO_PAD, R.DROP], ids=MODE_IDS)
@pytest.mark.parametrize("pairing", [True, False], ids=["paired", "per_frame"])
@pytest.mark.parametrize("n,h", FEAT_SHAPES)
def test_spectrogram_frame_local_accuracy(pkg, oracle, torch_cuda, n, h, pairing, mode):
    torch = torch_cuda
    if (n, h) in R.SPEC_SHAPES:
        c = case(oracle, n, h, mode)
        inputs = [("", c["x"], c["full"])] + ([("loud tail: ", c["x_tail"], c["tail"])] if mode == R.DROP else [])
    else:   # (1024/300: the per-wave walker at a hop that is no multiple of 64)
        inputs = [("", R.make_spec_streams(n, h), None)]
        if mode == R.DROP:
            inputs.append(("loud tail: ", R.make_tail_streams(n, h), None))
        inputs = [(label, x, refs_of(oracle, x, n, h, mode)) for label, x, _ in inputs]
    plan = pkg.Plan(frame_size=n, hop_size=h, boundary_mode=mode, frame_pairing=pairing)
    fp = pkg.Features(plan, kind=pkg.FEAT_POWER)
    fm = pkg.Features(plan, kind=pkg.FEAT_MAGNITUDE)
    floor = 1e-10
    fdb = pkg.Features(plan, weights=pkg.mel_filterbank(40, n, 16000.0), log=pkg.FEAT_DB, floor=floor)
    db_floor = 10.0 * np.log10(np.float64(np.float32(floor)))
    misses, worst, ks = [], 0.0, None
    for label, x, refs in inputs:
        xd = upload(torch, x)
        X = host(plan.stft(xd))
        p = host(fp.spectrogram(xd))
        ks = plan.last_launch()["kernels"]
        assert ("k_pair_feat" in ks) == (pairing and (n, h) in PAIR_FEAT), ks
        m = host(fm.spectrogram(xd))
        db = host(fdb.spectrogram(xd))
        # one walk over the whole stream (the default chunking of streams this short keeps a
        # walk to a few pairs): the regime bits shift through every pair, and nothing changes
        plan.set_chunks(1)
        for f, base, what in ((fp, p, "power"), (fdb, db, "dB bands")):
            if not np.array_equal(bits(host(f.spectrogram(xd))), bits(base)):
                misses.append(f"{label}{what}: bits change at 1 chunk")
        plan.set_chunks(0)
        # the existing contract, where k_pair_feat's regime branch switches
        want = power_of(X)
        if not np.array_equal(bits(p), bits(want)):
            bad = np.argwhere(np.any(bits(p) != bits(want), axis=2))
            misses.append(f"{label}power differs from fl(fl(re^2) + fl(im^2)) of crlot_stft at (stream, frame) "
                          f"{bad[:6].tolist()}")
        if not np.array_equal(bits(m), bits(np.sqrt(want))):
            misses.append(f"{label}magnitude differs from sqrt of the power")
        assert R.silent_frames(refs[2]["own"])[0] == 0   # (db[2][0]: a silent frame, the value compared below)
        for s in range(S):
            r = refs[s]
            sil = R.silent_frames(r["own"])
            if np.any(bits(p[s][sil]) != 0):
                misses.append(f"{label}stream {s}: silent frames' power is not +0 (max {np.max(np.abs(p[s][sil])):.3e})")
            # max(+0, floor) = floor in every band of a silent frame: one value, the float32 log
            # of the floor (logf / log10f are documented at 1-2 ulp, DB adds a rounding: <= 4 ulp)
            if sil.size:
                v = db[s][sil]
                if np.any(bits(v) != bits(db[2][0, :1])) or np.max(ulps(v, db_floor)) > 4.0:
                    misses.append(f"{label}stream {s}: dB bands of silent frames are not log(floor): {np.unique(v)[:4]}")
            # against float64 directly: the complex error bound squared out, plus three roundings
            a64 = np.abs(r["X64"])
            scale = (r["pair"] if pairing else r["own"])[:, None]
            e = R.SPEC_MAX_ABS * scale
            bound = (2 * a64 + e) * e + 2.0 ** -22 * (a64 + e) ** 2
            d = np.abs(p[s].astype(np.float64) - a64 ** 2)
            ratio = float(np.max(np.where(bound > 0, d / np.maximum(bound, 1e-300), np.where(d > 0, np.inf, 0.0))))
            worst = max(worst, ratio)
            if ratio > 1.0:
                misses.append(f"{label}stream {s}: power vs float64 at {ratio:.3g} of its bound")
    print(f"\nspectrogram {n}/{h} {MODE_IDS[mode]} pairing={'on' if pairing else 'off'} {ks}: "
          f"power error at most {worst:.3f} of the float64 bound, misses {len(misses)}")
    for msg in misses:
        print("  MISS", msg)
    for f in (fp, fm, fdb):
        f.close()
    assert not misses, f"{n}/{h}: " + "; ".join(misses[:8])


# ------------------------------------------------------------------ (c) Stream.stft_hop
@pytest.mark.parametrize("n,h", [(512, 128), (2048, 512), (960, 240), (4096, 1024)])
def test_stft_hop_frame_local_accuracy(pkg, oracle, torch_cuda, n, h):
    """The per-hop path never pairs: row k against the DROP frame k under the own bars.
    512/128 and 2048/512 take the resident body, 960/240 and 4096/1024 the any-shape one."""
    torch = torch_cuda
    c = case(oracle, n, h, R.DROP)
    x, F = c["x"], c["F"]
    plan = pkg.Plan(frame_size=n, hop_size=h, boundary_mode=pkg.DROP)
    xd = upload(torch, x)
    st = pkg.Stream(plan, S)
    rows = []
    for q in range(x.shape[1] // h):
        spec, em = st.stft_hop(xd[:, q * h:(q + 1) * h].contiguous())
        assert em == (1 if (q + 1) * h >= n else 0), q
        if em:
            rows.append(spec.clone())
    X = host(torch.stack(rows, dim=1))
    assert X.shape == (S, F, n // 2 + 1)
    judge = Judge(n, False)
    judge(X, c["full"], "stft_hop")
    st.close()
    judge.report(f"stft_hop {n}/{h}")


# ------------------------------------------------------------------ (d) FFT-plan rows
def fft_rows(n, cplx):
    """Six rows spanning 2^32 in level: unit Gaussian noise, a tone exactly at bin n // 3,
    noise 2^-20, noise 2^12, an all-zero row, a unit impulse at n // 2."""
    rng = np.random.default_rng(7000 + n)
    t = np.arange(n)

    def noise():
        return rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)

    ph = 2 * np.pi * (n // 3) * t / n
    imp = np.zeros(n)
    imp[n // 2] = 1.0
    rows = [noise(), np.exp(1j * ph) if cplx else np.cos(ph), noise() * 2.0 ** -20, noise() * 2.0 ** 12, np.zeros(n), imp]
    return np.stack(rows).astype(np.complex64 if cplx else np.float32)


ZERO_ROW = 4


def judge_rows(got, ref, m, oracle_rows, what, misses):
    """Per row: max-abs error / the row's own float64 peak and rel-L2 against the bars
    (spec_bars: 4x the oracle's figure on the same row where length m needs a generic
    butterfly); the zero row comes back all zero.  Returns the worst two figures."""
    worst = [0.0, 0.0]
    for b in range(ref.shape[0]):
        if b == ZERO_ROW:
            if np.any(got[b] != 0):
                misses.append(f"{what}: the zero row is not zero")
            continue
        fig = []
        for y in (got[b],) + (() if oracle_rows is None else (oracle_rows[b],)):
            d = np.asarray(y, np.complex128) - ref[b]
            fig.append((float(np.max(np.abs(d)) / np.max(np.abs(ref[b]))), float(np.linalg.norm(d) / np.linalg.norm(ref[b]))))
        bar, bar_l2 = R.spec_bars(m, *(fig[1] if oracle_rows is not None else (0.0, 0.0)))
        worst = [max(worst[0], fig[0][0]), max(worst[1], fig[0][1])]
        if not np.all(np.isfinite(np.asarray(got[b], np.complex128).view(np.float64))):
            misses.append(f"{what} row {b}: non-finite values")
        if fig[0][0] > bar:
            misses.append(f"{what} row {b}: max-abs / peak {fig[0][0]:.3e} > {bar:.3e}")
        if fig[0][1] > bar_l2:
            misses.append(f"{what} row {b}: rel-L2 {fig[0][1]:.3e} > {bar_l2:.3e}")
    return worst


def alone(fn, torch, rows, got, what, misses):
    """Every non-zero row's bits are the same when it is transformed alone."""
    for b in range(rows.shape[0]):
        if b != ZERO_ROW:
            one = host(fn(dev(torch, rows[b:b + 1])))[0]
            if not np.array_equal(np.ascontiguousarray(one).view(np.uint32), np.ascontiguousarray(got[b]).view(np.uint32)):
                misses.append(f"{what} row {b}: alone differs from its bits in the batch")


@pytest.mark.parametrize("n", [2, 6, 30, 96, 100, 256, 998, 1000, 1024, 4096, 4410, 12000])
def test_fft_plan_real_rows_vs_float64(pkg, oracle, torch_cuda, n):
    torch = torch_cuda
    x = fft_rows(n, False)
    plan = pkg.FftPlan(n, pkg.FFT_REAL)
    generic = R.generic_butterfly(n // 2)
    k = oracle.KissR(n) if generic else None
    misses = []
    ref = np.fft.rfft(x.astype(np.float64), axis=1)
    X = host(plan.forward(dev(torch, x)))
    wf = judge_rows(X, ref, n // 2, None if k is None else [k.forward(r) for r in x], "forward", misses)
    alone(plan.forward, torch, x, X, "forward", misses)
    if np.any(X[:, 0].imag != 0) or np.any(X[:, -1].imag != 0):
        misses.append("forward: DC / Nyquist imaginary part not zero")
    Y = ref.astype(np.complex64)
    Y[:, 0] = Y[:, 0].real      # (the real inverse ignores them; zero keeps the reference unambiguous)
    Y[:, -1] = Y[:, -1].real
    yref = np.fft.irfft(Y.astype(np.complex128), n=n, axis=1)
    y = host(plan.inverse(dev(torch, Y)))
    wi = judge_rows(y, yref, n // 2, None if k is None else [k.inverse(r) for r in Y], "inverse", misses)
    alone(plan.inverse, torch, Y, y, "inverse", misses)
    print(f"\nfft real n={n}: forward {wf[0]:.2e} / {wf[1]:.2e}  inverse {wi[0]:.2e} / {wi[1]:.2e}  "
          f"(max-abs / peak, rel-L2) misses {len(misses)}")
    for msg in misses:
        print("  MISS", msg)
    plan.close()
    assert not misses, f"n={n}: " + "; ".join(misses[:8])


@pytest.mark.parametrize("n", [1, 3, 5, 7, 12, 100, 499, 1000, 3000, 4096, 8192])
def test_fft_plan_complex_rows_vs_float64(pkg, oracle, torch_cuda, n):
    torch = torch_cuda
    z = fft_rows(n, True)
    plan = pkg.FftPlan(n, pkg.FFT_COMPLEX)
    generic = R.generic_butterfly(n)
    k = oracle.KissC(n) if generic else None
    misses = []
    ref = np.fft.fft(z.astype(np.complex128), axis=1)
    Z = host(plan.forward_complex(dev(torch, z)))
    wf = judge_rows(Z, ref, n, None if k is None else [k.forward(r) for r in z], "forward_complex", misses)
    alone(plan.forward_complex, torch, z, Z, "forward_complex", misses)
    Y = ref.astype(np.complex64)
    yref = np.fft.ifft(Y.astype(np.complex128), axis=1)
    y = host(plan.inverse_complex(dev(torch, Y)))
    wi = judge_rows(y, yref, n, None if k is None else [k.inverse(r) for r in Y], "inverse_complex", misses)
    alone(plan.inverse_complex, torch, Y, y, "inverse_complex", misses)
    print(f"\nfft complex n={n}: forward {wf[0]:.2e} / {wf[1]:.2e}  inverse {wi[0]:.2e} / {wi[1]:.2e}  "
          f"(max-abs / peak, rel-L2) misses {len(misses)}")
    for msg in misses:
        print("  MISS", msg)
    plan.close()
    assert not misses, f"n={n}: " + "; ".join(misses[:8])
