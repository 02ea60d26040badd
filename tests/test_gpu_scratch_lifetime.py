"""The composite entries across streams, threads, scratch growth, slot recycling and
graph replay (include/crlot_dsp.h, "Streams and threads").

crlot_spectrogram (staged), crlot_time_stretch, crlot_pitch_shift, crlot_griffin_lim,
crlot_hpss and crlot_convolve keep their spectra, masks and staging buffers in the
calling stream's scratch slot, which crlot_roundtrip's staged paths and the chunked
crlot_phase_vocoder share.  A pointer that survives a regrowth, a carve that leaks
from one entry into the next, a slot that is shared between streams or freed early:
none of these shows in a call that runs alone.

The yardstick is the serial run: the same call with the same arguments, alone on the
current stream, followed by a device synchronise, compared bit for bit (bits never
depend on batch, chunking or layout, so any difference is a bug).  Each composite's
serial result is itself held once to the reference of the entry's own test module, at
that module's bar: the composition on the public entries (bit equality) and, for
crlot_convolve, float64 as well.

Every queued section starts with a device-side sleep on each participating stream and
ends with the assertion that those streams are still busy: the calls were all queued
before any of them ran.
"""
import threading
import types

import numpy as np
import pytest

import convolve_reference as CR
import test_gpu_convolve as CV
import test_gpu_griffin_lim as GLT
import test_gpu_hpss as HP
import test_gpu_pitch_shift as PS
import test_gpu_time_stretch as TS
from test_gpu_concurrency import check_vs_oracle
from test_gpu_features import power_of
from test_gpu_parity import bits, host

pytestmark = pytest.mark.gpu

SLEEP = 100_000_000  # cycles: about 50 ms (tests/test_gpu_concurrency.py)
NAN = float("nan")
RATE = 1.3
UP, DOWN = 160, 147
N_ITER, MOMENTUM = 3, 0.99
CONV_B, CONV_K, CONV_NF = 128, 3 * 128 + 7, 2
IDLE = "the stream drained before the last call was queued: this run exercised nothing"

# (N, H, frame pairing): the pair and the walk routes, the mixed radix as frame pairs
# and with both halves of every composite staged, and the shape whose
# crlot_spectrogram is staged under the default pairing
PLANS = [(1024, 256, True), (1024, 256, False), (960, 240, True), (960, 240, False), (512, 128, True)]


# ------------------------------------------------------------------ buffers
def same_bits(torch, a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def out_rows(torch, shape, odd):
    """A NaN-filled output of `shape` inside rows a float or two longer: an odd leading
    dimension (4-byte aligned rows only) when `odd`, else an even one (8-byte aligned)."""
    L = shape[-1]
    pad = 1 + L % 2 if odd else L % 2
    return torch.full(tuple(shape[:-1]) + (L + pad,), NAN, device="cuda")[..., :L]


def offset_rows(torch, x):
    """x one float into rows of T + 1: a 4-byte offset from an 8-byte boundary."""
    S, T = x.shape
    big = torch.zeros((S, T + 1), device="cuda")
    big[:, 1:] = x
    v = big[:, 1:]
    assert v.data_ptr() % 8 == 4
    return v


def make_call(name, plan, alloc, run):
    """alloc(): fresh outputs; run(outs): the call, on the current stream; plan: the
    plan whose launch record the call leaves."""
    return types.SimpleNamespace(name=name, plan=plan, alloc=alloc, run=run)


def run_serial(torch, c):
    """The yardstick: the call alone on the current stream, then a synchronise."""
    torch.cuda.synchronize()
    outs = c.alloc()
    c.run(outs)
    torch.cuda.synchronize()
    return outs, c.plan.last_launch()


def all_same(torch, got, want):
    return len(got) == len(want) and all(same_bits(torch, g, w) for g, w in zip(got, want))


def fresh_streams(torch, k):
    """k torch streams with pairwise distinct handles, none of them the current stream's."""
    streams = [torch.cuda.Stream() for _ in range(k)]
    handles = [s.cuda_stream for s in streams] + [torch.cuda.current_stream().cuda_stream]
    assert len(set(handles)) == k + 1, handles
    return streams


def hold(torch, streams):
    for s in streams:
        with torch.cuda.stream(s):
            torch.cuda._sleep(SLEEP)


# ------------------------------------------------------------------ the entries as calls
def spectrogram_call(torch, feat, x, odd):
    S, T = x.shape
    shape = (S, feat.plan.frame_count(T), feat.n_out)
    return make_call("spectrogram", feat.plan, lambda: [out_rows(torch, shape, odd)],
                     lambda o: feat.spectrogram(x, out=o[0]))


def time_stretch_call(torch, plan, x, odd, rate=RATE):
    shape = (x.shape[0], plan.stretch_output_length(x.shape[1], rate))
    return make_call("time_stretch", plan, lambda: [out_rows(torch, shape, odd)],
                     lambda o: plan.time_stretch(x, rate, y=o[0]))


def pitch_shift_call(torch, plan, res, x, odd):
    return make_call("pitch_shift", plan, lambda: [out_rows(torch, tuple(x.shape), odd)],
                     lambda o: plan.pitch_shift(x, res, y=o[0]))


def hpss_call(torch, plan, x, odd):
    shape = (x.shape[0], plan.frame_count(x.shape[1]) * plan.hop_size)
    return make_call("hpss", plan, lambda: [out_rows(torch, shape, odd), out_rows(torch, shape, odd)],
                     lambda o: plan.hpss(x, y_h=o[0], y_p=o[1]))


def griffin_lim_call(torch, plan, mag, odd):
    shape = (mag.shape[0], mag.shape[1] * plan.hop_size)
    return make_call("griffin_lim", plan, lambda: [out_rows(torch, shape, odd)],
                     lambda o: plan.griffin_lim(mag, N_ITER, MOMENTUM, y=o[0]))


def convolve_call(torch, conv, x, odd):
    shape = (x.shape[0], conv.output_length(x.shape[1]))
    return make_call("convolve", conv.plan, lambda: [out_rows(torch, shape, odd)],
                     lambda o: conv.convolve(x, y=o[0]))


def gl_mag(torch, n, h, S, F, flip=False):
    """Griffin-Lim target magnitudes of tests/test_gpu_griffin_lim.py's signals: the first F frames."""
    mag = GLT.fixture_np(n, h, S)[0][:, :F]
    return torch.from_numpy(np.array(mag[::-1] if flip else mag)).cuda()  # (a writable copy: the fixture is shared)


class Bench:
    """One plan with the objects its composites take, and the input sets of a stream."""

    def __init__(self, pkg, torch, n, h, pairing=True):
        self.pkg, self.torch, self.n, self.h = pkg, torch, n, h
        self.plan = pkg.Plan(frame_size=n, hop_size=h, frame_pairing=pairing)
        self.feat = pkg.Features(self.plan, kind=pkg.FEAT_POWER)
        self.res = pkg.Resampler(UP, DOWN)
        self.res.prepare()
        self.taps = CR.make_filter(CONV_NF, CONV_K, seed=CONV_K)
        self.conv = pkg.Convolver(self.taps, block=CONV_B)
        self.conv.prepare()  # (the lazy uploads are not what is tested)
        assert self.conv.plan is not None

    def inputs(self, S, T, F_gl, seed, odd):
        """x for the plan's entries, the magnitudes and the convolver's x; odd: the
        sample rows sit at a 4-byte offset with a leading dimension of T + 1."""
        torch = self.torch
        x = HP.signal(torch, S, T, seed)
        xc = torch.from_numpy(CR.make_streams(S, T, CONV_B, seed)).cuda()
        if odd:
            x, xc = offset_rows(torch, x), offset_rows(torch, xc)
        return types.SimpleNamespace(x=x, xc=xc, mag=gl_mag(torch, self.n, self.h, S, F_gl, flip=odd), odd=odd)

    def calls(self, i):
        """The six composites in the order every stream queues them."""
        torch, plan = self.torch, self.plan
        return [spectrogram_call(torch, self.feat, i.x, i.odd), time_stretch_call(torch, plan, i.x, i.odd),
                pitch_shift_call(torch, plan, self.res, i.x, i.odd), hpss_call(torch, plan, i.x, i.odd),
                griffin_lim_call(torch, plan, i.mag, i.odd), convolve_call(torch, self.conv, i.xc, i.odd)]

    def close(self):
        self.feat.close()
        self.res.close()
        self.conv.close()
        self.plan.close()


def check_references(bench, oracle, i, serial, pairing):
    """Each composite's serial result against the reference of its own test module."""
    torch, plan, pkg = bench.torch, bench.plan, bench.pkg
    by_name = {c.name: outs for c, (outs, _) in zip(bench.calls(i), serial)}
    # crlot_spectrogram: per bin crlot_stft's power, bit for bit (tests/test_gpu_features.py)
    want = power_of(host(plan.stft(i.x)))
    assert np.array_equal(bits(host(by_name["spectrogram"][0])), bits(want)), "spectrogram"
    # the compositions on the public entries, bit for bit
    assert same_bits(torch, by_name["time_stretch"][0], TS.composed(torch, plan, i.x, RATE)), "time_stretch"
    assert same_bits(torch, by_name["pitch_shift"][0], PS.composed(torch, plan, bench.res, i.x)[0]), "pitch_shift"
    want_h, want_p = HP.compose(torch, plan, i.x)
    assert same_bits(torch, by_name["hpss"][0], want_h) and same_bits(torch, by_name["hpss"][1], want_p), "hpss"
    # (the fused Griffin-Lim shapes are the composition with the pairing off)
    fused = (bench.n, bench.h) in GLT.FUSED
    off = pkg.Plan(frame_size=bench.n, hop_size=bench.h, frame_pairing=False) if fused and pairing else plan
    want = GLT.compose(torch, off, i.mag, N_ITER, MOMENTUM)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0.05
    assert same_bits(torch, by_name["griffin_lim"][0], want), "griffin_lim"
    if off is not plan:
        off.close()
    # crlot_convolve: the hand composition, and float64 at tests/test_gpu_convolve.py's bars
    got = by_name["convolve"][0]
    assert same_bits(torch, got, CV.compose(bench.conv, i.xc)), "convolve"
    xc = host(i.xc)
    y64 = CR.convolve_f64(xc, bench.taps)
    ofig = CR.error_figures(CR.convolve_oracle_f32(oracle, xc, bench.taps, CONV_B), y64)
    for (l2, peak), (ol2, opeak) in zip(CR.error_figures(host(got), y64), ofig):
        bar_l2, bar_peak = CR.bars(ol2, opeak)
        assert l2 <= bar_l2 and peak <= bar_peak, (l2, peak, bar_l2, bar_peak)


# ------------------------------------------------------------------ 1. two streams of one plan
@pytest.mark.parametrize("n,h,pairing", PLANS)
def test_every_composite_on_two_streams(pkg, oracle, torch_cuda, n, h, pairing):
    """Stream A: 2 streams of 6 N + 77 samples in aligned rows; stream B: 5 streams of
    20 011 samples at a 4-byte offset, outputs with odd leading dimensions (the staged
    routes where the plan has them).  Both queue all six composites, call by call in
    turn, three times over, the first issuer alternating, behind a sleep on each stream."""
    torch = torch_cuda
    bench = Bench(pkg, torch, n, h, pairing)
    sets = [bench.inputs(2, 6 * n + 77, 24, 11, False), bench.inputs(5, 20_011, 17, 12, True)]
    calls = [bench.calls(i) for i in sets]
    serial = [[run_serial(torch, c) for c in cs] for cs in calls]
    for k in range(2):
        check_references(bench, oracle, sets[k], serial[k], pairing)
    assert "k_phase_voc" in serial[0][1][1]["kernels"] and "k_hpss_freq" in serial[0][3][1]["kernels"]
    if n != 1024:  # (N = 1024 has feature walkers for both of crlot_stft's routes: nothing staged)
        assert "k_feat_step" in serial[1][0][1]["kernels"], serial[1][0][1]
    if (n, h, pairing) == (1024, 256, False):  # the walk's output rows must be 8-byte aligned: B is staged
        assert "k_gather" in serial[1][1][1]["kernels"] and "k_gather" not in serial[0][1][1]["kernels"]
    if (n, h, pairing) == (960, 240, False):  # no walker takes the mixed radix: frames and spectra are staged
        for k in range(2):
            for j in (1, 2, 3, 4):
                assert {"k_frames_w", "k_gather"} <= set(serial[k][j][1]["kernels"]), (k, calls[k][j].name)
    streams = fresh_streams(torch, 2)
    reps = 3
    outs = [[[c.alloc() for c in calls[k]] for k in range(2)] for _ in range(reps)]
    torch.cuda.synchronize()
    for rep in range(reps):
        order = (0, 1) if rep % 2 == 0 else (1, 0)
        hold(torch, [streams[k] for k in order])
        for j in range(len(calls[0])):
            for k in order:
                with torch.cuda.stream(streams[k]):
                    calls[k][j].run(outs[rep][k][j])
        for k in range(2):
            assert not streams[k].query(), IDLE
    # what each stream's last call on each plan launched, read back per stream
    for k in range(2):
        for plan, last in ((bench.plan, 4), (bench.conv.plan, 5)):
            assert calls[k][last].plan is plan
            assert plan.last_launch(stream=streams[k].cuda_stream) == serial[k][last][1], (k, calls[k][last].name)
    assert serial[0][4][1] != serial[1][4][1] and serial[0][5][1] != serial[1][5][1]  # (A's records are not B's)
    torch.cuda.synchronize()
    for rep in range(reps):
        for k in range(2):
            for c, got, (want, _) in zip(calls[k], outs[rep][k], serial[k]):
                assert all_same(torch, got, want), (rep, "AB"[k], c.name)
    bench.close()


# ------------------------------------------------------------------ 2. growth and re-carving in a queue
def test_growth_and_recarving_in_one_queue(pkg, oracle, torch_cuda):
    """512 / 128 on one side stream, nothing synchronised in between.  The slot's
    workspace starts at the small crlot_time_stretch's need: S = 1, T = 3072, rate 1.3:
    F = 24, F' = 19, (24 + 19) rows x 514 floats x 4 bytes = 88 408 bytes (frame pairs:
    nothing staged; F' < 64: no chunk sums).  crlot_hpss with S = 8, T = 20 000 then
    needs F = 157 rows of 514 (spectrum) + 3 x 257 (medians, two masks) floats per stream:
    8 x 157 x 1285 x 4 = 6 455 840 bytes, so the workspace is freed and allocated anew in
    stream order while the first call has not run.  Every later call carves the grown
    buffer its own way: the staged round trips put frames and spectra at its start, the
    chunked vocoder its sums, the staged spectrogram and Griffin-Lim their regions."""
    torch = torch_cuda
    n, h = 512, 128
    bins, row = n // 2 + 1, n + 2
    plan = pkg.Plan(frame_size=n, hop_size=h)
    feat = pkg.Features(plan, kind=pkg.FEAT_POWER)
    x1 = HP.signal(torch, 1, 6 * n, 31)
    x8 = HP.signal(torch, 8, 20_000, 32)
    F1, F8 = plan.frame_count(6 * n), plan.frame_count(20_000)
    Fp1 = pkg.stretch_frame_count(F1, RATE)
    assert (F1, Fp1, F8) == (24, 19, 157)
    small, big = (F1 + Fp1) * row * 4, 8 * F8 * (row + 3 * bins) * 4
    assert (small, big) == (88_408, 6_455_840) and big > small
    x3 = offset_rows(torch, HP.signal(torch, 3, 5000, 33))
    L3 = plan.output_length(5000)
    mask = torch.rand((plan.frame_count(5000), bins), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    spec = torch.from_numpy(np.array(TS.spectra(n, 40, 2))).cuda()
    Fp = pkg.stretch_frame_count(40, RATE)
    mag = gl_mag(torch, n, h, 3, 24)

    def masked(o):
        plan.set_frame_pairing(False)  # (frame pairs take any 4-byte aligned rows: the walk does not)
        plan.set_spectral_mask(mask)
        try:
            plan.roundtrip(x3, o[0])
        finally:
            plan.set_spectral_mask(None)
            plan.set_frame_pairing(True)

    def chunked(o):
        plan.set_chunks(3)
        try:
            plan.phase_vocoder(spec, RATE, out=o[0])
        finally:
            plan.set_chunks(0)

    calls = [
        time_stretch_call(torch, plan, x1, False),
        hpss_call(torch, plan, x8, False),
        time_stretch_call(torch, plan, x1, False),
        make_call("roundtrip", plan, lambda: [out_rows(torch, (3, L3), True)], lambda o: plan.roundtrip(x3, o[0])),
        make_call("masked roundtrip", plan, lambda: [out_rows(torch, (3, L3), True)], masked),
        make_call("phase_vocoder", plan,
                  lambda: [torch.view_as_complex(torch.full((2, Fp, bins, 2), NAN, device="cuda"))], chunked),
        spectrogram_call(torch, feat, x3, True),
        griffin_lim_call(torch, plan, mag, True),
    ]
    serial = [run_serial(torch, c) for c in calls]
    recs = [rec["kernels"] for _, rec in serial]
    assert "k_synth" in recs[3] and "k_gather" in recs[3], recs[3]           # staged: frames in the workspace
    assert "k_spec_step" in recs[4] and "k_gather" in recs[4], recs[4]       # staged: spectra and frames
    assert "k_phase_voc_sums" in recs[5], recs[5]                            # the sums are in the workspace
    assert "k_feat_step" in recs[6], recs[6]
    check_vs_oracle(oracle, host(x3), host(serial[3][0][0]), n, h, (0, 2))
    s, = fresh_streams(torch, 1)
    outs = [c.alloc() for c in calls]
    torch.cuda.synchronize()
    hold(torch, [s])
    with torch.cuda.stream(s):
        for c, o in zip(calls, outs):
            c.run(o)
    assert not s.query(), IDLE
    torch.cuda.synchronize()
    assert plan._mask is None
    for c, got, (want, _) in zip(calls, outs, serial):
        assert all_same(torch, got, want), c.name
    assert all_same(torch, outs[0], outs[2])
    feat.close()
    plan.close()


# ------------------------------------------------------------------ 3. slot recycling
def recycling_inputs(pkg, torch, k):
    """Two plans of one configuration (960 / 240, pairing off: both halves of
    crlot_time_stretch staged) -- the serial runs go to the second, so the plan under
    test has no slot but those of the k side streams -- and k calls of differing sizes
    with their serial results."""
    n, h = 960, 240
    plan = pkg.Plan(frame_size=n, hop_size=h, frame_pairing=False)
    twin = pkg.Plan(frame_size=n, hop_size=h, frame_pairing=False)
    xs = [HP.signal(torch, 2, 6 * n + h * i + 7, 50 + i) for i in range(k)]
    calls = [time_stretch_call(torch, plan, x, i % 2 == 1) for i, x in enumerate(xs)]
    serial = []
    for i, x in enumerate(xs):
        outs, rec = run_serial(torch, time_stretch_call(torch, twin, x, i % 2 == 1))
        assert "k_frames_w" in rec["kernels"] and "k_gather" in rec["kernels"], rec
        serial.append(outs)
    assert same_bits(torch, serial[0][0], TS.composed(torch, twin, xs[0], RATE))
    twin.close()
    return plan, calls, serial


def test_slots_recycle_past_sixteen_streams(pkg, torch_cuda):
    """20 streams, one staged crlot_time_stretch each, one after another: the 17th to
    20th take the slots of the first four, which then run again on fresh slots."""
    torch = torch_cuda
    plan, calls, serial = recycling_inputs(pkg, torch, 20)
    streams = fresh_streams(torch, 20)
    order = list(range(20)) + [0, 1, 2, 3]
    outs = [calls[i].alloc() for i in order]
    torch.cuda.synchronize()
    for i, o in zip(order, outs):
        with torch.cuda.stream(streams[i]):
            calls[i].run(o)  # (an error code raises)
    torch.cuda.synchronize()
    for i, o in zip(order, outs):
        assert all_same(torch, o, serial[i]), i
    plan.close()


def test_slot_recycled_under_work_in_flight(pkg, torch_cuda):
    """Streams 0 to 15 each hold a sleep and a queued crlot_time_stretch, which fills
    the plan's 16 slots; the call on stream 16 takes the oldest slot, stream 0's, whose
    work has not run: the device is drained before that slot's buffers are freed."""
    torch = torch_cuda
    plan, calls, serial = recycling_inputs(pkg, torch, 17)
    streams = fresh_streams(torch, 17)
    outs = [c.alloc() for c in calls]
    torch.cuda.synchronize()
    hold(torch, streams[:16])
    for i in range(16):
        with torch.cuda.stream(streams[i]):
            calls[i].run(outs[i])
    for i in range(16):
        assert not streams[i].query(), IDLE
    with torch.cuda.stream(streams[16]):
        calls[16].run(outs[16])
    torch.cuda.synchronize()
    for i in range(17):
        assert all_same(torch, outs[i], serial[i]), i
    plan.close()


# ------------------------------------------------------------------ 4. host threads
def test_two_host_threads_mixed_entries(pkg, torch_cuda):
    """Two host threads on one 512 / 128 plan, a stream each: one loops
    crlot_time_stretch and crlot_griffin_lim (which switches the plan's pairing off
    under the plan's lock while it runs), the other crlot_pitch_shift and the staged
    crlot_spectrogram; four rounds each."""
    torch = torch_cuda
    bench = Bench(pkg, torch, 512, 128)
    a, b = bench.inputs(3, 6 * 512 + 77, 24, 41, False), bench.inputs(4, 9000, 24, 42, True)
    mine = [[time_stretch_call(torch, bench.plan, a.x, False), griffin_lim_call(torch, bench.plan, a.mag, False)],
            [pitch_shift_call(torch, bench.plan, bench.res, b.x, True), spectrogram_call(torch, bench.feat, b.x, True)]]
    serial = [[run_serial(torch, c)[0] for c in cs] for cs in mine]
    torch.cuda.synchronize()
    streams = fresh_streams(torch, 2)
    results, errors = [[], []], []
    barrier = threading.Barrier(2)

    def work(i):
        try:
            barrier.wait(timeout=30)
            with torch.cuda.stream(streams[i]):
                for _ in range(4):
                    for c in mine[i]:
                        o = c.alloc()
                        c.run(o)
                        results[i].append(o)
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
        assert len(results[i]) == 8
        for j, got in enumerate(results[i]):
            assert all_same(torch, got, serial[i][j % 2]), (i, j, mine[i][j % 2].name)
    bench.close()


# ------------------------------------------------------------------ 5. capture and replay
@pytest.mark.parametrize("n,h,odd", [(512, 128, False), (960, 240, True)])
def test_capture_and_replay(pkg, torch_cuda, n, h, odd):
    """After a warm call of the same shape on the stream -- the slot exists and is
    large enough, every launcher has made its one-time queries -- the host path of each
    of these entries only launches kernels and asynchronous device-to-device copies
    (crlot_griffin_lim into 4-byte aligned rows, crlot_convolve's crop), so the call can
    be captured alone on that stream and replayed.  512 / 128: the fused Griffin-Lim
    walk; 960 / 240 with odd leading dimensions: the staged one and the copies."""
    torch = torch_cuda
    bench = Bench(pkg, torch, n, h)
    i = bench.inputs(3, 6 * n + 77, 24, 61, odd)
    calls = bench.calls(i)
    assert [c.name for c in calls] == ["spectrogram", "time_stretch", "pitch_shift", "hpss", "griffin_lim", "convolve"]
    serial = [run_serial(torch, c) for c in calls]
    assert "k_feat_step" in serial[0][1]["kernels"]
    assert ("k_gl_iter" in serial[4][1]["kernels"]) == ((n, h) in GLT.FUSED)
    s, = fresh_streams(torch, 1)
    for c, (want, _) in zip(calls, serial):
        outs = c.alloc()
        with torch.cuda.stream(s):
            c.run(outs)  # warm
        s.synchronize()
        assert all_same(torch, outs, want), (c.name, "warm")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            c.run(outs)
        for replay in range(2):
            for o in outs:
                o.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert all_same(torch, outs, want), (c.name, replay)
    bench.close()
