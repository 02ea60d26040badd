"""Where the kernels read and write: every walker family and entry, with guards.

The parity tests judge what a kernel computes.  An overrun of stream s lands in
the first samples of stream s+1 of a contiguous batch and races with that
stream's own correct store, so a parity test sees it sometimes or never.  Here
every operand of a call -- input rows, mask, spectra, output rows -- is a view
into ONE flat allocation with a guard band of at least N + H floats in front of
row 0, between rows and behind the last row.  Input guards (and the padding
inside padded spectra and masks) hold NaN, output guards a sentinel bit
pattern.  After the call:

  1. everything outside the output elements is bit-identical to before the call,
     compared as bits on the device: output guards still hold the sentinel
     (in front of rows, between them, behind them), inputs and their guards are
     untouched;
  2. the output is bit-equal to the same call on tight tensors holding the same
     data (rows end to end, one float of padding where an odd length would
     otherwise make the row stride odd: the walkers other than K_pair need
     8-byte rows; the bands in front of the first row and behind the last stay,
     and the same checks run), both calls having run the same kernels; where the
     routes differ (odd row strides, padded spectra on the staged path) the two
     agree within test_gpu_parity's REL_L2 / MAX_ABS bar;
  3. the output is finite: no NaN of an input guard was read.

The kernels each call ran are asserted against the literal lists in ROUTES /
ODD_ROUTES, so no shape can quietly fall onto another path.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_close, host

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5C3D2  # a NaN bit pattern no kernel produces
FQ = {"boundary_mode": 2, "pad_mode": 1}  # FrameQueue framing, centred, reflect padding

# name -> (N, H, plan options)
SHAPES = {
    "1024/256": (1024, 256, {}),
    "1024/1024": (1024, 1024, {}),
    "1024/256 unpaired": (1024, 256, {"frame_pairing": False}),
    "512/128": (512, 128, {}),
    "2048/512": (2048, 512, {}),
    "2048/256": (2048, 256, {}),
    "4096/1024": (4096, 1024, {}),
    "4096/1024 unpaired": (4096, 1024, {"frame_pairing": False}),
    "256/128": (256, 128, {}),
    "960/240": (960, 240, {}),
    "480/120": (480, 120, {}),
    "480/160": (480, 160, {}),
    "882/441": (882, 441, {}),
    "1000/250": (1000, 250, {}),
    "640/320": (640, 320, {}),
    "1764/441": (1764, 441, {}),
    "1920/480": (1920, 480, {}),
    "1024/300 staged": (1024, 300, {}),
    "998/499 staged": (998, 499, {}),
    "1024/256 framequeue": (1024, 256, FQ),
    "960/480 framequeue": (960, 480, FQ),
}

ENTRIES = ["roundtrip", "roundtrip_gain", "mask_shared", "mask_stream", "stft", "istft_ola", "istft_stft",
           "interleaved2", "interleaved6"]

# The kernels each entry runs, in launch order (the padded call and the tight call alike unless
# TIGHT_ROUTES says otherwise).  "mask" serves both masked entries; istft_stft runs "stft" then "istft_ola".
ROUTES = {
    "1024/256": {
        "roundtrip": ["k_pair_hot", "k_pair_fix"], "roundtrip_gain": ["k_pair_hot", "k_pair_fix"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_pair_hot", "k_pair_fix"],
        "interleaved6": ["k_deinterleave", "k_pair_hot", "k_pair_fix", "k_interleave"]},
    "1024/1024": {
        "roundtrip": ["k_pair_all"], "roundtrip_gain": ["k_pair_all"], "mask": ["k_stft_masked"], "stft": ["k_stft"],
        "istft_ola": ["k_istft"], "interleaved2": ["k_deinterleave", "k_pair_all", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair_all", "k_interleave"]},
    "1024/256 unpaired": {
        "roundtrip": ["k_fused2"], "roundtrip_gain": ["k_fused2"], "mask": ["k_stft_masked"], "stft": ["k_stft"],
        "istft_ola": ["k_istft"], "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "512/128": {
        "roundtrip": ["k_pair512_hot", "k_pair512"], "roundtrip_gain": ["k_pair512"], "mask": ["k_pair_mask"],
        "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "2048/512": {
        "roundtrip": ["k_pair2k_hot", "k_pair2k"], "roundtrip_gain": ["k_pair2k"], "mask": ["k_pair_mask"],
        "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "2048/256": {
        "roundtrip": ["k_pair2k"], "roundtrip_gain": ["k_pair2k"], "mask": ["k_pair_mask"], "stft": ["k_pair_stft"],
        "istft_ola": ["k_pair_istft"], "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "4096/1024": {
        "roundtrip": ["k_pair4k_hot", "k_pair4k"], "roundtrip_gain": ["k_pair4k_hot", "k_pair4k"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "4096/1024 unpaired": {
        "roundtrip": ["k_fused_wg"], "roundtrip_gain": ["k_fused_wg"], "mask": ["k_stft_masked"], "stft": ["k_stft"],
        "istft_ola": ["k_istft"], "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "256/128": {
        "roundtrip": ["k_fused"], "roundtrip_gain": ["k_fused"], "mask": ["k_stft_masked"], "stft": ["k_stft"],
        "istft_ola": ["k_istft"], "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "960/240": {
        "roundtrip": ["k_pair15", "k_fused_any"], "roundtrip_gain": ["k_pair15", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"]},
    "480/120": {
        "roundtrip": ["k_pair15", "k_fused_any"], "roundtrip_gain": ["k_pair15", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"]},
    "480/160": {
        "roundtrip": ["k_pair15", "k_fused_any"], "roundtrip_gain": ["k_pair15", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"]},
    "882/441": {
        "roundtrip": ["k_pairn", "k_fused_any"], "roundtrip_gain": ["k_pairn", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"]},
    "1000/250": {
        "roundtrip": ["k_pairn", "k_fused_any"], "roundtrip_gain": ["k_pairn", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"]},
    "640/320": {
        "roundtrip": ["k_pairn", "k_fused_any"], "roundtrip_gain": ["k_pairn", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"]},
    "1764/441": {
        "roundtrip": ["k_pairn", "k_fused_any"], "roundtrip_gain": ["k_pairn", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pairn", "k_fused_any", "k_interleave"]},
    "1920/480": {
        "roundtrip": ["k_pair30", "k_fused_any"], "roundtrip_gain": ["k_pair30", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair30", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair30", "k_fused_any", "k_interleave"]},
    "1024/300 staged": {
        "roundtrip": ["k_synth", "k_gather"], "roundtrip_gain": ["k_synth", "k_gather"],
        "mask": ["k_stft", "k_spec_step", "k_fft", "k_gather"], "stft": ["k_stft"],
        "istft_ola": ["k_spec_step", "k_fft", "k_gather"],
        "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "998/499 staged": {
        "roundtrip": ["k_fused_any"], "roundtrip_gain": ["k_fused_any"],
        "mask": ["k_frames_w", "k_fft_any", "k_spec_step", "k_fft_any", "k_gather"],
        # padded spectra: one rfft launch per stream (stft_impl); by S
        "stft": {3: ["k_frames_w", "k_fft_any", "k_fft_any", "k_fft_any"],
                 4: ["k_frames_w", "k_fft_any", "k_fft_any", "k_fft_any", "k_fft_any"]},
        "istft_ola": ["k_spec_step", "k_fft_any", "k_gather"],
        "interleaved2": ["k_deinterleave", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_fused_any", "k_interleave"]},
    "1024/256 framequeue": {
        "roundtrip": ["k_pair_all"], "roundtrip_gain": ["k_pair_all"], "mask": ["k_pair_mask"],
        "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair_all", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair_all", "k_interleave"]},
    "960/480 framequeue": {
        "roundtrip": ["k_fused_any"], "roundtrip_gain": ["k_fused_any"], "mask": ["k_pair_mask"],
        "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_fused_any", "k_interleave"]},
}

# The staged spectral entries look at the spectra's layout: dense spectra take one
# rfft launch for all streams and, with no gain or mask, no copy through k_spec_step
# (stft_impl / istft_impl: ld_spec == F * ld_frame).  The tight call's lists where they differ:
TIGHT_ROUTES = {
    "1024/300 staged": {"istft_ola": ["k_fft", "k_gather"]},
    "998/499 staged": {"stft": ["k_frames_w", "k_fft_any"], "istft_ola": ["k_fft_any", "k_gather"]},
}

# rows 4-byte aligned only (odd row strides): what the guards in abi.cpp document
ODD_ROUTES = {
    "1024/256": {
        "roundtrip": ["k_pair_hot", "k_pair_fix"], "roundtrip_gain": ["k_pair_hot", "k_pair_fix"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_pair_hot", "k_pair_fix"],
        "interleaved6": ["k_deinterleave", "k_pair_hot", "k_pair_fix", "k_interleave"]},
    "512/128": {
        "roundtrip": ["k_synth", "k_gather"], "roundtrip_gain": ["k_synth", "k_gather"], "mask": ["k_pair_mask"],
        "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_synth", "k_gather", "k_interleave"]},
    "960/240": {
        "roundtrip": ["k_pair15", "k_fused_any"], "roundtrip_gain": ["k_pair15", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"]},
    "480/120": {
        "roundtrip": ["k_pair15", "k_fused_any"], "roundtrip_gain": ["k_pair15", "k_fused_any"],
        "mask": ["k_pair_mask"], "stft": ["k_pair_stft"], "istft_ola": ["k_pair_istft"],
        "interleaved2": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"],
        "interleaved6": ["k_deinterleave", "k_pair15", "k_fused_any", "k_interleave"]},
}


def route_key(entry):
    return {"mask_shared": "mask", "mask_stream": "mask"}.get(entry, entry)


def expected_route(table, shape, entry, S, tight=False):
    if entry == "istft_stft":  # two calls: the stft, then the istft_ola
        return expected_route(table, shape, "stft", S, tight) + expected_route(table, shape, "istft_ola", S, tight)
    key = route_key(entry)
    if tight and key in TIGHT_ROUTES.get(shape, {}):
        return TIGHT_ROUTES[shape][key]
    want = table[shape][key]
    return want[S] if isinstance(want, dict) else want


class Arena:
    """One flat allocation for every operand of a call.  add() reserves
    [guard | lead | the operand's extent | tail | guard]; inputs (and their lead /
    tail padding) are filled with NaN, outputs with the sentinel."""

    def __init__(self, guard):
        self.guard, self.size, self.ops = guard, 0, []

    def add(self, shape, strides, out, lead=0, tail=0):
        extent = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
        begin = self.size
        off = begin + self.guard + lead
        self.size = off + extent + tail + self.guard
        self.size += self.size & 1  # the next operand starts 8-byte aligned
        self.ops.append((off, tuple(shape), tuple(strides), out, begin, self.size))
        return len(self.ops) - 1

    def build(self, torch):
        self.i32 = torch.full((self.size,), SENTINEL, dtype=torch.int32, device="cuda")
        self.f32 = self.i32.view(torch.float32)
        for off, shape, strides, out, begin, end in self.ops:
            assert off % 2 == 0 and off - begin >= self.guard
            if not out:
                self.f32[begin:end] = float("nan")
        return self

    def view(self, i, buf=None):
        off, shape, strides = self.ops[i][:3]
        return (self.f32 if buf is None else buf).as_strided(shape, strides, off)

    def check_untouched(self, torch, before, what):
        """Everything but the output elements holds the bits it held before the call."""
        after = self.i32.clone()
        for i, op in enumerate(self.ops):
            if op[3]:
                self.view(i, after).copy_(self.view(i, before))
        if not torch.equal(after, before):
            bad = torch.nonzero(after != before).flatten()
            where = [(int(b), next((j, int(b) - op[0]) for j, op in enumerate(self.ops) if op[4] <= int(b) < op[5]))
                     for b in bad[:4]]
            raise AssertionError(f"{what}: {bad.numel()} elements outside the output changed; "
                                 f"first (flat index, (operand, offset from its first element)): {where}")


def even(v):
    return v + (v & 1)


def layout(entry, S, T, F, n, h, guard, odd):
    """The operands of one call as Arena reservations.  guard = 0: the tight
    layout (rows end to end, row strides rounded up to even; the guard bands in
    front of the first row and behind the last stay: a store past the last row
    of a dense batch has nowhere else to show).  odd: row strides of the real
    rows are odd (spectra keep their even strides: complex pairs)."""
    bins, L = n // 2 + 1, F * h
    a = Arena(even(n + h))
    ops = {}

    def ld(width):
        v = even(width + guard)
        return v + 1 if odd else v

    if entry.startswith("interleaved"):
        C = int(entry[len("interleaved"):])
        ops["x"] = a.add((S, T, C), (ld(T * C), C, 1), False)
        ops["y"] = a.add((S, L, C), (ld(L * C), C, 1), True)
        return a, ops
    pad_f, pad_b = (2, 3) if guard else (0, 0)  # spectra: (S, F+2, bins+3) complex, the call's rows in the middle
    row = 2 * (bins + pad_b)
    spec_shape, spec_strides = (S, F, bins, 2), ((F + pad_f) * row + even(guard), row, 2, 1)
    lead, tail = (row, row + 2 * pad_b) if guard else (0, 0)
    if entry != "istft_ola":
        ops["x"] = a.add((S, T), (ld(T), 1), False)
    if entry in ("mask_shared", "mask_stream"):
        mrow = bins + (2 if guard else 0)
        if entry == "mask_shared":
            ops["mask"] = a.add((F, bins), (mrow, 1), False, tail=mrow - bins)
        else:
            ops["mask"] = a.add((S, F, bins), ((F + (1 if guard else 0)) * mrow, mrow, 1), False, tail=mrow - bins)
    if entry in ("stft", "istft_stft"):
        ops["spec"] = a.add(spec_shape, spec_strides, True, lead, tail)
    if entry == "istft_ola":
        ops["spec"] = a.add(spec_shape, spec_strides, False, lead, tail)
    if entry not in ("stft",):
        ops["y"] = a.add((S, L), (ld(L), 1), True)
    return a, ops


def run_entry(torch, plan, entry, t):
    """The call itself on the operand views t; returns (outputs, kernels)."""
    ks = []

    def launched():
        ks.extend(plan.last_launch()["kernels"])

    out = {}
    if entry in ("roundtrip", "roundtrip_gain"):
        plan.roundtrip(t["x"], t["y"])
        launched()
        out["y"] = t["y"]
    elif entry in ("mask_shared", "mask_stream"):
        plan.set_spectral_mask(t["mask"])
        try:
            plan.roundtrip(t["x"], t["y"])
            launched()
        finally:
            plan.set_spectral_mask(None)
        out["y"] = t["y"]
    elif entry == "stft":
        plan.stft(t["x"], torch.view_as_complex(t["spec"]))
        launched()
        out["spec"] = t["spec"]
    elif entry == "istft_ola":
        plan.istft_ola(torch.view_as_complex(t["spec"]), t["y"])
        launched()
        out["y"] = t["y"]
    elif entry == "istft_stft":
        spec = torch.view_as_complex(t["spec"])
        plan.stft(t["x"], spec)
        launched()
        plan.istft_ola(spec, t["y"])
        launched()
        out["spec"], out["y"] = t["spec"], t["y"]
    else:
        plan.roundtrip_interleaved(t["x"], t["y"])
        launched()
        out["y"] = t["y"]
    torch.cuda.synchronize()
    return out, ks


def one_call(torch, plan, entry, S, T, n, h, odd, data):
    """The guarded call and the tight call; returns (kernels guarded, kernels tight)."""
    F = plan.frame_count(T)
    assert F >= 1
    res = []
    for guard in (even(n + h), 0):
        arena, ops = layout(entry, S, T, F, n, h, guard, odd and guard > 0)
        arena.build(torch)
        t = {k: arena.view(i) for k, i in ops.items()}
        for k in ("x", "mask", "spec"):
            if k in t and not arena.ops[ops[k]][3]:
                t[k].copy_(data[k].reshape(t[k].shape))
        before = arena.i32.clone()
        what = f"{entry} S={S} T={T} {'odd ' if odd else ''}{'guarded' if guard else 'tight'}"
        out, ks = run_entry(torch, plan, entry, t)
        arena.check_untouched(torch, before, what)
        for k, v in out.items():
            assert bool(torch.isfinite(v).all()), f"{what}: {k} is not finite (a guard was read, or never written)"
        res.append(({k: v.clone() for k, v in out.items()}, ks))
    (got, ks_g), (ref, ks_t) = res
    for k in got:
        if ks_g == ks_t:
            assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), \
                f"{entry} S={S} T={T}: {k} differs from the tight call ({ks_g})"
        else:
            g, r = host(got[k]).reshape(S, -1), host(ref[k]).reshape(S, -1)
            for s in range(S):
                assert_close(g[s], r[s], float(np.max(np.abs(r[s]))), f"{entry} S={S} T={T} {k} stream {s}",
                             float(np.linalg.norm(r[s].astype(np.float64))))
    return ks_g, ks_t


def make_plan(pkg, shape, entry):
    n, h, opts = SHAPES[shape]
    plan = pkg.Plan(frame_size=n, hop_size=h, **opts)
    if entry == "roundtrip_gain":
        plan.set_spectral_gain(np.linspace(1.0, 0.5, n // 2 + 1, dtype=np.float32))
    return plan, n, h


def make_data(torch, plan, entry, S, T, n, seed):
    """x, mask and (for istft_ola) spectra, drawn on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    F, bins = plan.frame_count(T), n // 2 + 1
    C = int(entry[len("interleaved"):]) if entry.startswith("interleaved") else 1
    data = {"x": (torch.rand((S, T * C), generator=g, device="cuda") * 2 - 1) * 0.5}
    if entry in ("mask_shared", "mask_stream"):
        data["mask"] = torch.rand((F, bins) if entry == "mask_shared" else (S, F, bins), generator=g,
                                  device="cuda") * 0.75 + 0.25
    if entry == "istft_ola":
        xe = torch.zeros((S, even(T)), device="cuda")
        xe[:, :T] = data["x"]
        data["spec"] = torch.view_as_real(plan.stft(xe[:, :T]))
    return data


def lengths(n, h):
    return [9 * n + 37, h - 1, n + 1]


def calls(n, h):
    """(T, chunks): a ragged T whose last frame is partial, T = H - 1 (one partial
    frame) and N + 1, each under one chunk and under three (chunk seams)."""
    return [(T, chunks) for T in lengths(n, h) for chunks in (1, 3)]


@pytest.mark.parametrize("S", [3, 4])
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_containment(pkg, torch_cuda, shape, entry, S):
    """S = 3: a lone last stream where streams pair up (N = 480); S = 4: two full pairs."""
    torch = torch_cuda
    plan, n, h = make_plan(pkg, shape, entry)
    want, tight = expected_route(ROUTES, shape, entry, S), expected_route(ROUTES, shape, entry, S, tight=True)
    try:
        for T, chunks in calls(n, h):
            data = make_data(torch, plan, entry, S, T, n, seed=n + h + S + T)
            plan.set_chunks(chunks)
            ks_g, ks_t = one_call(torch, plan, entry, S, T, n, h, False, data)
            assert ks_g == want and ks_t == tight, (shape, entry, S, T, chunks, ks_g, ks_t)
    finally:
        plan.set_chunks(0)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", ["1024/256", "512/128", "960/240", "480/120"])
def test_containment_odd_row_stride(pkg, torch_cuda, shape, entry):
    """Rows 4-byte aligned only.  K_pair (N = 1024) and the N = 960 / 480 walkers move
    single floats and keep their route; the other fused walkers move float2 and
    the call leaves them for the route ODD_ROUTES names (use_fused, istft_walk_ok)."""
    torch = torch_cuda
    plan, n, h = make_plan(pkg, shape, entry)
    try:
        for S, chunks in ((3, 1), (4, 3)):
            want, tight = expected_route(ODD_ROUTES, shape, entry, S), expected_route(ROUTES, shape, entry, S)
            T = lengths(n, h)[0]
            data = make_data(torch, plan, entry, S, T, n, seed=n + h + S)
            plan.set_chunks(chunks)
            ks_g, ks_t = one_call(torch, plan, entry, S, T, n, h, True, data)
            assert ks_g == want and ks_t == tight, (shape, entry, S, chunks, ks_g, ks_t)
    finally:
        plan.set_chunks(0)
