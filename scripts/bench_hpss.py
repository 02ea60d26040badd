#!/usr/bin/env python3
"""Measure harmonic / percussive separation (Plan.hpss) against what it replaces.

Cases: 1024/256 and 512/128; --few-streams and --streams x --samples (10 s of 48 kHz
audio by default); kernel_size 31, power 2, margins 1 (librosa's defaults).  Arms,
timed in one process, alternating by round, each with its own warm-up and device
events around its calls:
  a   Plan.hpss
  b   the four-call composition: Plan.stft, Plan.hpss_masks, and Plan.istft_ola twice,
      each under Plan.set_spectral_mask
  c   Plan.stft and the two masked Plan.istft_ola with precomputed masks: the floor
      the masks add to
  d   the masks in torch on the same spectra: abs, index-gathered reflect padding,
      unfold(31).median(-1) on both axes, the soft mask; then arm c's calls.  The
      unfolded copy is 31 x the magnitudes, so the batch goes in slices of
      --torch-slice streams
Before timing, at the timed size: a equals b bit for bit, and d's masks are compared
with the library's (largest absolute difference reported).  Per case: ms per call,
Msamples/s, a/c and d/a, and the mask kernels' own time (b's hpss_masks call alone).
Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1024, 256), (512, 128))
WIN = 31


def time_leg(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def reflect_index(torch, n, r, device):
    j = torch.remainder(torch.arange(-r, n + r, device=device), 2 * n)
    return torch.where(j < n, j, 2 * n - 1 - j)


def torch_masks(torch, spec, slice_streams):
    """librosa.decompose.hpss(mask=True) restated in torch ops (power 2, margins 1)."""
    S, F, bins = spec.shape
    r = (WIN - 1) // 2
    it, ib = reflect_index(torch, F, r, spec.device), reflect_index(torch, bins, r, spec.device)
    mh = torch.empty((S, F, bins), dtype=torch.float32, device=spec.device)
    mp = torch.empty_like(mh)
    tiny = torch.finfo(torch.float32).tiny
    for s0 in range(0, S, slice_streams):
        m = spec[s0:s0 + slice_streams].abs()
        h = m.index_select(1, it).unfold(1, WIN, 1).median(-1).values
        p = m.index_select(2, ib).unfold(2, WIN, 1).median(-1).values
        Z = torch.maximum(h, p)
        bad = Z < tiny
        Z = torch.where(bad, torch.ones_like(Z), Z)
        a, b = (h / Z) ** 2, (p / Z) ** 2
        d = a + b
        mh[s0:s0 + slice_streams] = torch.where(bad, 0.5, a / d)
        mp[s0:s0 + slice_streams] = torch.where(bad, 0.5, b / d)
    return mh, mp


def run_case(pkg, torch, n, h, S, T, rounds, calls, warmup, torch_slice):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC0FFEE ^ S ^ n)
    t = torch.arange(T, device=dev, dtype=torch.float32)
    f0 = 0.01 + 0.05 * torch.rand((S, 1), generator=g, device=dev)
    x = 0.5 * torch.sin(2 * torch.pi * f0 * t) + 0.05 * torch.randn((S, T), generator=g, device=dev)
    x[:, 1000::12000] += 1.0  # a click every 0.25 s
    del t
    plan = pkg.Plan(frame_size=n, hop_size=h)
    F = plan.frame_count(T)
    bins = n // 2 + 1
    L = F * h
    y_h = torch.empty((S, L), dtype=torch.float32, device=dev)
    y_p = torch.empty_like(y_h)
    spec = torch.empty((S, F, bins), dtype=torch.complex64, device=dev)
    m_h = torch.empty((S, F, bins), dtype=torch.float32, device=dev)
    m_p = torch.empty_like(m_h)

    def invert(mh, mp):
        plan.set_spectral_mask(mh)
        plan.istft_ola(spec, y_h)
        plan.set_spectral_mask(mp)
        plan.istft_ola(spec, y_p)
        plan.set_spectral_mask(None)

    def arm_a():
        plan.hpss(x, y_h=y_h, y_p=y_p)

    def arm_b():
        plan.stft(x, spec)
        plan.hpss_masks(spec, mask_h=m_h, mask_p=m_p)
        invert(m_h, m_p)

    def arm_c():
        plan.stft(x, spec)
        invert(m_h, m_p)

    def arm_d():
        plan.stft(x, spec)
        invert(*torch_masks(torch, spec, torch_slice))

    def masks_only():
        plan.hpss_masks(spec, mask_h=m_h, mask_p=m_p)

    # ---- correctness at the timed size
    arm_b()
    want = (y_h.clone(), y_p.clone())
    y_h.zero_()
    y_p.zero_()
    arm_a()
    rec = plan.last_launch()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip((y_h, y_p), want))
    del want
    if not same:
        raise SystemExit(f"{n}/{h} S={S}: a does not equal b bit for bit")
    tm_h, tm_p = torch_masks(torch, spec[:torch_slice], torch_slice)
    mask_gap = max(float((tm_h - m_h[:torch_slice]).abs().max()), float((tm_p - m_p[:torch_slice]).abs().max()))
    del tm_h, tm_p

    # ---- timing
    legs = {"a": arm_a, "b": arm_b, "c": arm_c, "d": arm_d, "masks": masks_only}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(time_leg(torch, fn, calls))
    samples = float(S) * T
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms_per_call": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                     "msamples_per_s": round(samples / (med * 1e-3) / 1e6, 1), "calls": rounds * calls}
    res["a"].update({"kernels_last_slice": rec["kernels"], "n_chunks": rec["n_chunks"], "grid": rec["grid"]})
    res["a_over_c"] = round(res["a"]["ms_per_call"] / res["c"]["ms_per_call"], 3)
    res["d_over_a"] = round(res["d"]["ms_per_call"] / res["a"]["ms_per_call"], 3)
    res["b_over_a"] = round(res["b"]["ms_per_call"] / res["a"]["ms_per_call"], 3)
    # the mask kernels alone: bins medians of 31 per (stream, frame) on each axis
    res["masks"]["gbins_per_s"] = round(float(S) * F * bins / (res["masks"]["ms_per_call"] * 1e-3) / 1e9, 2)
    res["check"] = {"a_bit_equal_b": same, "torch_mask_max_abs_gap": mask_gap}
    res["frames"] = F
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--few-streams", type=int, default=64)
    ap.add_argument("--samples", type=int, default=480_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1, help="calls per arm and round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--torch-slice", type=int, default=16, help="streams per slice of the torch baseline")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    out = {"suite": "hpss", "kernel_size": WIN, "power": 2, "margin": 1.0,
           "build": {k: v for k, v in pkg.build_info().items() if k != "path"},
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for n, h in SHAPES:
        for S in (a.few_streams, a.streams):
            key = f"{n}/{h} S={S} T={a.samples}"
            out["cases"][key] = run_case(pkg, torch, n, h, S, a.samples, a.rounds, a.calls, a.warmup, a.torch_slice)
            print(key, json.dumps(out["cases"][key]), file=sys.stderr, flush=True)
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
