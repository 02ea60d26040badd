#!/usr/bin/env python3
"""Measure the fused spectrogram features against what a user does without them.

Shapes: --streams x --samples seeded input at 1024/256 (the frame-pair feature
walker), 1024/300 (one frame per wave) and 4096/1024 (the staged form).  Legs,
timed in one process, alternating, each with its own warm-up and device events
around its calls:
  a      Plan.stft alone
  b      Plan.stft, then torch re*re + im*im              (the per-bin baseline)
  b_mel  ... then @ W.T with the mel-80 HTK weights        (the band baseline)
  c      Features.spectrogram, one value per bin
  d      Features.spectrogram, mel-80 HTK
Before timing, at the timed size: c equals b bit for bit, and d lies within the
band bound of tests/test_gpu_features.py ((width + 2) 2^-24 sum |w||v|) of the
float64 sum over b's values.  Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
SHAPES = [(1024, 256), (1024, 300), (4096, 1024)]
N_MELS = 80


def time_leg(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def run_shape(pkg, torch, np, n, h, S, T, rounds, calls, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC0FFEE ^ n ^ (h << 16))
    x = torch.randn((S, T), generator=g, device=dev, dtype=torch.float32) * 0.25
    plan = pkg.Plan(frame_size=n, hop_size=h)
    F, bins = plan.frame_count(T), n // 2 + 1
    W = pkg.mel_filterbank(N_MELS, n, 16000.0)
    Wt = torch.from_numpy(W).to(dev).t().contiguous()
    f_bin, f_mel = pkg.Features(plan), pkg.Features(plan, weights=W)
    spec = torch.empty((S, F, bins), dtype=torch.complex64, device=dev)
    out_c = torch.empty((S, F, bins), dtype=torch.float32, device=dev)
    out_d = torch.empty((S, F, N_MELS), dtype=torch.float32, device=dev)

    def leg_a():
        plan.stft(x, spec)

    def power():
        plan.stft(x, spec)
        re, im = spec.real, spec.imag
        return re * re + im * im

    def leg_b():
        power()

    def leg_b_mel():
        return power() @ Wt

    def leg_c():
        f_bin.spectrogram(x, out_c)

    def leg_d():
        f_mel.spectrogram(x, out_d)

    legs = {"a": leg_a, "b": leg_b, "b_mel": leg_b_mel, "c": leg_c, "d": leg_d}
    kernels = {}
    for name in ("a", "c", "d"):
        legs[name]()
        kernels[name] = plan.last_launch()["kernels"]

    # ---- correctness at the timed size
    ref = power()
    leg_c()
    same = bool(torch.equal(out_c.view(torch.int32), ref.view(torch.int32)))
    leg_d()
    lo, hi = pkg.filterbank_spans(W)
    width = torch.from_numpy((hi - lo + 2).astype(np.float64)).to(dev)
    W64, Wabs = Wt.double(), Wt.double().abs()
    worst = 0.0
    step = max(1, (1 << 27) // (F * bins))  # streams per float64 block
    for s0 in range(0, S, step):
        v = ref[s0:s0 + step].double()
        bound = (v.abs() @ Wabs) * width * 2.0 ** -24
        err = (out_d[s0:s0 + step].double() - v @ W64).abs()
        ratio = err / bound.clamp_min(1e-300)
        worst = max(worst, float(ratio.max()))
    del ref
    if not same or not worst <= 1.0:
        raise SystemExit(f"{n}/{h}: per-bin equal to the baseline: {same}; worst band error / bound: {worst}")

    # ---- timing
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(time_leg(torch, fn, calls))
    samples = S * T
    bin_b, mel_b = 4.0 * bins / h, 4.0 * N_MELS / h
    alg = {"a": 4 + 2 * bin_b, "b": 4 + 2 * bin_b + 2 * bin_b + bin_b,
           "b_mel": 4 + 2 * bin_b + 2 * bin_b + bin_b + bin_b + mel_b, "c": 4 + bin_b, "d": 4 + mel_b}
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms_per_call": round(med, 4), "msamples_per_s": round(samples / med / 1e3, 1),
                     "spread": round((max(v) - min(v)) / med, 4), "alg_bytes_per_sample": round(alg[name], 3),
                     "hbm_share": round(alg[name] * samples / (med * 1e-3) / HBM_BYTES_PER_S, 4),
                     "calls": rounds * calls}
    res["speedup_c_over_b"] = round(res["b"]["ms_per_call"] / res["c"]["ms_per_call"], 3)
    res["speedup_d_over_b_mel"] = round(res["b_mel"]["ms_per_call"] / res["d"]["ms_per_call"], 3)
    res["d_over_a_time"] = round(res["d"]["ms_per_call"] / res["a"]["ms_per_call"], 3)
    res["check"] = {"c_bit_equal_b": same, "d_worst_error_over_bound": round(worst, 4)}
    res["kernels"] = kernels
    res["frames"] = F
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=480_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4, help="calls per leg and round (rounds x calls >= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=None, help="comma-separated N/H subset of the three shapes (profiling passes)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    out = {"suite": "features", "streams": a.streams, "samples": a.samples, "n_mels": N_MELS,
           "build": {k: v for k, v in pkg.build_info().items() if k != "path"},
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    want = None if a.shapes is None else set(a.shapes.split(","))
    for n, h in SHAPES:
        if want is not None and f"{n}/{h}" not in want:
            continue
        out["shapes"][f"{n}/{h}"] = run_shape(pkg, torch, np, n, h, a.streams, a.samples, a.rounds, a.calls,
                                              a.warmup)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
