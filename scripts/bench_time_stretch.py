#!/usr/bin/env python3
"""Measure the phase vocoder and the time stretch against the same recurrence in torch.

Shapes at 1024/256: --streams x --samples (the batched case) and one stream of
--long-samples (the chunked route), rates 0.8 and 1.25.  Legs, timed in one
process, alternating, each with its own warm-up and device events around its calls:
  a   the recurrence as torch ops on Plan.stft's output (angle, abs, two gathers,
      wrap, cumsum, polar)
  b   Plan.phase_vocoder on the same spectra
  c   Plan.stft + a + Plan.istft_ola
  d   Plan.time_stretch
Before timing, at the timed size: |b| equals |a| within float32 rounding, and d
equals istft_ola(b(stft(x))) bit for bit.  b's traffic is set against the
algorithmic 8 bins S (F_visited + F') bytes and 8 TB/s.  Prints one JSON line (and
writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
N, H = 1024, 256
RATES = (0.8, 1.25)


def time_leg(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def run_case(pkg, torch, np, S, T, rate, rounds, calls, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC0FFEE ^ S ^ int(rate * 1000))
    x = torch.randn((S, T), generator=g, device=dev, dtype=torch.float32) * 0.25
    plan = pkg.Plan(frame_size=N, hop_size=H)
    F, bins = plan.frame_count(T), N // 2 + 1
    Fp = pkg.stretch_frame_count(F, rate)
    tau = np.arange(Fp, dtype=np.float64) * rate
    i_np = np.floor(tau).astype(np.int64)
    idx0 = torch.from_numpy(i_np).to(dev)
    idx1 = idx0 + 1
    alpha = torch.from_numpy((tau - i_np).astype(np.float32)).to(dev)[None, :, None]
    adv = torch.linspace(0, math.pi * H, bins, device=dev)[None, None, :]
    visited = np.union1d(i_np, i_np + 1)
    F_visited = int((visited < F).sum())
    spec = plan.stft(x)
    out_b = torch.empty((S, Fp, bins), dtype=torch.complex64, device=dev)
    y_d = torch.empty((S, Fp * H), dtype=torch.float32, device=dev)

    def torch_vocoder(sp):
        zero = torch.zeros((S, 1, bins), dtype=torch.float32, device=dev)
        ang = torch.cat([torch.angle(sp), zero], 1)
        mag = torch.cat([sp.abs(), zero], 1)
        a0, a1 = ang.index_select(1, idx0), ang.index_select(1, idx1)
        m0, m1 = mag.index_select(1, idx0), mag.index_select(1, idx1)
        ph = a1 - a0 - adv
        ph = ph - 2 * math.pi * torch.round(ph / (2 * math.pi))
        ph = ph + adv
        ph = torch.cat([ang[:, :1], ph[:, :-1]], 1)
        return torch.polar(alpha * m1 + (1 - alpha) * m0, torch.cumsum(ph, 1))

    def leg_a():
        return torch_vocoder(spec)

    def leg_b():
        plan.phase_vocoder(spec, rate, out_b)

    def leg_c():
        return plan.istft_ola(torch_vocoder(plan.stft(x)))

    def leg_d():
        plan.time_stretch(x, rate, y_d)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}

    # ---- correctness at the timed size
    ref = leg_a()
    leg_b()
    rec_b = plan.last_launch()
    mag_err = float((out_b.abs() - ref.abs()).abs().max() / ref.abs().max())
    del ref
    want = plan.istft_ola(out_b)
    leg_d()
    rec_d = plan.last_launch()
    same = bool(torch.equal(y_d.view(torch.int32), want.view(torch.int32)))
    del want
    if not same or not mag_err <= 1e-5:
        raise SystemExit(f"S={S} rate={rate}: d equals the composition: {same}; |b| vs |a|: {mag_err}")

    # ---- timing
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(time_leg(torch, fn, calls))
    alg_b = 8.0 * bins * S * (F_visited + Fp)
    # the chunked route reads every row but the last chunk's once more (the increment sums)
    nc = max(1, rec_b["n_chunks"])
    moved_b = alg_b + (8.0 * bins * S * F_visited * (nc - 1) / nc if nc > 1 else 0.0)
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms_per_call": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                     "calls": rounds * calls}
    tb = res["b"]["ms_per_call"] * 1e-3
    res["b"].update({"alg_bytes": alg_b, "moved_bytes": moved_b,
                     "alg_hbm_share": round(alg_b / tb / HBM_BYTES_PER_S, 4),
                     "moved_hbm_share": round(moved_b / tb / HBM_BYTES_PER_S, 4),
                     "kernels": rec_b["kernels"], "n_chunks": rec_b["n_chunks"], "grid": rec_b["grid"]})
    res["d"].update({"kernels_last_slice": rec_d["kernels"]})
    res["speedup_b_over_a"] = round(res["a"]["ms_per_call"] / res["b"]["ms_per_call"], 3)
    res["speedup_d_over_c"] = round(res["c"]["ms_per_call"] / res["d"]["ms_per_call"], 3)
    res["check"] = {"d_bit_equal_composition": same, "b_vs_a_magnitude_error": mag_err}
    res["frames"] = {"F": F, "F_out": Fp, "F_visited": F_visited}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--samples", type=int, default=480_000)
    ap.add_argument("--long-samples", type=int, default=30_720_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4, help="calls per leg and round (rounds x calls >= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    out = {"suite": "time_stretch", "frame": f"{N}/{H}",
           "build": {k: v for k, v in pkg.build_info().items() if k != "path"},
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for S, T in ((a.streams, a.samples), (1, a.long_samples)):
        for rate in RATES:
            out["cases"][f"S={S} T={T} rate={rate}"] = run_case(pkg, torch, np, S, T, rate, a.rounds, a.calls,
                                                               a.warmup)
            torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
