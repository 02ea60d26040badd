#!/usr/bin/env python3
"""Measure the resampler and the pitch shift against the same filter in torch.

Cases: 44.1 -> 48 kHz (160/147), 48 -> 16 kHz (1/3), x2, /2 and one semitone
(89/84), each at --streams x --samples and at one stream of --long-samples, at
zeros 6 and 16.  Legs, timed in one process, alternating, each with its own
warm-up and device events around its calls:
  a   the library's table as a torch conv1d with stride D over the padded signal
      (torchaudio.functional.resample's formulation: U output channels, one per
      phase, interleaved afterwards)
  b   Resampler.resample
  c   Plan.time_stretch (1024/256) + a on its output, fixed to T samples
  d   Plan.pitch_shift
Before timing, at the timed size: b equals a within float32 rounding of a K-tap
sum, and d equals resample(time_stretch(x)) bit for bit.  b's time is set against
the algorithmic traffic 4 S (T + L) bytes and 8 TB/s.  Prints one JSON line and
writes it to --out after every case (--append keeps the cases already there).
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
N, H = 1024, 256
CASES = {"44k1_to_48k": (160, 147), "48k_to_16k": (1, 3), "x2": (2, 1), "div2": (1, 2), "semitone": (89, 84)}


def time_leg(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def conv_resampler(torch, r, T):
    """Leg a for inputs of T samples: y[q U + p] = sum_i h[(p D) mod U][i] x[q D + (p D) div U - W + 1 + i]
    as one strided convolution with U output channels."""
    U, D, W, K = r.up, r.down, r.half_width, r.taps
    L = r.output_length(T)
    tab = torch.from_numpy(r.table())
    Kc = K + D - 1
    kern = torch.zeros((U, 1, Kc))
    for p in range(U):
        off = (p * D) // U
        kern[p, 0, off:off + K] = tab[(p * D) % U]
    kern = kern.cuda()
    Q = -(-L // U)
    right = max(0, (Q - 1) * D + Kc - (W - 1) - T)

    def run(x):
        xp = torch.nn.functional.pad(x, (W - 1, right))[:, None]
        y = torch.nn.functional.conv1d(xp, kern, stride=D)
        return y.transpose(1, 2).reshape(x.shape[0], -1)[:, :L]

    return run, L


def run_case(pkg, torch, S, T, up, down, zeros, rounds, calls, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC0FFEE ^ S ^ (up * 4099 + down))
    x = torch.randn((S, T), generator=g, device=dev, dtype=torch.float32) * 0.25
    r = pkg.Resampler(up, down, zeros=zeros)
    plan = pkg.Plan(frame_size=N, hop_size=H)
    conv_x, L = conv_resampler(torch, r, T)
    Ls = plan.stretch_output_length(T, r.up / r.down)
    conv_z, Lz = conv_resampler(torch, r, Ls)
    y_b = torch.empty((S, L), dtype=torch.float32, device=dev)
    y_d = torch.empty((S, T), dtype=torch.float32, device=dev)

    def fix(w):
        if w.shape[1] >= T:
            return w[:, :T]
        return torch.nn.functional.pad(w, (0, T - w.shape[1]))

    def leg_a():
        return conv_x(x)

    def leg_b():
        r.resample(x, y_b)

    def leg_c():
        return fix(conv_z(plan.time_stretch(x, r.up / r.down))).contiguous()

    def leg_d():
        plan.pitch_shift(x, r, y=y_d)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}

    # ---- correctness at the timed size
    ref = leg_a()
    leg_b()
    rec_b = r.last_launch()
    err = float((y_b - ref).abs().max() / ref.abs().max())
    del ref
    want = fix(r.resample(plan.time_stretch(x, r.up / r.down))).contiguous()
    leg_d()
    rec_d = plan.last_launch()
    same = bool(torch.equal(y_d.view(torch.int32), want.view(torch.int32)))
    del want
    if not same or not err <= 1e-5:
        raise SystemExit(f"S={S} {up}/{down} zeros={zeros}: d equals the composition: {same}; b vs a: {err}")

    # ---- timing
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(time_leg(torch, fn, calls))
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        res[name] = {"ms_per_call": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                     "calls": rounds * calls}
    alg = 4.0 * S * (T + L)
    tb = res["b"]["ms_per_call"] * 1e-3
    res["b"].update({"alg_bytes": alg, "alg_hbm_share": round(alg / tb / HBM_BYTES_PER_S, 4),
                     "outputs_per_us": round(S * L / tb * 1e-6, 1), "launch": rec_b})
    res["d"].update({"kernels_last_slice": rec_d["kernels"]})
    res["speedup_b_over_a"] = round(res["a"]["ms_per_call"] / res["b"]["ms_per_call"], 3)
    res["speedup_d_over_c"] = round(res["c"]["ms_per_call"] / res["d"]["ms_per_call"], 3)
    res["check"] = {"d_bit_equal_composition": same, "b_vs_a_relative_error": err}
    res["shape"] = {"U": r.up, "D": r.down, "K": r.taps, "T": T, "L": L, "stretched": Ls, "zeros": zeros}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--samples", type=int, default=480_000)
    ap.add_argument("--long-samples", type=int, default=30_720_000)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    ap.add_argument("--zeros", default="6,16")
    ap.add_argument("--sizes", default="batch,long", help="batch (--streams x --samples), long (1 x --long-samples)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4, help="calls per leg and round (rounds x calls >= 20)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the cases --out already holds")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    out = {"suite": "resample", "pitch_shift_frame": f"{N}/{H}",
           "build": {k: v for k, v in pkg.build_info().items() if k != "path"},
           "device": torch.cuda.get_device_name(0), "cases": {}}
    if a.append and a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            out["cases"] = json.load(fh).get("cases", {})
    sizes = {"batch": (a.streams, a.samples), "long": (1, a.long_samples)}
    for size in a.sizes.split(","):
        S, T = sizes[size]
        for name in a.cases.split(","):
            up, down = CASES[name]
            for zeros in (int(z) for z in a.zeros.split(",")):
                key = f"{name} S={S} T={T} zeros={zeros}"
                out["cases"][key] = run_case(pkg, torch, S, T, up, down, zeros, a.rounds, a.calls, a.warmup)
                print(key, json.dumps(out["cases"][key]), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
                if a.out:
                    with open(a.out, "w") as fh:
                        fh.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
