#!/usr/bin/env python3
"""Per-hop latency of Stream.features_hop against what a caller does without it.

One process.  A hop is timed on the host clock around the call(s) and a stream
synchronise; each leg has its own Stream object and runs --hops hops per round
after its warm-up, the legs alternating round by round.  Per leg: the median over
the rounds of the round's p50 and p99, and the spread of the p50s over the rounds.
  a  stft_hop
  b  stft_hop, then torch: log10(clamp((spec.abs() ** 2) @ W.T, floor))   (5 more launches)
  c  features_hop, mel-80 HTK in dB, no spectrum
  d  the same with the spectrum row
  e  features_hop, one value per bin (|X|^2)
Shapes: 512/128 at 2 and at 64 channels, 1024/256 and 960/240 at 2 channels.
Before timing: e equals re*re + im*im of a's spectrum bit for bit, and c lies
within 1e-3 dB of torch's float64 value of the same hop where that is finite.
Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(512, 128, 2), (512, 128, 64), (1024, 256, 2), (960, 240, 2)]
N_MELS = 80
FLOOR = 1e-10
B_EXTRA_LAUNCHES = 5  # abs, pow, matmul, clamp, log10


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def run_shape(pkg, torch, n, h, C, rounds, hops, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xFEA7 ^ n ^ (h << 16) ^ (C << 8))
    ring = [(torch.randn((C, h), generator=g, device=dev, dtype=torch.float32) * 0.25).contiguous() for _ in range(64)]
    plan = pkg.Plan(frame_size=n, hop_size=h)
    bins = n // 2 + 1
    W = pkg.mel_filterbank(N_MELS, n, 16000.0)
    Wt = torch.from_numpy(W).to(dev).t().contiguous()
    f_db = pkg.Features(plan, weights=W, log=pkg.FEAT_DB, floor=FLOOR)
    f_bin = pkg.Features(plan)
    spec = torch.zeros((C, bins), dtype=torch.complex64, device=dev)
    out_mel = torch.zeros((C, N_MELS), dtype=torch.float32, device=dev)
    out_bin = torch.zeros((C, bins), dtype=torch.float32, device=dev)
    cur = torch.cuda.current_stream()

    def leg_a(st, hop):
        st.stft_hop(hop, spec)

    def leg_b(st, hop):
        st.stft_hop(hop, spec)
        return torch.log10(torch.clamp((spec.abs() ** 2) @ Wt, min=FLOOR))

    def leg_c(st, hop):
        st.features_hop(f_db, hop, out=out_mel)

    def leg_d(st, hop):
        st.features_hop(f_db, hop, out=out_mel, spec=spec)

    def leg_e(st, hop):
        st.features_hop(f_bin, hop, out=out_bin)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d, "e": leg_e}
    objs = {k: pkg.Stream(plan, C) for k in legs}

    # ---- correctness at the timed size (hops 0 .. N/H: the last completes a frame)
    for q in range(-(-n // h) + 1):
        leg_a(objs["a"], ring[q])
        leg_c(objs["c"], ring[q])
        leg_e(objs["e"], ring[q])
    re, im = spec.real, spec.imag
    same = bool(torch.equal((re * re + im * im).view(torch.int32), out_bin.view(torch.int32)))
    ref = 10.0 * torch.log10(torch.clamp(((re.double() ** 2 + im.double() ** 2) @ Wt.double()), min=FLOOR))
    worst_db = float((out_mel.double() - ref).abs().max())
    if not same or not worst_db <= 1e-3:
        raise SystemExit(f"{n}/{h} C={C}: per-bin equal to the spectrum's power: {same}; worst dB error: {worst_db}")
    for st in objs.values():
        st.reset()

    # ---- timing
    q = {k: 0 for k in legs}

    def one(name):
        hop = ring[q[name] % len(ring)]
        q[name] += 1
        t0 = time.perf_counter_ns()
        legs[name](objs[name], hop)
        cur.synchronize()
        return (time.perf_counter_ns() - t0) * 1e-3

    for name in legs:
        for _ in range(warmup):
            one(name)
    p50 = {k: [] for k in legs}
    p99 = {k: [] for k in legs}
    for _ in range(rounds):
        for name in legs:
            us = [one(name) for _ in range(hops)]
            p50[name].append(pct(us, 0.50))
            p99[name].append(pct(us, 0.99))
    res = {}
    for name in legs:
        med = statistics.median(p50[name])
        res[name] = {"p50_us": round(med, 2), "p99_us": round(statistics.median(p99[name]), 2),
                     "spread": round((max(p50[name]) - min(p50[name])) / med, 4), "hops": rounds * hops}
    a, b, c, d = (res[k]["p50_us"] for k in "abcd")
    res["c_minus_a_us"] = round(c - a, 2)
    res["d_minus_c_us"] = round(d - c, 2)
    res["one_launch_us"] = round((b - a) / B_EXTRA_LAUNCHES, 2)
    res["c_below_b"] = bool(c < b)
    res["check"] = {"e_bit_equal_power": same, "c_worst_db_error": round(worst_db, 7)}
    for st in objs.values():
        st.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hops", type=int, default=600, help="timed hops per leg and round")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    out = {"suite": "stream_features", "n_mels": N_MELS, "rounds": a.rounds, "hops_per_round": a.hops,
           "b_extra_launches": B_EXTRA_LAUNCHES,
           "build": {k: v for k, v in pkg.build_info().items() if k != "path"},
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for n, h, C in SHAPES:
        out["shapes"][f"{n}/{h} C={C}"] = run_shape(pkg, torch, n, h, C, a.rounds, a.hops, a.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
