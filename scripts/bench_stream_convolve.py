#!/usr/bin/env python3
"""Per-hop latency of StreamConvolver.push against the plain hop and against what a
caller can compose without it.

One process.  A hop is timed on the host clock around the call(s) and a stream
synchronise; each leg has its own objects and runs --hops hops per round after its
warm-up, the legs alternating round by round.  Per leg: the median over the rounds of
the round's p50 and p99, and the spread of the p50s over the rounds.
  a  Stream.push_hop on a plain N = 2B / H = B plan: the hop path with no convolution
  b  the composition: Plan.rfft of the zero-padded block -> a torch ring of P spectra,
     a complex multiply and sum against Convolver.spectra() -> Stream.istft_hop on
     the convolver's plan
  c  StreamConvolver route 2, manual prefetch: push + synchronise is timed; the
     prefetch (+ synchronise) after it is timed apart ("c_prefetch")
  d  route 2, automatic prefetch
  e  route 1 (one launch, the whole chain in the head)
Shapes: B in {128, 256, 512}, K in {B, 4800, 48000}, 2 and 64 channels.
Route sweep: the same legs at K = P B for P in {2, 3, 4, 6}, reported as d against e
("route_sweep"): the evidence for the library's choice between the routes at small P.
Before timing: c, d and e give the same blocks as each other and as
Convolver.convolve with frame pairing off, bit for bit.
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

BLOCKS = (128, 256, 512)
CHANNELS = (2, 64)
SWEEP_P = (2, 3, 4, 6)


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def build_check(pkg) -> dict:
    """The loaded library's baked-in source hash against the tree's (tools/src_hash.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import src_hash as SH
    info = pkg.build_info()
    tree = SH.lib_hash()
    if info["src"] != tree:
        raise SystemExit(f"stale library: built from {info['src']}, the tree is {tree}")
    return {"lib_src_hash": info["src"], "tree_src_hash": tree, "arch": info["arch"], "match": True}


def same_bits(torch, a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def run_shape(pkg, torch, np, B, K, C, rounds, hops, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5C0 ^ B ^ (K << 8) ^ (C << 24))
    ring_in = [(torch.randn((C, B), generator=g, device=dev, dtype=torch.float32) * 0.25).contiguous()
               for _ in range(64)]
    rng = np.random.default_rng(K + B)
    taps = (rng.standard_normal((2, K)) * np.exp(-4.0 * np.arange(K) / K)[None] / np.sqrt(K / 8.0 + 1.0)).astype(np.float32)
    conv = pkg.Convolver(taps, block=B)
    P, bins = conv.partitions, B + 1
    plain = pkg.Plan(frame_size=2 * B, hop_size=B)
    out = torch.zeros((C, B), dtype=torch.float32, device=dev)
    cur = torch.cuda.current_stream()

    # ---- the three routes against the offline convolver, bit for bit
    n_check = min(2 * P + 3, P + 8)
    x = torch.cat([ring_in[j % 64] for j in range(n_check)], dim=1)
    conv.plan.set_frame_pairing(False)
    try:
        want = conv.convolve(x)[:, :n_check * B]
        torch.cuda.synchronize()
    finally:
        conv.plan.set_frame_pairing(True)
    modes = {"c": (2, False), "d": (2, True), "e": (1, True)}
    sconv, routes = {}, {}
    for name, (route, auto) in modes.items():
        sc = pkg.StreamConvolver(conv, C)
        sc.set_route(route)
        sc.set_prefetch(auto)
        blocks = []
        for j in range(n_check):
            blocks.append(sc.push(ring_in[j % 64]))
            if name == "c":
                sc.prefetch()
        torch.cuda.synchronize()
        if not same_bits(torch, torch.cat(blocks, dim=1), want):
            raise SystemExit(f"B={B} K={K} C={C}: leg {name} differs from Convolver.convolve")
        routes[name] = sc.last_launch()["route"]
        sc.reset()
        sc.set_route(route)
        sconv[name] = sc

    # ---- the composition a caller can write without the streaming convolver
    Hc = torch.from_numpy(conv.spectra()).to(dev)[torch.arange(C, device=dev) % 2].contiguous()   # (C, P, bins)
    b_ring = torch.zeros((C, P, bins), dtype=torch.complex64, device=dev)
    b_frame = torch.zeros((C, 2 * B), dtype=torch.float32, device=dev)
    b_stream = pkg.Stream(conv.plan, C)
    a_stream = pkg.Stream(plain, C)
    ar = torch.arange(P, device=dev)
    count = {k: 0 for k in "abcde"}

    def leg_a(hop):
        a_stream.push_hop(hop, out)

    def leg_b(hop):
        k = count["b"]
        b_frame[:, :B] = hop
        b_ring[:, k % P] = conv.plan.rfft(b_frame)
        y = (b_ring[:, (k - ar) % P] * Hc).sum(dim=1)
        b_stream.istft_hop(y, out=out)

    def leg_s(name):
        return lambda hop: sconv[name].push(hop, out)

    legs = {"a": leg_a, "b": leg_b, "c": leg_s("c"), "d": leg_s("d"), "e": leg_s("e")}
    pre_us = []

    def one(name, record=True):
        hop = ring_in[count[name] % 64]
        t0 = time.perf_counter_ns()
        legs[name](hop)
        cur.synchronize()
        us = (time.perf_counter_ns() - t0) * 1e-3
        count[name] += 1
        if name == "c":   # the manual prefetch, off the timed hop
            t0 = time.perf_counter_ns()
            sconv["c"].prefetch()
            cur.synchronize()
            if record:
                pre_us.append((time.perf_counter_ns() - t0) * 1e-3)
        return us

    for name in legs:
        for _ in range(warmup):
            one(name, record=False)
    p50 = {k: [] for k in legs}
    p99 = {k: [] for k in legs}
    pre50 = []
    for _ in range(rounds):
        for name in legs:
            del pre_us[:]
            us = [one(name) for _ in range(hops)]
            p50[name].append(pct(us, 0.50))
            p99[name].append(pct(us, 0.99))
            if name == "c":
                pre50.append(pct(pre_us, 0.50))
    res = {"P": P, "routes": routes}
    for name in legs:
        med = statistics.median(p50[name])
        res[name] = {"p50_us": round(med, 2), "p99_us": round(statistics.median(p99[name]), 2),
                     "spread": round((max(p50[name]) - min(p50[name])) / med, 4), "hops": rounds * hops}
    res["c_prefetch"] = {"p50_us": round(statistics.median(pre50), 2),
                         "spread": round((max(pre50) - min(pre50)) / statistics.median(pre50), 4)}
    a, b, c, d, e = (res[k]["p50_us"] for k in "abcde")
    res["c_over_a"] = round(c / a, 3)
    res["b_over_c"] = round(b / c, 3)
    res["e_over_d"] = round(e / d, 3)
    res["check"] = {"c_d_e_bit_equal_offline": True, "blocks": n_check}
    for sc in sconv.values():
        sc.close()
    a_stream.close()
    b_stream.close()
    conv.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hops", type=int, default=300, help="timed hops per leg and round")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    out = {"suite": "stream_convolve", "rounds": a.rounds, "hops_per_round": a.hops, "build": build_check(pkg),
           "device": torch.cuda.get_device_name(0), "shapes": {}, "c_p50_us_against_P": {}, "route_sweep": {}}
    for B in BLOCKS:
        for C in CHANNELS:
            for K in (B, 4800, 48000):
                r = run_shape(pkg, torch, np, B, K, C, a.rounds, a.hops, a.warmup)
                out["shapes"][f"B={B} K={K} C={C}"] = r
                out["c_p50_us_against_P"].setdefault(f"B={B} C={C}", []).append([r["P"], r["c"]["p50_us"]])
    for B in BLOCKS:
        for C in CHANNELS:
            for P in SWEEP_P:
                r = run_shape(pkg, torch, np, B, P * B, C, a.rounds, a.hops, a.warmup)
                out["route_sweep"][f"B={B} P={P} C={C}"] = {"c": r["c"], "d": r["d"], "e": r["e"],
                                                           "c_prefetch": r["c_prefetch"], "e_over_d": r["e_over_d"]}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
