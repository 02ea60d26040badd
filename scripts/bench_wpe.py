#!/usr/bin/env python3
"""The dereverberator's accumulate and filter kernels against a device copy, and the
per-hop entry's latency.

One process.
Kernels: Dereverberator.accumulate (k_wpe_acc) and Dereverberator.filter (k_wpe_filter) over
1876 frames of N = 1024 spectra at M = 4, K = 10 (L = 40), G = 1 and 64 groups, device time
on events, over the bytes each must move (both: the M rows of every frame read once, 8 M
per bin and frame; accumulate: 4 per bin and frame of inverse power, and the state written,
4 (L L + 2 L M) per bin; filter: 8 M per bin and frame written and the taps read, 8 L M per
bin): bytes/s and its ratio to a device-to-device copy moving the same number of bytes.
What the kernels actually load is more (every tile's wave reads its eight rows; every
microphone's wave reads all L stacked rows): the ratio says how much of that the caches
absorb.  A combination whose spectra exceed --max-gib is skipped and listed.
Per hop: Dereverberator.hop (stft_hop -> k_wpe_gain -> k_wpe_update -> istft_hop, four
launches) at 512/128, M = 2, 4, 8 with K = 10, 10, 8, one group: wall time of a hop with a
stream synchronise, --hops hops per round after a warm-up; the median over the rounds of
the round's p50 and p99, and the spread of the p50s.
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


def timed(torch, fn, n):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(n):
        fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) / n * 1e-3


def copy_rate(torch, moved, rounds, n=5):
    dev = torch.device("cuda:0")
    src = torch.empty(max(moved // 8, 1), dtype=torch.float32, device=dev)  # a copy moves 2 x its size
    dst = torch.empty_like(src)
    dst.copy_(src)
    c_s = statistics.median(timed(torch, lambda: dst.copy_(src), n) for _ in range(rounds))
    return src.numel() * 8 / c_s


def run_kernels(pkg, torch, M, K, G, F, rounds):
    dev = torch.device("cuda:0")
    N, H = 1024, 256
    plan = pkg.Plan(frame_size=N, hop_size=H)
    bins, L = N // 2 + 1, M * K
    X = torch.view_as_complex(torch.randn((G, M, F, bins, 2), device=dev, dtype=torch.float32))
    d = pkg.Dereverberator(plan, M, taps=K, delay=3, groups=1)
    io = d.power(X)
    taps = torch.view_as_complex(0.01 * torch.randn((G, L, M, bins, 2), device=dev, dtype=torch.float32))
    out = torch.empty((G, M, F, bins), device=dev, dtype=torch.complex64)
    state = torch.empty((G, L * L + 2 * L * M, bins), device=dev, dtype=torch.float32)
    res, n = {}, 3
    for name, fn, moved in (
            ("accumulate", lambda: d.accumulate(X, io, state_out=state), G * bins * (F * (8 * M + 4) + 4 * (L * L + 2 * L * M))),
            ("filter", lambda: d.filter(X, taps, out=out), G * bins * (F * 16 * M + 8 * L * M))):
        fn()
        torch.cuda.synchronize()
        t = statistics.median(timed(torch, fn, n) for _ in range(rounds))
        rate, copy = moved / t, copy_rate(torch, moved, rounds)
        res[name] = {"seconds": t, "bytes": moved, "bytes_per_s": rate, "copy_bytes_per_s": copy, "of_copy": rate / copy,
                     "launch": d.last_launch()}
    d.close()
    return res


def run_hop(pkg, torch, M, K, hops, rounds, warm):
    dev = torch.device("cuda:0")
    N, H = 512, 128
    plan = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True, boundary_mode=pkg.DROP)
    d = pkg.Dereverberator(plan, M, taps=K, delay=3, alpha=0.999)
    s_in, s_out = pkg.Stream(plan, M), pkg.Stream(plan, M)
    x = torch.randn((M, H * (warm + hops * rounds)), device=dev)
    out = torch.empty((M, H), device=dev)
    q = 0
    for _ in range(warm):
        d.hop(s_in, s_out, x[:, q * H:(q + 1) * H].contiguous(), out)
        q += 1
    torch.cuda.synchronize()
    p50, p99 = [], []
    for _ in range(rounds):
        ts = []
        for _ in range(hops):
            hop = x[:, q * H:(q + 1) * H].contiguous()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.hop(s_in, s_out, hop, out)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            q += 1
        p50.append(pct(ts, 0.5)), p99.append(pct(ts, 0.99))
    rec = d.last_launch()
    for o in (d, s_in, s_out):
        o.close()
    return {"p50_s": statistics.median(p50), "p99_s": statistics.median(p99), "p50_spread_s": max(p50) - min(p50),
            "launch": rec}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1876)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--max-gib", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpe_suite.json"))
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    res = {"bench": "wpe_suite", "build": build_check(pkg), "device": torch.cuda.get_device_name(0), "kernels": {},
           "hop": {}, "skipped": []}
    M, K = 4, 10
    for G in (1, 64):
        gib = 2 * G * M * a.frames * 513 * 8 / 2 ** 30
        if gib > a.max_gib:
            res["skipped"].append({"G": G, "gib": gib})
            continue
        res["kernels"][f"M{M}_K{K}_G{G}"] = run_kernels(pkg, torch, M, K, G, a.frames, a.rounds)
    for M, K in ((2, 10), (4, 10), (8, 8)):
        res["hop"][f"M{M}_K{K}"] = run_hop(pkg, torch, M, K, a.hops, a.rounds, a.warmup)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
