#!/usr/bin/env python3
"""Per-hop latency of AdaptiveFilter.push against the plain hop and against a torch
composition of the same algorithm.

One process.  A hop is timed on the host clock around the call(s) and a stream
synchronise; each leg has its own objects and runs --hops hops per round after its
warm-up, the legs alternating round by round.  Per leg: the median over the rounds of
the round's p50 and p99, and the spread of the p50s over the rounds.
  a   Stream.push_hop on a plain N = 2B / H = B plan: the hop path with no filter
  f   the frozen filter (adaptation off): one launch
  m0  adapting, no constraint: hop + update
  m1  adapting, round-robin constraint (the default): hop + update + constrain(k mod P)
  m2  adapting, every partition constrained every hop
  t   the same algorithm (mode 1) composed from torch.fft and tensor arithmetic
Shapes: B in {128, 256, 512}, K in {B, 4800, 48000}, 2 and 64 channels.
Before timing: m1 equals m0 hops followed by explicit constrain(k mod P) calls, bit for
bit, and the torch composition's e agrees with m1's to 1e-3 rel-L2 over the check hops.
Update kernel: per shape, the device time of a batch of m0 hops minus that of a batch of
frozen hops (events, no synchronise inside a batch), over the 3 P (B+1) 8 bytes per
channel the update moves: bytes/s, and its ratio to a device-to-device copy moving the
same number of bytes (the difference also holds the hop's second transform, so the
figure is a lower bound).
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
LEGS = ("a", "f", "m0", "m1", "m2", "t")


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


class TorchFdaf:
    """Steps 1 - 8 of the contract (mode 1) on torch.fft, complex64."""

    def __init__(self, torch, B, K, C, mu, lam, delta, dev):
        self.torch, self.B, self.P, self.C = torch, B, -(-K // B), C
        self.mu_p, self.lam, self.delta = mu / self.P, lam, delta
        P, bins = self.P, B + 1
        self.ring = torch.zeros((C, P, bins), dtype=torch.complex64, device=dev)
        self.W = torch.zeros((C, P, bins), dtype=torch.complex64, device=dev)
        self.pw = torch.zeros((C, bins), dtype=torch.float32, device=dev)
        self.frame = torch.zeros((C, 2 * B), dtype=torch.float32, device=dev)
        self.eframe = torch.zeros((C, 2 * B), dtype=torch.float32, device=dev)
        self.ar = torch.arange(P, device=dev)
        self.k = 0

    def push(self, x, d):
        torch, B, P, k = self.torch, self.B, self.P, self.k
        self.frame[:, :B] = self.frame[:, B:].clone()
        self.frame[:, B:] = x
        X = torch.fft.rfft(self.frame)
        self.ring[:, k % P] = X
        rows = self.ring[:, (k - self.ar) % P]           # row p pairs with W_p (zeros before hop 0)
        y = torch.fft.irfft((rows * self.W).sum(dim=1), n=2 * B)[:, B:]
        e = d - y
        self.eframe[:, B:] = e
        E = torch.fft.rfft(self.eframe)
        m = X.real * X.real + X.imag * X.imag
        self.pw = m if k == 0 else self.lam * self.pw + (1.0 - self.lam) * m
        G = (self.mu_p / (self.pw + self.delta)) * E
        self.W += rows.conj() * G[:, None]
        p = k % P
        w = torch.fft.irfft(self.W[:, p], n=2 * B)
        w[:, B:] = 0
        self.W[:, p] = torch.fft.rfft(w)
        self.k += 1
        return e


def run_shape(pkg, torch, np, B, K, C, rounds, hops, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xFDA ^ B ^ (K << 8) ^ (C << 24))
    xs = [(torch.randn((C, B), generator=g, device=dev, dtype=torch.float32) * 0.25).contiguous() for _ in range(64)]
    ds = [(torch.randn((C, B), generator=g, device=dev, dtype=torch.float32) * 0.25).contiguous() for _ in range(64)]
    P = -(-K // B)
    plain = pkg.Plan(frame_size=2 * B, hop_size=B)
    out = torch.zeros((C, B), dtype=torch.float32, device=dev)
    cur = torch.cuda.current_stream()
    mu, lam, delta = 0.5, 0.9, 1e-3

    def make(mode, adapt=True):
        af = pkg.AdaptiveFilter(B, K, C)
        af.set_step(mu, lam, delta)
        af.set_constraint(mode)
        af.set_adapt(adapt)
        af.prepare()
        return af

    # ---- mode 1 against mode 0 + explicit constraint (bits) and against the torch composition
    n_check = min(2 * P + 3, P + 8)
    a1, a0, tc = make(1), make(0), TorchFdaf(torch, B, K, C, mu, lam, delta, dev)
    num = den = 0.0
    for j in range(n_check):
        e1 = a1.push(xs[j % 64], ds[j % 64])
        e0 = a0.push(xs[j % 64], ds[j % 64])
        a0.constrain(j % P)
        et = tc.push(xs[j % 64], ds[j % 64])
        if not same_bits(torch, e1, e0):
            raise SystemExit(f"B={B} K={K} C={C}: mode 1 differs from mode 0 + constrain at hop {j}")
        num += float(((et - e1).double() ** 2).sum())
        den += float((e1.double() ** 2).sum())
    torch.cuda.synchronize()
    if not same_bits(torch, a1.state()["W"], a0.state()["W"]):
        raise SystemExit(f"B={B} K={K} C={C}: mode 1 weights differ from mode 0 + constrain")
    rel = (num / den) ** 0.5
    if not rel <= 1e-3:
        raise SystemExit(f"B={B} K={K} C={C}: the torch composition's e is {rel:.2e} rel-L2 from the library's")
    a1.close()
    a0.close()

    af = {"f": make(1, adapt=False), "m0": make(0), "m1": make(1), "m2": make(2)}
    tleg = TorchFdaf(torch, B, K, C, mu, lam, delta, dev)
    a_stream = pkg.Stream(plain, C)
    count = {k: 0 for k in LEGS}

    def leg(name):
        if name == "a":
            return lambda x, d: a_stream.push_hop(x, out)
        if name == "t":
            return lambda x, d: tleg.push(x, d)
        return lambda x, d: af[name].push(x, d, e=out)

    legs = {name: leg(name) for name in LEGS}

    def one(name):
        j = count[name] % 64
        t0 = time.perf_counter_ns()
        legs[name](xs[j], ds[j])
        cur.synchronize()
        count[name] += 1
        return (time.perf_counter_ns() - t0) * 1e-3

    for name in LEGS:
        for _ in range(warmup):
            one(name)
    p50 = {k: [] for k in LEGS}
    p99 = {k: [] for k in LEGS}
    for _ in range(rounds):
        for name in LEGS:
            us = [one(name) for _ in range(hops)]
            p50[name].append(pct(us, 0.50))
            p99[name].append(pct(us, 0.99))
    res = {"P": P}
    for name in LEGS:
        med = statistics.median(p50[name])
        res[name] = {"p50_us": round(med, 2), "p99_us": round(statistics.median(p99[name]), 2),
                     "spread": round((max(p50[name]) - min(p50[name])) / med, 4), "hops": rounds * hops}
    res["m1_over_a"] = round(res["m1"]["p50_us"] / res["a"]["p50_us"], 3)
    res["m1_over_f"] = round(res["m1"]["p50_us"] / res["f"]["p50_us"], 3)
    res["t_over_m1"] = round(res["t"]["p50_us"] / res["m1"]["p50_us"], 3)
    res["check"] = {"m1_bit_equal_m0_plus_constrain": True, "torch_rel_l2": float(f"{rel:.3e}"), "hops": n_check}

    # ---- the update kernel's traffic: batches of hops on device events
    def batch_ms(name, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for j in range(n):
            legs[name](xs[j % 64], ds[j % 64])
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    n = 100
    diffs = []
    for _ in range(rounds):
        diffs.append((batch_ms("m0", n) - batch_ms("f", n)) / n * 1e-3)   # seconds per hop
    per_hop = statistics.median(diffs)
    moved = 3 * P * (B + 1) * 8 * C
    buf = torch.empty(max(moved // 8, 1), dtype=torch.float32, device=dev)   # a copy moves 2 x its size
    dst = torch.empty_like(buf)
    copies = []
    for _ in range(rounds):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(20):
            dst.copy_(buf)
        ev1.record()
        ev1.synchronize()
        copies.append(ev0.elapsed_time(ev1) / 20 * 1e-3)
    copy_s = statistics.median(copies)
    res["update"] = {"bytes_per_hop": moved, "seconds_per_hop": float(f"{per_hop:.4e}"),
                     "bytes_per_s": float(f"{moved / per_hop:.4e}") if per_hop > 0 else None,
                     "copy_bytes_per_s": float(f"{buf.numel() * 8 / copy_s:.4e}"),
                     "fraction_of_copy": round(copy_s * moved / (per_hop * buf.numel() * 8), 3) if per_hop > 0 else None}
    for f in af.values():
        f.close()
    a_stream.close()
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
    out = {"suite": "fdaf", "rounds": a.rounds, "hops_per_round": a.hops, "build": build_check(pkg),
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    for B in BLOCKS:
        for C in CHANNELS:
            for K in (B, 4800, 48000):
                out["shapes"][f"B={B} K={K} C={C}"] = run_shape(pkg, torch, np, B, K, C, a.rounds, a.hops, a.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
