#!/usr/bin/env python3
"""The cross-spectral estimator's accumulate kernel against a device copy, and the per-hop
delay tracker against a torch composition of the same algorithm.

One process.
Accumulate: CrossSpectrum.accumulate (k_xspec_acc) over 1876 frames of N = 1024 spectra at
1, 64 and 1024 pairs, device time on events, over the bytes it moves (16 per bin and frame
read, 16 per bin written); bytes/s and its ratio to a device-to-device copy moving the same
number of bytes.
Tracker: per hop two Stream.stft_hop (reference and desired), then, once a frame completes,
  l   CrossSpectrum.accumulate with F = 1 on the carried state, then CrossSpectrum.delay
  t   the same from torch tensor arithmetic on the spectra and the state, torch.fft.irfft,
      torch.argmax and the parabolic refinement
timed on the host clock around the calls and a stream synchronise; each leg has its own
objects and runs --hops hops per round after its warm-up, the legs alternating round by
round.  Per leg: the median over the rounds of the round's p50 and p99, and the spread of
the p50s.  Shapes 512/128 and 1024/256, 2 and 64 pairs, exponential averaging (alpha 0.9).
Before timing: over the check hops the two legs agree in the integer lag of every pair.
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

SHAPES = ((512, 128), (1024, 256))
PAIRS = (2, 64)
LEGS = ("l", "t")
ALPHA = 0.9
DELAY = 17


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


class Tracker:
    """Two analysis streams, the carried averages and the delay, by the library or by torch."""

    def __init__(self, pkg, torch, plan, P, dev, use_lib):
        self.torch, self.plan, self.use_lib = torch, plan, use_lib
        self.sa, self.sb = pkg.Stream(plan, P), pkg.Stream(plan, P)
        N = plan.frame_size
        bins = N // 2 + 1
        self.N, self.m = N, N // 2 - 1
        self.ra = torch.zeros((P, bins), dtype=torch.complex64, device=dev)
        self.rb = torch.zeros((P, bins), dtype=torch.complex64, device=dev)
        self.out = torch.zeros((P, 3), dtype=torch.float32, device=dev)
        if use_lib:
            self.xs = pkg.CrossSpectrum(plan, P, ALPHA)
            self.xs.prepare()
        else:
            self.Sab = torch.zeros((P, bins), dtype=torch.complex64, device=dev)
            self.rows = torch.arange(P, device=dev)

    def push(self, hop_a, hop_b):
        torch = self.torch
        _, ea = self.sa.stft_hop(hop_a, spec=self.ra)
        _, eb = self.sb.stft_hop(hop_b, spec=self.rb)
        if not (ea and eb):
            return None
        if self.use_lib:
            self.xs.accumulate(self.ra[:, None, :], self.rb[:, None, :], carry=True)
            return self.xs.delay(out=self.out)
        # the delay needs Sab alone: the torch leg skips Saa and Sbb
        self.Sab = ALPHA * self.Sab + (1.0 - ALPHA) * (torch.conj(self.ra) * self.rb)
        W = self.Sab / torch.clamp_min(torch.abs(self.Sab), 1e-30)
        cc = torch.fft.irfft(W, n=self.N, dim=-1)
        m = self.m
        win = torch.cat([cc[:, -m:], cc[:, :m + 1]], dim=1)
        j = torch.argmax(win, dim=1)
        lag = j - m
        y0, y1, y2 = cc[self.rows, (lag - 1) % self.N], cc[self.rows, lag % self.N], cc[self.rows, (lag + 1) % self.N]
        den = (y0 - 2.0 * y1) + y2
        frac = torch.where(den == 0, torch.zeros_like(den), 0.5 * (y0 - y2) / den)
        self.out[:, 0], self.out[:, 1], self.out[:, 2] = lag.to(torch.float32), frac, y1
        return self.out


def run_tracker(pkg, torch, N, H, P, rounds, hops, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC5 ^ N ^ (P << 16))
    n_hops = 64
    base = torch.randn((P, n_hops * H + DELAY), generator=g, device=dev, dtype=torch.float32) * 0.25
    xa = base[:, DELAY:]
    xb = base[:, :n_hops * H] + 0.025 * torch.randn((P, n_hops * H), generator=g, device=dev, dtype=torch.float32)
    ha = [xa[:, q * H:(q + 1) * H].contiguous() for q in range(n_hops)]
    hb = [xb[:, q * H:(q + 1) * H].contiguous() for q in range(n_hops)]
    plan = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True, boundary_mode=pkg.DROP)
    cur = torch.cuda.current_stream()

    # ---- the two legs against each other: the integer lag of every pair, once the average has settled
    chk = {k: Tracker(pkg, torch, plan, P, dev, k == "l") for k in LEGS}
    n_check = N // H + 40
    agreed = 0
    for q in range(n_check):
        outs = {k: t.push(ha[q % n_hops], hb[q % n_hops]) for k, t in chk.items()}
        if outs["l"] is None or q < N // H + 20 or (q + 1) % n_hops < N // H:
            continue  # (the hops wrap: frames that straddle the seam are not a delayed pair)
        la, lt = outs["l"][:, 0].cpu().tolist(), outs["t"][:, 0].cpu().tolist()
        if la != lt or any(int(v) != DELAY for v in la):
            raise SystemExit(f"N={N} H={H} P={P}: hop {q}: the library's lags {la[:4]} and torch's {lt[:4]} (delay {DELAY})")
        agreed += 1
    torch.cuda.synchronize()

    legs = {k: Tracker(pkg, torch, plan, P, dev, k == "l") for k in LEGS}
    count = {k: 0 for k in LEGS}

    def one(name):
        j = count[name] % n_hops
        t0 = time.perf_counter_ns()
        legs[name].push(ha[j], hb[j])
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
    res = {}
    for name in LEGS:
        med = statistics.median(p50[name])
        res[name] = {"p50_us": round(med, 2), "p99_us": round(statistics.median(p99[name]), 2),
                     "spread": round((max(p50[name]) - min(p50[name])) / med, 4), "hops": rounds * hops}
    res["t_over_l"] = round(res["t"]["p50_us"] / res["l"]["p50_us"], 3)
    res["check"] = {"hops_with_equal_integer_lag": agreed, "delay": DELAY}
    return res


def run_acc(pkg, torch, P, F, rounds):
    dev = torch.device("cuda:0")
    N, H = 1024, 256
    plan = pkg.Plan(frame_size=N, hop_size=H)
    bins = N // 2 + 1
    A = torch.view_as_complex(torch.randn((P, F, bins, 2), device=dev, dtype=torch.float32))
    B = torch.view_as_complex(torch.randn((P, F, bins, 2), device=dev, dtype=torch.float32))
    state = torch.empty((P, 4, bins), device=dev, dtype=torch.float32)
    xs = pkg.CrossSpectrum(plan, 1)
    xs.accumulate(A, B, state_out=state)
    torch.cuda.synchronize()
    moved = P * F * bins * 16 + P * bins * 16

    def timed(fn, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n * 1e-3

    n = 5
    k_s = statistics.median(timed(lambda: xs.accumulate(A, B, state_out=state), n) for _ in range(rounds))
    src = torch.empty(moved // 8, dtype=torch.float32, device=dev)  # a copy moves 2 x its size
    dst = torch.empty_like(src)
    dst.copy_(src)
    c_s = statistics.median(timed(lambda: dst.copy_(src), n) for _ in range(rounds))
    copy_bps = src.numel() * 8 / c_s
    return {"pairs": P, "frames": F, "bins": bins, "bytes": moved, "seconds": float(f"{k_s:.4e}"),
            "us_per_frame": round(k_s / F * 1e6, 4), "gbytes_per_s": round(moved / k_s * 1e-9, 2),
            "copy_gbytes_per_s": round(copy_bps * 1e-9, 2), "fraction_of_copy": round(moved / k_s / copy_bps, 4),
            "grid": xs.last_launch()["grids"][0]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hops", type=int, default=300, help="timed hops per leg and round")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    out = {"suite": "xspec", "rounds": a.rounds, "hops_per_round": a.hops, "build": build_check(pkg),
           "device": torch.cuda.get_device_name(0), "accumulate": {}, "tracker": {}}
    for P in (1, 64, 1024):
        out["accumulate"][f"P={P} F=1876"] = run_acc(pkg, torch, P, 1876, a.rounds)
    for N, H in SHAPES:
        for P in PAIRS:
            out["tracker"][f"N={N} H={H} P={P}"] = run_tracker(pkg, torch, N, H, P, a.rounds, a.hops, a.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
