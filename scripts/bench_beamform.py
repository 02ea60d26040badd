#!/usr/bin/env python3
"""The beamformer's apply and accumulate kernels against a device copy, and the per-hop
entry against a torch composition of the same algorithm.

One process.
Kernels: Beamformer.apply (k_bf_apply) and Beamformer.accumulate (k_bf_acc, target 0) over
1876 frames of N = 1024 spectra, M = 2, 4, 8 microphones, G = 1, 64, 512 groups, device
time on events, over the bytes each moves (apply: 8 M per bin and frame read, 8 written,
16 M per bin of weights; accumulate: the two matrices' waves each read the M rows and the
mask, 2 (8 M + 4) per bin and frame, and write 8 M M per bin); bytes/s and its ratio to a
device-to-device copy moving the same number of bytes.  A combination whose spectra exceed
--max-gib is skipped and listed.
Per hop: Beamformer.hop (stft_hop -> k_bf_hop -> istft_hop, three launches)
  l   the library
  t   the same from torch: a carried history, torch.fft.rfft of the windowed frame, the
      covariance updates by einsum, torch.linalg.solve of the loaded noise matrices
      against the target matrices, the weights, einsum for the output row,
      torch.fft.irfft and a windowed overlap-add
timed on the host clock around the call and a stream synchronise; each leg has its own
objects and runs --hops hops per round after its warm-up, the legs alternating round by
round.  Per leg: the median over the rounds of the round's p50 and p99, and the spread of
the p50s.  Shapes 512/128 and 1024/256, M = 4, G = 1 and 16, alpha 0.95, update_every 1.
Before timing: over the check hops the two legs' weights agree within the float64 bar of
the tests (7e-4 of the largest weight).
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
LEGS = ("l", "t")
ALPHA = 0.95
LOADING = 1e-3
WEIGHT_BAR = 7e-4


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


def run_kernels(pkg, torch, M, G, F, rounds):
    dev = torch.device("cuda:0")
    N, H = 1024, 256
    plan = pkg.Plan(frame_size=N, hop_size=H)
    bins = N // 2 + 1
    X = torch.view_as_complex(torch.randn((G, M, F, bins, 2), device=dev, dtype=torch.float32))
    mask = torch.rand((G, F, bins), device=dev, dtype=torch.float32)
    w = torch.view_as_complex(torch.randn((G, M, bins, 2), device=dev, dtype=torch.float32))
    out = torch.empty((G, F, bins), device=dev, dtype=torch.complex64)
    state = torch.empty((G, 2, M * M, bins), device=dev, dtype=torch.float32)
    bf = pkg.Beamformer(plan, M, 1)
    res, n = {}, 5
    for name, fn, moved in (
            ("apply", lambda: bf.apply(X, w, out=out), G * bins * (F * 8 * (M + 1) + 16 * M)),
            ("accumulate", lambda: bf.accumulate(X, mask, state_out=state), G * bins * (F * 2 * (8 * M + 4) + 8 * M * M))):
        fn()
        torch.cuda.synchronize()
        grid = bf.last_launch()["grids"][0]
        k_s = statistics.median(timed(torch, fn, n) for _ in range(rounds))
        bps = copy_rate(torch, moved, rounds)
        res[name] = {"bytes": moved, "seconds": float(f"{k_s:.4e}"), "us_per_frame": round(k_s / F * 1e6, 4),
                     "gbytes_per_s": round(moved / k_s * 1e-9, 2), "copy_gbytes_per_s": round(bps * 1e-9, 2),
                     "fraction_of_copy": round(moved / k_s / bps, 4), "grid": grid}
    bf.close()
    return res


class Hop:
    """One hop of the chain, by the library or by torch."""

    def __init__(self, pkg, torch, plan, G, M, dev, use_lib):
        self.torch, self.use_lib, self.G, self.M = torch, use_lib, G, M
        N, H = plan.frame_size, plan.hop_size
        self.N, self.H = N, H
        bins = N // 2 + 1
        self.out = torch.zeros((G, H), dtype=torch.float32, device=dev)
        if use_lib:
            self.bf = pkg.Beamformer(plan, M, G, alpha=ALPHA, loading=LOADING)
            self.bf.prepare()
            self.s_in, self.s_out = pkg.Stream(plan, G * M), pkg.Stream(plan, G)
            return
        self.win = torch.from_numpy(pkg.window_table(pkg.HANN, N, True)).to(dev)
        self.hist = torch.zeros((G, M, N), dtype=torch.float32, device=dev)
        self.acc = torch.zeros((G, N), dtype=torch.float32, device=dev)
        self.Ps = torch.zeros((G, bins, M, M), dtype=torch.complex64, device=dev)
        self.Pn = torch.zeros((G, bins, M, M), dtype=torch.complex64, device=dev)
        self.eye = torch.eye(M, dtype=torch.complex64, device=dev)
        self.w = None
        self.q = 0

    def push(self, hop, row):
        torch = self.torch
        if self.use_lib:
            return self.bf.hop(self.s_in, self.s_out, hop, row, self.out)[1]
        G, M, N, H = self.G, self.M, self.N, self.H
        self.hist = torch.cat([self.hist[:, :, H:], hop.view(G, M, H)], dim=2)
        self.q += 1
        if self.q * H < N:
            return 0
        X = torch.fft.rfft(self.hist * self.win, dim=-1)  # (G, M, bins)
        outer = torch.einsum("gib,gjb->gbij", X, torch.conj(X))
        mu = row[:, :, None, None]
        self.Ps = ALPHA * self.Ps + (1.0 - ALPHA) * (mu * outer)
        self.Pn = ALPHA * self.Pn + (1.0 - ALPHA) * ((1.0 - mu) * outer)
        tr = torch.einsum("gbii->gb", self.Pn).real / M
        A = self.Pn + (LOADING * tr).clamp_min(1e-30)[:, :, None, None] * self.eye
        Gm = torch.linalg.solve(A, self.Ps)
        den = torch.einsum("gbii->gb", Gm).real.clamp_min(1e-30)
        self.w = Gm[:, :, :, 0] / den[:, :, None]  # (G, bins, M), the reference microphone's column
        Y = torch.einsum("gbm,gmb->gb", torch.conj(self.w), X)
        y = torch.fft.irfft(Y, n=N, dim=-1) * self.win
        self.acc = self.acc + y
        self.out.copy_(self.acc[:, :H])
        self.acc = torch.cat([self.acc[:, H:], torch.zeros_like(self.acc[:, :H])], dim=1)
        return H


def run_hop(pkg, torch, N, H, G, M, rounds, hops, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xBF ^ N ^ (G << 16))
    n_hops = 64
    bins = N // 2 + 1
    x = torch.randn((G * M, n_hops * H), generator=g, device=dev, dtype=torch.float32) * 0.25
    rows = torch.rand((n_hops, G, bins), generator=g, device=dev, dtype=torch.float32)
    hs = [x[:, q * H:(q + 1) * H].contiguous() for q in range(n_hops)]
    plan = pkg.Plan(frame_size=N, hop_size=H, window_type=pkg.HANN, periodic=True, boundary_mode=pkg.DROP)
    cur = torch.cuda.current_stream()

    # ---- the two legs against each other: the weights, hop by hop
    chk = {k: Hop(pkg, torch, plan, G, M, dev, k == "l") for k in LEGS}
    worst = 0.0
    for q in range(N // H + 40):
        em = {k: t.push(hs[q % n_hops], rows[q % n_hops]) for k, t in chk.items()}
        if em["l"] != em["t"]:
            raise SystemExit(f"N={N} H={H} G={G}: hop {q}: the legs emitted {em}")
        if not em["l"]:
            continue
        wl, wt = chk["l"].bf.weights(), chk["t"].w.permute(0, 2, 1)
        d = float((wl - wt).abs().max() / wt.abs().max())
        worst = max(worst, d)
        if not d <= WEIGHT_BAR:
            raise SystemExit(f"N={N} H={H} G={G}: hop {q}: the legs' weights differ by {d:.2e} of the largest")
    torch.cuda.synchronize()

    legs = {k: Hop(pkg, torch, plan, G, M, dev, k == "l") for k in LEGS}
    count = {k: 0 for k in LEGS}

    def one(name):
        j = count[name] % n_hops
        t0 = time.perf_counter_ns()
        legs[name].push(hs[j], rows[j])
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
    res["check"] = {"weights_within": float(f"{worst:.3e}"), "bar": WEIGHT_BAR}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hops", type=int, default=300, help="timed hops per leg and round")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--frames", type=int, default=1876)
    ap.add_argument("--max-gib", type=float, default=40.0, help="skip a kernel combination whose spectra are larger")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device")
    out = {"suite": "beamform", "rounds": a.rounds, "hops_per_round": a.hops, "build": build_check(pkg),
           "device": torch.cuda.get_device_name(0), "kernels": {}, "skipped": [], "hop": {}}
    for M in (2, 4, 8):
        for G in (1, 64, 512):
            key = f"M={M} G={G} F={a.frames}"
            if G * M * a.frames * 513 * 8 > a.max_gib * 2 ** 30:
                out["skipped"].append(key)
                continue
            out["kernels"][key] = run_kernels(pkg, torch, M, G, a.frames, a.rounds)
            torch.cuda.empty_cache()
    for N, H in SHAPES:
        for G in (1, 16):
            out["hop"][f"N={N} H={H} M=4 G={G}"] = run_hop(pkg, torch, N, H, G, 4, a.rounds, a.hops, a.warmup)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
