#!/usr/bin/env python3
"""Per-hop latency of Stream.denoise_hop against the plain and the masked hop and against
a torch composition of the same algorithm, and the offline gains kernel's throughput.

One process.  A hop is timed on the host clock around the call(s) and a stream
synchronise; each leg has its own objects and runs --hops hops per round after its
warm-up, the legs alternating round by round.  Per leg: the median over the rounds of
the round's p50 and p99, and the spread of the p50s over the rounds.
  a   Stream.push_hop: the hop path with no spectral step
  m   Stream.push_hop_masked with a ready mask row per channel
  f   Stream.denoise_hop, fused route: one launch (shapes that have it)
  s   Stream.denoise_hop, staged route: stft_hop, the gains kernel with F = 1, istft_hop
  t   the same algorithm composed from Stream.stft_hop, torch tensor arithmetic on the
      spectrum and the state, and Stream.istft_hop
Shapes: 256/128, 512/128, 1024/256, 2 and 64 channels.
Before timing: over the check hops the fused and the staged route give the same bits,
and the torch composition's output agrees with them to 1e-2 rel-L2 (a presence compare
may flip on a rounding difference).
Gains kernel: Denoiser.gains over 1876 frames of N = 1024 spectra at 1 stream and at 1024
streams, device time on events, over the bytes it moves (8 per bin read, 4 written);
bytes/s and its ratio to a device-to-device copy moving the same number of bytes.
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

SHAPES = ((256, 128), (512, 128), (1024, 256))
CHANNELS = (2, 64)
LEGS = ("a", "m", "f", "s", "t")
WINDOW = 64


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


class TorchDenoise:
    """Steps 1 - 6 of the contract in torch tensor arithmetic between stft_hop and istft_hop."""

    def __init__(self, pkg, torch, plan, C, dev):
        self.torch, self.st = torch, pkg.Stream(plan, C)
        bins = plan.frame_size // 2 + 1
        self.spec = torch.zeros((C, bins), dtype=torch.complex64, device=dev)
        self.S = self.Smin = self.Stmp = self.p = self.lam = self.A2 = None
        self.k = 0

    def push(self, hop, out):
        torch = self.torch
        spec, em = self.st.stft_hop(hop, spec=self.spec)
        if not em:
            return out, 0
        X = torch.view_as_real(spec)
        P = X[..., 0] * X[..., 0] + X[..., 1] * X[..., 1]
        if self.k == 0:
            self.S, self.Smin, self.Stmp, self.lam = P.clone(), P.clone(), P.clone(), P.clone()
            self.p, self.A2 = torch.zeros_like(P), torch.zeros_like(P)
        else:
            self.S = 0.8 * self.S + 0.2 * P
            if self.k % WINDOW == 0:
                self.Smin = torch.minimum(self.Stmp, self.S)
                self.Stmp = self.S.clone()
            else:
                self.Smin = torch.minimum(self.Smin, self.S)
                self.Stmp = torch.minimum(self.Stmp, self.S)
            present = (self.S > 5.0 * self.Smin).to(P.dtype)
            self.p = 0.2 * self.p + 0.8 * present
            ad = 0.95 + 0.05 * self.p
            self.lam = ad * self.lam + (1.0 - ad) * P
        lc = torch.clamp_min(self.lam, 1e-30)
        xi = 0.98 * (self.A2 / lc) + 0.02 * torch.clamp_min(P / lc - 1.0, 0.0)
        G = torch.clamp_min(xi / (1.0 + xi), 0.1)
        self.A2 = G * G * P
        self.k += 1
        self.st.istft_hop(spec, mask=G, out=out)
        return out, hop.shape[-1]


def run_shape(pkg, torch, N, H, C, rounds, hops, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xD0 ^ N ^ (C << 16))
    xs = [(torch.randn((C, H), generator=g, device=dev, dtype=torch.float32) * 0.25).contiguous() for _ in range(64)]
    plan = pkg.Plan(frame_size=N, hop_size=H, boundary_mode=pkg.DROP)
    bins = N // 2 + 1
    out = torch.zeros((C, H), dtype=torch.float32, device=dev)
    cur = torch.cuda.current_stream()

    def make(route):
        dn = pkg.Denoiser(plan, C, window=WINDOW)
        dn.set_route(route)
        dn.prepare()
        return dn

    fused_ok = make(0).fused_ok
    legs_here = tuple(k for k in LEGS if k != "f" or fused_ok)

    # ---- the routes against each other (bits) and against the torch composition
    n_check = 2 * WINDOW + N // H + 3
    routes = {r: (make(r), pkg.Stream(plan, C)) for r in ((1, 2) if fused_ok else (2,))}
    tc = TorchDenoise(pkg, torch, plan, C, dev)
    num = den = 0.0
    for j in range(n_check):
        ys = {r: st.denoise_hop(dn, xs[j % 64])[0].clone() for r, (dn, st) in routes.items()}
        yt, em = tc.push(xs[j % 64], torch.empty_like(out))
        if fused_ok and not same_bits(torch, ys[1], ys[2]):
            raise SystemExit(f"N={N} H={H} C={C}: the fused route differs from the staged one at hop {j}")
        if em:
            num += float(((yt - ys[2]).double() ** 2).sum())
            den += float((ys[2].double() ** 2).sum())
    torch.cuda.synchronize()
    rel = (num / den) ** 0.5
    if not rel <= 1e-2:
        raise SystemExit(f"N={N} H={H} C={C}: the torch composition is {rel:.2e} rel-L2 from the library's")
    auto = make(0)
    pkg.Stream(plan, C).denoise_hop(auto, xs[0])
    chosen = auto.last_launch()["route"]

    streams = {k: pkg.Stream(plan, C) for k in ("a", "m", "f", "s")}
    dns = {"f": make(1) if fused_ok else None, "s": make(2)}
    tleg = TorchDenoise(pkg, torch, plan, C, dev)
    mask = torch.rand((C, bins), generator=g, device=dev, dtype=torch.float32)
    legs = {"a": lambda x: streams["a"].push_hop(x, out),
            "m": lambda x: streams["m"].push_hop_masked(x, mask, out),
            "f": lambda x: streams["f"].denoise_hop(dns["f"], x, out),
            "s": lambda x: streams["s"].denoise_hop(dns["s"], x, out),
            "t": lambda x: tleg.push(x, out)}
    count = {k: 0 for k in LEGS}

    def one(name):
        j = count[name] % 64
        t0 = time.perf_counter_ns()
        legs[name](xs[j])
        cur.synchronize()
        count[name] += 1
        return (time.perf_counter_ns() - t0) * 1e-3

    for name in legs_here:
        for _ in range(warmup):
            one(name)
    p50 = {k: [] for k in legs_here}
    p99 = {k: [] for k in legs_here}
    for _ in range(rounds):
        for name in legs_here:
            us = [one(name) for _ in range(hops)]
            p50[name].append(pct(us, 0.50))
            p99[name].append(pct(us, 0.99))
    res = {"fused_ok": fused_ok, "library_route": chosen}
    for name in legs_here:
        med = statistics.median(p50[name])
        res[name] = {"p50_us": round(med, 2), "p99_us": round(statistics.median(p99[name]), 2),
                     "spread": round((max(p50[name]) - min(p50[name])) / med, 4), "hops": rounds * hops}
    if fused_ok:
        res["f_over_a"] = round(res["f"]["p50_us"] / res["a"]["p50_us"], 3)
        res["f_over_m"] = round(res["f"]["p50_us"] / res["m"]["p50_us"], 3)
        res["s_over_f"] = round(res["s"]["p50_us"] / res["f"]["p50_us"], 3)
        res["t_over_f"] = round(res["t"]["p50_us"] / res["f"]["p50_us"], 3)
    res["s_over_a"] = round(res["s"]["p50_us"] / res["a"]["p50_us"], 3)
    res["t_over_s"] = round(res["t"]["p50_us"] / res["s"]["p50_us"], 3)
    res["check"] = {"fused_bit_equal_staged": bool(fused_ok), "torch_rel_l2": float(f"{rel:.3e}"), "hops": n_check}
    return res


def run_gains(pkg, torch, S, F, rounds):
    dev = torch.device("cuda:0")
    N, H = 1024, 256
    plan = pkg.Plan(frame_size=N, hop_size=H)
    bins = N // 2 + 1
    spec = torch.view_as_complex(torch.randn((S, F, bins, 2), device=dev, dtype=torch.float32))
    mask = torch.empty((S, F, bins), device=dev, dtype=torch.float32)
    dn = pkg.Denoiser(plan, 1, window=WINDOW)
    dn.gains(spec, mask=mask)
    torch.cuda.synchronize()
    moved = S * F * bins * 12

    def timed(fn, n):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(n):
            fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) / n * 1e-3

    n = 5
    k_s = statistics.median(timed(lambda: dn.gains(spec, mask=mask), n) for _ in range(rounds))
    src = torch.empty(moved // 8, dtype=torch.float32, device=dev)  # a copy moves 2 x its size
    dst = torch.empty_like(src)
    c_s = statistics.median(timed(lambda: dst.copy_(src), n) for _ in range(rounds))
    copy_bps = src.numel() * 8 / c_s
    return {"streams": S, "frames": F, "bins": bins, "bytes": moved, "seconds": float(f"{k_s:.4e}"),
            "gbytes_per_s": round(moved / k_s * 1e-9, 2), "copy_gbytes_per_s": round(copy_bps * 1e-9, 2),
            "fraction_of_copy": round(moved / k_s / copy_bps, 4), "grid": dn.last_launch()["grids"][0]}


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
    out = {"suite": "denoise", "rounds": a.rounds, "hops_per_round": a.hops, "build": build_check(pkg),
           "device": torch.cuda.get_device_name(0), "shapes": {}, "gains": {}}
    for N, H in SHAPES:
        for C in CHANNELS:
            out["shapes"][f"N={N} H={H} C={C}"] = run_shape(pkg, torch, N, H, C, a.rounds, a.hops, a.warmup)
    for S in (1, 1024):
        out["gains"][f"S={S} F=1876"] = run_gains(pkg, torch, S, 1876, a.rounds)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
