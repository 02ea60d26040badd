#!/usr/bin/env python3
"""Measure Griffin-Lim against the loop a user writes around Plan.stft / Plan.istft_ola.

Cases: 1024/256 and 512/128; --streams x --samples and --few-streams x --samples;
--iters iterations; momentum 0.99 and 0.  Legs, timed in one process, alternating
by round, each with its own warm-up and device events around its calls:
  a   the loop on Plan.stft / Plan.istft_ola with the projection in torch ops
  b   the same loop with Plan.gl_project
  c   Plan.griffin_lim
Before timing, at the timed size and with frame pairing off: c equals b bit for
bit; the spectral convergence of c is reported.  The timed plans keep the default
pairing.  Per case: ms per iteration, Msamples/s per iteration and the share of
8 TB/s against the derived traffic of the fused walk (16 B per output sample
without momentum, 48 B with it).  Prints one JSON line (and writes it to --out).
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
SHAPES = ((1024, 256), (512, 128))
MOMENTA = (0.99, 0.0)


def time_leg(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def loop(torch, plan, mag, n_iter, momentum, project):
    y = plan.istft_ola(torch.complex(mag, torch.zeros_like(mag)))
    tprev = None
    for _ in range(n_iter):
        X = plan.stft(y)
        y = plan.istft_ola(project(X, mag, tprev if momentum > 0 else None, momentum))
        tprev = X
    return y


def torch_project(torch):
    def project(X, mag, tprev, momentum):
        c = X if tprev is None else X - tprev * (momentum / (1.0 + momentum))
        return c * (mag / (c.abs() + 1e-16))
    return project


def spectral_convergence(torch, plan, y, mag):
    return float(torch.linalg.norm(plan.stft(y).abs() - mag) / torch.linalg.norm(mag))


def run_case(pkg, torch, n, h, S, T, momentum, n_iter, rounds, calls, warmup):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0xC0FFEE ^ S ^ n)
    t = torch.arange(T, device=dev, dtype=torch.float32)
    f0 = 0.01 + 0.05 * torch.rand((S, 1), generator=g, device=dev)
    x = 0.5 * torch.sin(2 * torch.pi * f0 * t) + 0.05 * torch.randn((S, T), generator=g, device=dev)
    plan = pkg.Plan(frame_size=n, hop_size=h)
    check = pkg.Plan(frame_size=n, hop_size=h, frame_pairing=False)
    F = plan.frame_count(T)
    mag = plan.stft(x).abs().contiguous()
    del x, t
    y_c = torch.empty((S, F * h), dtype=torch.float32, device=dev)
    gl = lambda X, m, tp, mom: plan.gl_project(X, m, tp, mom)  # noqa: E731
    legs = {"a": lambda: loop(torch, plan, mag, n_iter, momentum, torch_project(torch)),
            "b": lambda: loop(torch, plan, mag, n_iter, momentum, gl),
            "c": lambda: plan.griffin_lim(mag, n_iter, momentum, y=y_c)}

    # ---- correctness at the timed size (pairing off: the bit contract's reference)
    want = loop(torch, check, mag, n_iter, momentum, lambda X, m, tp, mom: check.gl_project(X, m, tp, mom))
    got = check.griffin_lim(mag, n_iter, momentum)
    torch.cuda.synchronize()
    same = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    del want, got
    if not same:
        raise SystemExit(f"{n}/{h} S={S} momentum={momentum}: c does not equal b bit for bit")
    legs["c"]()
    rec = plan.last_launch()
    sc = spectral_convergence(torch, plan, y_c, mag)
    sc0 = spectral_convergence(torch, plan, plan.griffin_lim(mag, 0, momentum), mag)

    # ---- timing
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            ms[name].append(time_leg(torch, fn, calls))
    samples = float(S) * F * h
    res = {}
    for name, v in ms.items():
        med = statistics.median(v)
        per_it = med / (n_iter + 1)  # (y_0 counts as one step of the same size)
        res[name] = {"ms_per_call": round(med, 4), "spread": round((max(v) - min(v)) / med, 4),
                     "ms_per_iteration": round(per_it, 5),
                     "msamples_per_s_per_iteration": round(samples / (per_it * 1e-3) / 1e6, 1),
                     "calls": rounds * calls}
    derived = (48.0 if momentum > 0 else 16.0) * samples
    res["c"].update({"derived_bytes_per_iteration": derived,
                     "derived_hbm_share": round(derived / (res["c"]["ms_per_iteration"] * 1e-3) / HBM_BYTES_PER_S, 4),
                     "kernels_last_iteration": rec["kernels"], "n_chunks": rec["n_chunks"], "grid": rec["grid"]})
    res["speedup_c_over_b"] = round(res["b"]["ms_per_call"] / res["c"]["ms_per_call"], 3)
    res["speedup_c_over_a"] = round(res["a"]["ms_per_call"] / res["c"]["ms_per_call"], 3)
    res["check"] = {"c_bit_equal_b_pairing_off": same, "sc_y0": round(sc0, 5), "sc_c": round(sc, 5)}
    res["frames"] = F
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--few-streams", type=int, default=16)
    ap.add_argument("--samples", type=int, default=480_000)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1, help="calls per leg and round")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_pkg
    pkg = load_pkg()
    out = {"suite": "griffin_lim", "iters": a.iters,
           "build": {k: v for k, v in pkg.build_info().items() if k != "path"},
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for n, h in SHAPES:
        for S in (a.streams, a.few_streams):
            for momentum in MOMENTA:
                key = f"{n}/{h} S={S} T={a.samples} momentum={momentum}"
                out["cases"][key] = run_case(pkg, torch, n, h, S, a.samples, momentum, a.iters, a.rounds, a.calls,
                                             a.warmup)
                print(key, json.dumps(out["cases"][key]), file=sys.stderr, flush=True)
                torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
