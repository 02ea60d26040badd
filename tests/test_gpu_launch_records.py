"""Every entry launches the kernels, grids and chunk counts the fixture records.

The host launch layer decides which kernels a call runs, over which grid and in
how many chunks per stream.  None of that shows in the output bits (every route
of a shape computes the same values, the parity tests prove it), so a change of
the launch layer is checked here against tests/golden/launch_records.json: for
each plan, batch and entry the record crlot_plan_last_launch returns after the
call -- kernels in launch order, the grid of each, chunks per stream, kernel
count -- or the class of the exception the call raises.

The grids scale with the device's compute-unit count, which the fixture stores;
on a device with another count the comparison means nothing and the test skips
(the only skip).  `python tests/test_gpu_launch_records.py --write` regenerates
the fixture from the library in the tree: do that only with a library whose
launch behaviour is the one to pin.
"""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_records.json")

FQ_REFLECT = {"boundary_mode": 2, "pad_mode": 1}
# id -> (frame, hop, plan options); "gain" sets a spectral gain after creation
PLANS = {f"{n}/{h}": (n, h, {}) for n, h in [
    (256, 128), (512, 128), (512, 512), (1024, 128), (1024, 256), (1024, 1024), (1024, 300), (2048, 256),
    (2048, 512), (4096, 512), (4096, 1024), (960, 240), (480, 120), (882, 441), (1000, 250), (1764, 441),
    (1920, 480), (100, 50),
    (1920, 455),  # an odd hop: K_pairN's 1920, not K_pair30's
]}
PLANS.update({
    "1024/256-unpaired": (1024, 256, {"frame_pairing": False}),
    "1024/256-two-regime": (1024, 256, {"frame_pairing": 2}),
    "1024/256-gain": (1024, 256, {"gain": True}),
    "1024/256-fq-reflect": (1024, 256, dict(FQ_REFLECT)),
    "4096/1024-gain": (4096, 1024, {"gain": True}),
    "4096/1024-unpaired": (4096, 1024, {"frame_pairing": False}),
    "960/240-unpaired": (960, 240, {"frame_pairing": False}),
})

BATCHES = [(1, 9), (3, 40), (8, 300)]
DEEP = (2048, 130)               # the only batch several resident rounds deep; H <= 256 only
KNOB_BATCH, KNOBS = (8, 300), (3, 1000)
INTERLEAVED = ("1024/256", "512/128")
UNALIGNED = ("1024/256", "512/128", "2048/512")


def _record(plan):
    r = plan.last_launch()
    return {"kernels": r["kernels"], "grid": r["grid"], "n_chunks": r["n_chunks"], "n_kernels": r["n_kernels"]}


def _call(plan, fn):
    try:
        fn()
    except Exception as e:  # recorded and compared like a launch record
        return {"raises": type(e).__name__}
    return _record(plan)


def _rand(torch, gen, shape):
    return torch.rand(shape, generator=gen, device="cuda") - 0.5


def _entries(pkg, torch, plan, gen, S, F, interleaved):
    """(name, record) of every entry at one batch, under the plan's current chunk knob."""
    n, h = plan.frame_size, plan.hop_size
    T = F * h
    x = _rand(torch, gen, (S, T))
    out = [("roundtrip", _call(plan, lambda: plan.roundtrip(x)))]

    def masked():
        plan.set_spectral_mask(torch.ones((plan.frame_count(T), n // 2 + 1), dtype=torch.float32, device="cuda"))
        try:
            plan.roundtrip(x)
        finally:
            plan.set_spectral_mask(None)
    out.append(("roundtrip_masked", _call(plan, masked)))

    spec = []
    out.append(("stft", _call(plan, lambda: spec.append(plan.stft(x)))))
    if spec:
        out.append(("istft_ola", _call(plan, lambda: plan.istft_ola(spec[0]))))
    del spec
    out.append(("spectrogram", _call(plan, lambda: pkg.Features(plan, kind=pkg.FEAT_POWER).spectrogram(x))))
    del x
    if interleaved:
        for C in (2, 6):
            xi = _rand(torch, gen, (S, T, C))
            out.append((f"roundtrip_interleaved C={C}", _call(plan, lambda: plan.roundtrip_interleaved(xi))))
            del xi
    torch.cuda.synchronize()
    return out


def _unaligned(torch, plan, gen, S, F):
    """roundtrip and the masked roundtrip with x and y one float into their allocations."""
    n, h = plan.frame_size, plan.hop_size
    T = F * h
    L = plan.output_length(T)
    x = _rand(torch, gen, (S * T + 1,))[1:].view(S, T)
    y = torch.empty(S * L + 1, dtype=torch.float32, device="cuda")[1:].view(S, L)
    assert x.data_ptr() % 8 == 4 and y.data_ptr() % 8 == 4
    out = [("roundtrip", _call(plan, lambda: plan.roundtrip(x, y)))]

    def masked():
        plan.set_spectral_mask(torch.ones((plan.frame_count(T), n // 2 + 1), dtype=torch.float32, device="cuda"))
        try:
            plan.roundtrip(x, y)
        finally:
            plan.set_spectral_mask(None)
    out.append(("roundtrip_masked", _call(plan, masked)))
    torch.cuda.synchronize()
    return out


def records_of(pkg, torch, plan_id):
    """{case: record} of one plan: every batch, entry, chunk knob and alignment case."""
    n, h, opts = PLANS[plan_id]
    opts = dict(opts)
    gain = opts.pop("gain", False)
    plan = pkg.Plan(frame_size=n, hop_size=h, **opts)
    if gain:
        plan.set_spectral_gain(np.linspace(1.0, 0.5, n // 2 + 1, dtype=np.float32))
    gen = torch.Generator(device="cuda").manual_seed(1000 * n + h)
    inter = plan_id in INTERLEAVED
    recs = {}
    for S, F in BATCHES + ([DEEP] if h <= 256 else []):
        for name, r in _entries(pkg, torch, plan, gen, S, F, inter):
            recs[f"{S}x{F} {name}"] = r
    for knob in KNOBS:
        plan.set_chunks(knob)
        try:
            for name, r in _entries(pkg, torch, plan, gen, *KNOB_BATCH, inter):
                recs[f"{KNOB_BATCH[0]}x{KNOB_BATCH[1]} chunks={knob} {name}"] = r
        finally:
            plan.set_chunks(0)
    if plan_id in UNALIGNED:
        for name, r in _unaligned(torch, plan, gen, 3, 40):
            recs[f"3x40 4-byte aligned {name}"] = r
    plan.close()
    return recs


@pytest.fixture(scope="module")
def fixture(torch_cuda):
    with open(FIXTURE) as f:
        fx = json.load(f)
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    if cus != fx["cus"]:
        pytest.skip(f"the fixture was recorded on {fx['cus']} compute units, this device has {cus}")
    return fx


@pytest.mark.parametrize("plan_id", list(PLANS))
def test_launch_records(pkg, torch_cuda, fixture, plan_id):
    want = fixture["plans"][plan_id]
    got = records_of(pkg, torch_cuda, plan_id)
    assert sorted(got) == sorted(want), (plan_id, sorted(set(got) ^ set(want)))
    diff = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not diff, (plan_id, diff)


def _write():
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    fx = {"cus": torch.cuda.get_device_properties(0).multi_processor_count,
          "library": pkg.build_info()["src"],
          "plans": {pid: records_of(pkg, torch, pid) for pid in PLANS}}
    with open(FIXTURE, "w") as f:
        f.write("{\n" + f' "cus": {fx["cus"]},\n "library": {json.dumps(fx["library"])},\n "plans": {{\n')
        rows = []
        for pid, recs in fx["plans"].items():
            cases = ",\n".join(f"   {json.dumps(c)}: {json.dumps(r)}" for c, r in recs.items())
            rows.append(f"  {json.dumps(pid)}: {{\n{cases}\n  }}")
        f.write(",\n".join(rows) + "\n }\n}\n")
    n = sum(len(r) for r in fx["plans"].values())
    raised = [(p, c) for p, r in fx["plans"].items() for c, v in r.items() if "raises" in v]
    print(f"wrote {FIXTURE}: {len(PLANS)} plans, {n} cases, {len(raised)} raising: {raised}")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gpu_launch_records.py --write")
    _write()
