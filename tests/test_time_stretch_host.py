"""CPU tests of the time stretch's host side (include/crlot_dsp.h, "time stretch"):
the four symbols are declared, exported and bound; the two kernel ids have their
names; crlot_stretch_frame_count is the predicate's count and refuses bad rates;
Plan.phase_vocoder's layout check refuses each bad tensor before anything touches
a device; the C++ mirror compiles.  No GPU compute here."""
import os
import re
import subprocess

import numpy as np
import pytest

import phase_vocoder_reference as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["crlot_stretch_frame_count", "crlot_stretch_output_length", "crlot_phase_vocoder", "crlot_time_stretch"]


def test_new_symbols_declared_exported_and_bound(pkg):
    L = pkg.lib()
    syms = pkg.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\b(crlot_[a-z0-9_]+)\b", out))
    for name in NEW_SYMBOLS:
        assert name in syms, name
        assert name in exported, name
        assert getattr(L, name).argtypes is not None, name
    assert L.crlot_abi_version() == 2
    for kid, name in ((35, "k_phase_voc"), (36, "k_phase_voc_sums")):
        assert pkg.kernel_name(kid) == name
    assert callable(pkg.Plan.phase_vocoder) and callable(pkg.Plan.time_stretch)
    assert callable(pkg.Plan.stretch_output_length)


def test_stretch_frame_count(pkg):
    L = pkg.lib()
    for F in (1, 2, 7, 40, 1875):
        for rate in (0.1, 1 / 3, 0.5, 0.75, 1, 1.3, 2, 3.7, 7):
            n = pkg.stretch_frame_count(F, rate)
            assert n == PV.frame_count(F, rate) == len(np.arange(0, F, rate)), (F, rate, n)
    assert pkg.stretch_frame_count(0, 1.3) == 0
    assert pkg.stretch_frame_count(5, 1 / 64) == 320 and pkg.stretch_frame_count(5, 64.0) == 1
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1 / 65, 64.5):
        assert L.crlot_stretch_frame_count(40, bad) == pkg.EINVAL, bad
        with pytest.raises(ValueError):
            pkg.stretch_frame_count(40, bad)
    assert L.crlot_stretch_frame_count(-1, 1.0) == pkg.EINVAL
    assert L.crlot_stretch_frame_count(2 ** 31, 1.0) == pkg.EINVAL        # F' > 2^31 - 1
    assert L.crlot_stretch_frame_count(2 ** 31 - 1, 1.0) == 2 ** 31 - 1
    assert L.crlot_stretch_frame_count(2 ** 26, 1 / 64) == pkg.EINVAL


def test_entries_reject_before_device(pkg):
    L = pkg.lib()
    assert L.crlot_phase_vocoder(None, None, None, 1, 4, 1.0, 0, 0, 0, 0, None) == pkg.EINVAL
    assert L.crlot_time_stretch(None, None, None, 1, 4, 1.0, 0, 0, None) == pkg.EINVAL
    assert L.crlot_stretch_output_length(None, 4, 1.0) == pkg.EINVAL


def test_stretch_spec_layout(pkg):
    """Every bad case differs from the good one in one thing."""
    S, F, bins, dev = 3, 16, 513, 0
    ok = ((S, F, bins), (F * bins, bins, 1), "complex64", 0)
    assert pkg._stretch_spec_layout(*ok, dev, bins) == (2 * F * bins, 2 * bins)
    padded = ((S, F, bins), ((F + 2) * (bins + 3), bins + 3, 1), "complex64", 0)
    assert pkg._stretch_spec_layout(*padded, dev, bins) == (2 * (F + 2) * (bins + 3), 2 * (bins + 3))
    # size-1 dims: their strides are meaningless
    assert pkg._stretch_spec_layout((1, 1, bins), (0, 0, 1), "complex64", 0, dev, bins) == (2 * bins, 2 * bins)
    assert pkg._stretch_spec_layout(*ok, dev, bins, "out", (S, F, bins)) == (2 * F * bins, 2 * bins)
    for bad in (((S, F, bins), (F * bins, bins, 1), "float32", 0),            # dtype
                ((S, F, bins), (F * bins, bins, 1), "complex128", 0),
                ((S, F, bins), (F * bins, bins, 1), "complex64", None),       # a host tensor
                ((S, F, bins), (F * bins, bins, 1), "complex64", 1),          # another device
                ((S, F, bins), (2 * F * bins, 2 * bins, 2), "complex64", 0),  # rows not contiguous
                ((S, F, bins), (F * bins, bins - 1, 1), "complex64", 0),      # ld_frame < N+2 floats
                ((S, F, bins), ((F - 1) * bins, bins, 1), "complex64", 0),    # streams overlap
                ((S, F, bins - 1), (F * (bins - 1), bins - 1, 1), "complex64", 0),  # wrong bin count
                ((F, bins), (bins, 1), "complex64", 0)):                      # not 3-d
        with pytest.raises(ValueError):
            pkg._stretch_spec_layout(*bad, dev, bins)
    with pytest.raises(ValueError):  # an output of the wrong shape
        pkg._stretch_spec_layout(*ok, dev, bins, "out", (S, F + 1, bins))
    # the torch front: a CPU tensor and a wrong dtype are refused before any call
    import torch
    plan = object.__new__(pkg.Plan)
    plan.frame_size, plan.hop_size = 1024, 256
    plan.cfg = pkg.PlanConfig(device=0)
    for bad in (torch.zeros(2, 8, 513, dtype=torch.complex64), torch.zeros(2, 8, 513)):
        with pytest.raises(ValueError):
            pkg.Plan.phase_vocoder(plan, bad, 1.3)
    for bad in (torch.zeros(2, 4096), torch.zeros(2, 4096, dtype=torch.float64)):
        with pytest.raises(ValueError):
            pkg.Plan.time_stretch(plan, bad, 1.3)


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(crlot::StftEngine& e, const float* d_x, float* d_y, const float* d_in, float* d_out) {
    e.phase_vocoder_device(d_in, d_out, 3, 40, 1.3, 40 * 1026, 1026, 31 * 1026, 1026);
    e.time_stretch_device(d_x, d_y, 3, 10000, 0.8, 10000, e.stretch_output_length(10000, 0.8));
    return crlot::StftEngine::stretch_frame_count(40, 1.3);
}
'''


def test_cpp_methods_compile(tmp_path):
    src = tmp_path / "stretch_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
