"""CPU tests of Griffin-Lim's host side (include/crlot_dsp.h, "Griffin-Lim"): the two
symbols are declared, exported and bound; the two kernel ids have their names;
the entries refuse bad arguments before any device is touched; the Python layout
validators refuse each bad tensor; the C++ mirror compiles.  No GPU compute here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["crlot_gl_project", "crlot_griffin_lim"]


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
    assert len(L.crlot_gl_project.argtypes) == 17 and len(L.crlot_griffin_lim.argtypes) == 14
    assert L.crlot_abi_version() == 2
    for kid, name in ((39, "k_gl_project"), (40, "k_gl_iter")):
        assert pkg.kernel_name(kid) == name
    assert pkg.kernel_name(41) == "unknown"
    assert callable(pkg.Plan.gl_project) and callable(pkg.Plan.griffin_lim)
    txt = open(pkg.HEADER_PATH).read()
    assert "#define CRLOT_K_GL_PROJECT 39" in txt and "#define CRLOT_K_GL_ITER 40" in txt


def test_entries_reject_before_device(pkg):
    L = pkg.lib()
    assert L.crlot_gl_project(None, None, None, None, None, 1, 4, 0.5, 0, 0, 0, 0, 0, 0, 0, 0, None) == pkg.EINVAL
    assert L.crlot_griffin_lim(None, None, 0, 0, None, 0, 0, None, 0, 1, 4, 3, 0.5, None) == pkg.EINVAL


def test_gl_scalars(pkg):
    assert pkg._gl_scalars(0, 0.0) == (0, 0.0)
    assert pkg._gl_scalars(65536, 0.99) == (65536, 0.99)
    for bad in (1.0, -0.1, float("nan"), float("inf"), 1.5):
        with pytest.raises(ValueError):
            pkg._gl_scalars(3, bad)
    for bad in (-1, 65537, 2.5):
        with pytest.raises(ValueError):
            pkg._gl_scalars(bad, 0.5)


def test_gl_mag_layout(pkg):
    """Every bad case differs from the good one in one thing."""
    S, F, bins, dev = 3, 16, 513, 0
    ok = ((S, F, bins), (F * bins, bins, 1), "float32", 0)
    assert pkg._gl_mag_layout(*ok, dev, bins) == (S, F, F * bins, bins)
    padded = ((S, F, bins), ((F + 2) * (bins + 3), bins + 3, 1), "float32", 0)
    assert pkg._gl_mag_layout(*padded, dev, bins) == (S, F, (F + 2) * (bins + 3), bins + 3)
    # size-1 dims: their strides are meaningless
    assert pkg._gl_mag_layout((1, 1, bins), (0, 0, 1), "float32", 0, dev, bins) == (1, 1, bins, bins)
    assert pkg._gl_mag_layout(*ok, dev, bins, "mag", (S, F, bins))[:2] == (S, F)
    for bad in (((S, F, bins), (F * bins, bins, 1), "float64", 0),            # dtype
                ((S, F, bins), (F * bins, bins, 1), "complex64", 0),
                ((S, F, bins), (F * bins, bins, 1), "float32", None),         # a host tensor
                ((S, F, bins), (F * bins, bins, 1), "float32", 1),            # another device
                ((S, F, bins), (2 * F * bins, 2 * bins, 2), "float32", 0),    # rows not contiguous
                ((S, F, bins), (F * bins, bins - 1, 1), "float32", 0),        # rows overlap
                ((S, F, bins), ((F - 1) * bins, bins, 1), "float32", 0),      # streams overlap
                ((S, F, bins - 1), (F * (bins - 1), bins - 1, 1), "float32", 0),  # wrong bin count
                ((F, bins), (bins, 1), "float32", 0)):                        # not 3-d
        with pytest.raises(ValueError):
            pkg._gl_mag_layout(*bad, dev, bins)
    for expect in ((S + 1, F, bins), (S, F + 1, bins)):  # mismatched S / F
        with pytest.raises(ValueError):
            pkg._gl_mag_layout(*ok, dev, bins, "mag", expect)


def test_gl_y_layout(pkg):
    S, L, dev = 3, 4096, 0
    assert pkg._gl_y_layout((S, L), (L, 1), "float32", 0, dev, S, L) == L
    assert pkg._gl_y_layout((S, L + 7), (L + 7, 1), "float32", 0, dev, S, L) == L + 7
    assert pkg._gl_y_layout((1, L), (0, 1), "float32", 0, dev, 1, L) == L
    for bad in (((S, L), (L, 1), "float64", 0),          # dtype
                ((S, L), (L, 1), "float32", None),       # a host tensor
                ((S, L), (L, 1), "float32", 1),          # another device
                ((S, L), (2 * L, 2), "float32", 0),      # rows not contiguous
                ((S, L), (L - 1, 1), "float32", 0),      # rows overlap
                ((S, L - 1), (L - 1, 1), "float32", 0),  # too short
                ((S + 1, L), (L, 1), "float32", 0),      # mismatched S
                ((L,), (1,), "float32", 0)):             # not 2-d
        with pytest.raises(ValueError):
            pkg._gl_y_layout(*bad, dev, S, L)


def test_torch_front_refuses_before_any_call(pkg):
    import torch
    plan = object.__new__(pkg.Plan)
    plan.frame_size, plan.hop_size = 1024, 256
    plan.cfg = pkg.PlanConfig(device=0)
    mag, spec = torch.zeros(2, 8, 513), torch.zeros(2, 8, 513, dtype=torch.complex64)
    for bad in (mag, mag.double(), torch.zeros(2, 8, 512)):  # host tensors, a wrong dtype, wrong bins
        with pytest.raises(ValueError):
            pkg.Plan.griffin_lim(plan, bad, 3, 0.5)
    with pytest.raises(ValueError):
        pkg.Plan.gl_project(plan, spec, mag)
    with pytest.raises(ValueError):
        pkg.Plan.griffin_lim(plan, mag, 3, 1.0)
    with pytest.raises(ValueError):
        pkg.Plan.griffin_lim(plan, mag, -1, 0.5)


CPP_TU = r'''
#include "crlot_dsp.hpp"
void probe(crlot::StftEngine& e, const float* d_spec, const float* d_mag, float* d_out, float* d_y) {
    e.gl_project_device(d_spec, nullptr, d_mag, d_out, 3, 24, 0.99);
    e.gl_project_device(d_spec, d_spec, d_mag, d_out, 3, 24, 0.5, 24 * 1030, 1030, 24 * 520, 520);
    e.griffin_lim_device(d_mag, nullptr, d_y, 3, 24, 32, 0.99, 24 * 256);
    e.griffin_lim_device(d_mag, d_spec, d_y, 3, 24, 0, 0.0, 24 * 256);
}
'''


def test_cpp_methods_compile(tmp_path):
    src = tmp_path / "gl_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
