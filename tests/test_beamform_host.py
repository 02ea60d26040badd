"""CPU tests of the beamformer's host side (include/crlot_dsp.h, "beamformer"): every new
symbol is declared, exported and bound with its argument count; the new kernel ids have
their names and the unassigned ones stay "unknown"; the descriptor and launch structs match
the header; the descriptor is checked before anything else, so every violation is
CRLOT_EINVAL with no plan and no device; the null arguments of every entry are refused;
the per-bin arithmetic and the four kernels' lanes equal plain loops on the CPU
(tools/bf_step_check.cpp); the Python layout checks and the steering helper; the C++
mirror compiles.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beamform_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"crlot_beamform_desc_default": 1, "crlot_beamformer_create": 4, "crlot_beamformer_destroy": 1,
               "crlot_beamformer_prepare": 1, "crlot_beamformer_reset": 1, "crlot_beamformer_info": 8,
               "crlot_beamformer_state": 2, "crlot_beamformer_weights": 2, "crlot_beamformer_steering": 2,
               "crlot_beamformer_last_launch": 2, "crlot_beamform_accumulate": 13, "crlot_beamform_solve": 6,
               "crlot_beamform_apply": 11, "crlot_beamform": 11, "crlot_stream_beamform_hop": 9}
KERNELS = {60: ("CRLOT_K_BF_ACC", "k_bf_acc"), 61: ("CRLOT_K_BF_SOLVE", "k_bf_solve"),
           62: ("CRLOT_K_BF_APPLY", "k_bf_apply"), 63: ("CRLOT_K_BF_HOP", "k_bf_hop")}


def test_new_symbols_declared_exported_and_bound(pkg):
    L = pkg.lib()
    syms = pkg.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\b(crlot_[a-z0-9_]+)\b", out))
    txt = open(pkg.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in NEW_SYMBOLS.items():
        assert name in syms, name
        assert name in exported, name
        assert len(getattr(L, name).argtypes) == nargs, name
        decl = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", code, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert L.crlot_abi_version() == 2
    for kid, (macro, name) in KERNELS.items():
        assert pkg.kernel_name(kid) == name
        assert re.search(rf"#define {macro} {kid}\b", txt), macro
    assert "#define CRLOT_ABI_VERSION 2" in txt
    for kid in (41, 44, 46, 52):
        assert pkg.kernel_name(kid) == "unknown"
    for member in ("accumulate", "solve", "apply", "beamform", "hop", "state", "weights", "steering", "set_weights",
                   "set_steering", "reset", "frames", "prepare", "last_launch", "close"):
        assert hasattr(pkg.Beamformer, member), member
    assert callable(pkg.steering_from_delays)


def _header_fields(txt, name):
    m = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", txt, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            for n in names.split(","):
                arr = re.match(r"(\w+)\[(\d+)\]", n.strip())
                fields.append((arr.group(1), ctype, int(arr.group(2))) if arr else (n.strip(), ctype, 0))
    return fields


def test_structs_match_header(pkg):
    txt = open(pkg.HEADER_PATH).read()
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for name, cls, names in (("crlot_beamform_launch", pkg.BeamformLaunch, ["n_kernels", "kernel", "reserved", "grid"]),
                             ("crlot_beamform_desc", pkg.BeamformDesc,
                              ["mics", "ref", "mode", "update_every", "alpha", "loading"])):
        want = [(n, ctypes_of[t] * k if k else ctypes_of[t]) for n, t, k in _header_fields(txt, name)]
        got = list(cls._fields_)
        assert [n for n, _ in want] == [n for n, _ in got] == names
        for (_, a), (_, b) in zip(want, got):
            assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", 0) == getattr(b, "_length_", 0)
    assert C.sizeof(pkg.BeamformLaunch) == 48 and pkg.BeamformLaunch.grid.offset == 24
    assert C.sizeof(pkg.BeamformDesc) == 32 and pkg.BeamformDesc.alpha.offset == 16
    d = pkg.BeamformDesc()
    assert pkg.lib().crlot_beamform_desc_default(C.byref(d)) == 0
    assert (d.mics, d.ref, d.mode, d.update_every, d.alpha, d.loading) == (2, 0, 0, 1, 0.0, 1e-3)
    assert re.search(r"#define CRLOT_BF_SOUDEN 0\b", txt) and re.search(r"#define CRLOT_BF_STEERED 1\b", txt)
    assert (pkg.BF_SOUDEN, pkg.BF_STEERED) == (0, 1)


def test_descriptor_is_checked_before_the_plan_and_any_device(pkg):
    L = pkg.lib()

    def err():
        return L.crlot_last_error().decode()

    def desc(**kw):
        d = pkg.BeamformDesc()
        assert L.crlot_beamform_desc_default(C.byref(d)) == 0
        d.mics = 4
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    nan, inf = float("nan"), float("inf")
    bad = [("mics", 1), ("mics", 0), ("mics", -3), ("mics", 9), ("ref", -1), ("ref", 4), ("mode", 2), ("mode", -1),
           ("update_every", 0), ("update_every", -5), ("alpha", -0.1), ("alpha", 1.0), ("alpha", 1.5), ("alpha", nan),
           ("alpha", inf), ("alpha", -inf), ("loading", -1e-9), ("loading", nan), ("loading", inf)]
    h = C.c_void_p()
    for field, value in bad:
        d = desc(**{field: value})
        # no plan at all: the descriptor's violation is what the call reports
        assert L.crlot_beamformer_create(None, C.byref(d), 1, C.byref(h)) == pkg.EINVAL, (field, value)
        assert not h and field in err(), (field, value, err())
        assert L.crlot_beamformer_create(None, C.byref(d), 1, None) == pkg.EINVAL and field in err()
    assert L.crlot_beamformer_create(None, None, 1, C.byref(h)) == pkg.EINVAL and "descriptor" in err()
    for good in (desc(), desc(mics=2), desc(mics=8, ref=7), desc(mode=1), desc(alpha=0.999999), desc(loading=0.0),
                 desc(update_every=1000)):  # a good descriptor gets as far as the missing plan
        assert L.crlot_beamformer_create(None, C.byref(good), 1, C.byref(h)) == pkg.EINVAL
        assert not h and "plan" in err(), err()
    assert L.crlot_beamformer_create(None, C.byref(desc()), 1, None) == pkg.EINVAL and "null" in err()
    assert L.crlot_beamform_desc_default(None) == pkg.EINVAL


def test_null_arguments(pkg):
    L = pkg.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    em = C.c_int32(5)
    assert L.crlot_beamformer_prepare(None) == pkg.EINVAL
    assert L.crlot_beamformer_reset(None) == pkg.EINVAL
    assert L.crlot_beamformer_info(None, None, None, None, None, None, None, None) == pkg.EINVAL
    assert L.crlot_beamformer_state(None, None) == pkg.EINVAL
    assert L.crlot_beamformer_weights(None, None) == pkg.EINVAL
    assert L.crlot_beamformer_steering(None, None) == pkg.EINVAL
    assert L.crlot_beamformer_last_launch(None, None) == pkg.EINVAL
    assert L.crlot_beamform_accumulate(None, p, 2, 2, p, 0, 1, 1, 1, 0, 0, p, None) == pkg.EINVAL
    assert L.crlot_beamform_solve(None, p, p, 1, p, None) == pkg.EINVAL
    assert L.crlot_beamform_apply(None, p, 2, 2, p, 1, 1, p, 2, 2, None) == pkg.EINVAL
    assert L.crlot_beamform(None, p, 16, p, 0, 1, p, 16, 1, 16, None) == pkg.EINVAL
    assert L.crlot_stream_beamform_hop(None, None, None, p, p, 0, p, C.byref(em), None) == pkg.EINVAL
    assert em.value == 0
    L.crlot_beamformer_destroy(None)


def test_arithmetic_and_lanes_equal_the_plain_loops_on_cpu(tmp_path):
    """tools/bf_step_check.cpp: csrc/beamform_chain.h compiled for the host with exact-size
    buffers against plain loops on full complex matrices: M = 2 .. 8; 63 / 64 / 65 / 129 bins;
    F = 1, 3, 4, 5, 26; both averaging modes; the three targets; a shared mask; a group of
    zeros; padded rows with sentinels; a cut and carry at every frame; both solve modes and
    every ref; the apply in chunks; the hop lane against its three-call sequence."""
    exe = tmp_path / "bfc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "crlot-dsp_amd", "csrc"),
                        os.path.join(ROOT, "tools", "bf_step_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]


def test_layout_checks_and_the_steering_helper(pkg):
    M, bins = 3, 9
    ok = pkg._bf_spec_layout((2, M, 5, bins), (M * 60, 60, 12, 1), "complex64", 0, 0, M, bins)
    assert ok == (2, 5, 120, 24)
    assert pkg._bf_spec_layout((1, M, 1, bins), (0, bins, 0, 1), "complex64", 0, 0, M, bins) == (1, 1, 2 * bins, 2 * bins)
    for shape, strides, dtype, dev in (((2, M, 5, bins), (M * 60 + 1, 60, 12, 1), "complex64", 0),  # groups not M rows apart
                                       ((2, M, 5, bins), (M * 60, 60, 8, 1), "complex64", 0),       # frames overlap
                                       ((2, M, 5, bins), (M * 40, 40, 12, 1), "complex64", 0),      # microphones overlap
                                       ((2, M, 5, bins), (M * 60, 60, 12, 2), "complex64", 0),      # strided rows
                                       ((2, M + 1, 5, bins), (240, 60, 12, 1), "complex64", 0),     # wrong M
                                       ((2, M, 5, bins + 1), (180, 60, 12, 1), "complex64", 0),     # wrong bins
                                       ((2, M, 5, bins), (180, 60, 12, 1), "complex128", 0),
                                       ((2, M, 5, bins), (180, 60, 12, 1), "complex64", None),
                                       ((2, M, 5, bins), (180, 60, 12, 1), "complex64", 1)):
        with pytest.raises(ValueError):
            pkg._bf_spec_layout(shape, strides, dtype, dev, 0, M, bins)
    assert pkg._bf_mask_layout((2, 5, bins), (50, 10, 1), "float32", 0, 0, 2, 5, bins) == (50, 10)
    assert pkg._bf_mask_layout((5, bins), (10, 1), "float32", 0, 0, 2, 5, bins) == (0, 10)
    assert pkg._bf_mask_layout((2, 5, bins), (0, 10, 1), "float32", 0, 0, 2, 5, bins) == (0, 10)
    for shape, strides, dtype, dev in (((2, 5, bins), (40, 10, 1), "float32", 0), ((2, 5, bins), (50, 8, 1), "float32", 0),
                                       ((3, 5, bins), (50, 10, 1), "float32", 0), ((2, 5, bins), (50, 10, 1), "float64", 0),
                                       ((2, 5, bins), (50, 10, 1), "float32", None), ((5, bins), (10, 2), "float32", 0)):
        with pytest.raises(ValueError):
            pkg._bf_mask_layout(shape, strides, dtype, dev, 0, 2, 5, bins)
    d = pkg.steering_from_delays([[0.0, 1.0, -2.5]], 16)
    assert d.shape == (1, 3, 9) and d.dtype == np.complex64
    assert np.array_equal(d, R.steering_from_delays([[0.0, 1.0, -2.5]], 16))
    assert np.all(d[0, 0] == 1) and abs(d[0, 1, 4] - (-1j)) < 1e-7 and abs(d[0, 1, 8] + 1) < 1e-7
    want = np.exp(-2j * np.pi * np.arange(9) * -2.5 / 16)
    assert np.abs(d[0, 2] - want).max() <= 2.0 ** -23
    for bad in (([0.0], 15), ([0.0], 0), ([float("nan")], 16)):
        with pytest.raises(ValueError):
            pkg.steering_from_delays(*bad)


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(crlot::StftEngine& eng, crlot_stream* a, crlot_stream* b, const float* d_x, const float* d_spec,
              const float* d_mask, float* d_out, hipStream_t s) {
    crlot::Beamformer bf(eng.plan(), 4, 2, 1, CRLOT_BF_STEERED, 0.9, 1e-3, 3);
    crlot::Beamformer other(eng.plan(), 2);
    bf = std::move(other);
    crlot::Beamformer third(std::move(bf));
    crlot_beamform_desc d{};
    crlot_beamform_desc_default(&d);
    crlot::Beamformer fourth(eng.plan(), d, 3);
    third.prepare();
    third.accumulate_device(d_spec, 10 * 514, 514, d_mask, 0, 257, 1, 10, 0, true, nullptr, s);
    third.solve_device(nullptr, nullptr, 1, nullptr, s);
    third.apply_device(d_spec, 10 * 514, 514, nullptr, 1, 10, d_out, 10 * 514, 514, s);
    third.beamform_device(d_x, 4096, d_mask, 0, 257, d_out, 4096, 1, 4096, s);
    const int emitted = third.hop_device(a, b, d_x, d_mask, 0, d_out, s);
    const crlot_beamform_launch r = third.last_launch();
    third.reset();
    return third.groups() + third.mics() + third.bins() + third.frames() + r.grid[0] + r.kernel[2] + emitted +
           (third.state() != nullptr) + (third.weights() != nullptr) + (third.steering() != nullptr) +
           (third.get() != nullptr) + fourth.groups();
}
'''


def test_cpp_class_compiles(tmp_path):
    src = tmp_path / "bf_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
