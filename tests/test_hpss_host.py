"""CPU tests of HPSS's host side (include/crlot_dsp.h, "HPSS"): the two symbols are
declared, exported and bound; the two kernel ids have their names; the descriptor
struct matches the header; the entries refuse bad descriptors and absent outputs
before any device is touched; the Python validators refuse each bad argument and
tensor; the sliding sorted window of the kernels equals a sort on the CPU; the
C++ mirror compiles.  No GPU compute here.  (Rejections that need a plan's frame
size -- short leading dimensions, overlaps at the C entry, a stored mask -- are in
tests/test_gpu_hpss.py::test_errors_and_empties.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["crlot_hpss_masks", "crlot_hpss"]


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
    assert len(L.crlot_hpss_masks.argtypes) == 14 and len(L.crlot_hpss.argtypes) == 11
    assert L.crlot_abi_version() == 2
    for kid, name in ((42, "k_hpss_freq"), (43, "k_hpss_time")):
        assert pkg.kernel_name(kid) == name
    assert pkg.kernel_name(44) == "unknown"
    assert callable(pkg.Plan.hpss_masks) and callable(pkg.Plan.hpss)
    txt = open(pkg.HEADER_PATH).read()
    assert "#define CRLOT_K_HPSS_FREQ 42" in txt and "#define CRLOT_K_HPSS_TIME 43" in txt
    assert "#define CRLOT_HPSS_HARD (-1)" in txt and pkg.HPSS_HARD == -1


def test_desc_layout_matches_header(pkg):
    """typedef struct { int32_t win_harm, win_perc, power; int32_t reserved; double
    margin_harm, margin_perc; } crlot_hpss_desc, field by field from the header."""
    txt = open(pkg.HEADER_PATH).read()
    m = re.search(r"typedef struct crlot_hpss_desc \{(.*?)\} crlot_hpss_desc;", txt, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(pkg.HpssDesc._fields_)
    D = pkg.HpssDesc
    assert C.sizeof(D) == 32
    assert [getattr(D, n).offset for n, _ in D._fields_] == [0, 4, 8, 12, 16, 24]


def test_entries_reject_before_device(pkg):
    """No plan exists here: a bad descriptor and absent outputs are refused ahead of
    the plan check, each with its own code and message; a good call then stops at
    the null plan."""
    L = pkg.lib()
    one = C.c_float()
    buf = C.addressof(one)

    def masks(desc, mh=buf, mp=buf):
        return L.crlot_hpss_masks(None, None if desc is None else C.byref(desc), None, mh, mp, 1, 4, 0, 0, 0, 0,
                                  0, 0, None)

    def hpss(desc, yh=buf, yp=buf):
        return L.crlot_hpss(None, None if desc is None else C.byref(desc), None, yh, yp, 1, 4096, 4096, 0, 0, None)

    def err():
        return L.crlot_last_error().decode()

    good = dict(win_harm=31, win_perc=31, power=2, reserved=0, margin_harm=1.0, margin_perc=1.0)
    cases = [(dict(win_harm=30), pkg.EINVAL, "odd"), (dict(win_perc=0), pkg.EINVAL, "odd"),
             (dict(win_harm=-3), pkg.EINVAL, "odd"), (dict(win_perc=65), pkg.EUNSUPPORTED, "above 63"),
             (dict(win_harm=64), pkg.EINVAL, "odd"), (dict(power=3), pkg.EUNSUPPORTED, "power"),
             (dict(power=0), pkg.EUNSUPPORTED, "power"), (dict(margin_harm=0.5), pkg.EINVAL, "margins"),
             (dict(margin_perc=float("nan")), pkg.EINVAL, "margins"),
             (dict(margin_perc=float("inf")), pkg.EINVAL, "margins")]
    for call in (masks, hpss):
        for change, code, word in cases:
            assert call(pkg.HpssDesc(**{**good, **change})) == code, change
            assert word in err(), (change, err())
        assert call(None) == pkg.EINVAL and "descriptor" in err()
        ok = pkg.HpssDesc(**good)
        assert call(ok, None, None) == pkg.EINVAL and "null" in err() and "plan" not in err()
        assert call(ok) == pkg.EINVAL and "null plan" in err()
        for power in (1, 2, pkg.HPSS_HARD):  # every supported power reaches the plan check
            assert call(pkg.HpssDesc(**{**good, "power": power, "win_harm": 63, "win_perc": 1})) == pkg.EINVAL
            assert "null plan" in err()


def test_hpss_desc_from_python_arguments(pkg):
    def fields(d):
        return (d.win_harm, d.win_perc, d.power, d.reserved, d.margin_harm, d.margin_perc)
    assert fields(pkg._hpss_desc()) == (31, 31, 2, 0, 1.0, 1.0)
    assert fields(pkg._hpss_desc((17, 63), 1, (2.0, 3.7))) == (17, 63, 1, 0, 2.0, 3.7)
    assert fields(pkg._hpss_desc(1, float("inf"), 1)) == (1, 1, pkg.HPSS_HARD, 0, 1.0, 1.0)
    assert fields(pkg._hpss_desc([3, 5], 2.0, [1, 2])) == (3, 5, 2, 0, 1.0, 2.0)
    for bad in (30, 0, -1, 65, 31.5, (31, 32), (31, 31, 31), True):
        with pytest.raises(ValueError):
            pkg._hpss_desc(bad)
    for bad in (0, 3, 1.5, -2, float("nan")):
        with pytest.raises(ValueError):
            pkg._hpss_desc(31, bad)
    for bad in (0.99, float("nan"), float("inf"), (1.0, 0.5), (1.0,)):
        with pytest.raises(ValueError):
            pkg._hpss_desc(31, 2, bad)


def _plan(pkg):
    plan = object.__new__(pkg.Plan)
    plan.frame_size, plan.hop_size = 1024, 256
    plan.cfg = pkg.PlanConfig(device=0)
    return plan


def test_torch_front_refuses_before_any_call(pkg):
    """Host tensors, wrong dtypes and wrong shapes never reach the library (the plan
    here has no handle: reaching it would raise AttributeError, not ValueError)."""
    import torch
    plan = _plan(pkg)
    spec = torch.zeros(2, 8, 513, dtype=torch.complex64)
    for bad in (spec, torch.zeros(2, 8, 513), torch.zeros(2, 8, 512, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            pkg.Plan.hpss_masks(plan, bad)
    for kw in (dict(kernel_size=30), dict(power=3), dict(margin=0.5), dict(mask_h=False, mask_p=False)):
        with pytest.raises(ValueError):
            pkg.Plan.hpss_masks(plan, spec, **kw)
    x = torch.zeros(2, 4096)
    for bad in (x, x.double(), torch.zeros(2, 3, 4096)):
        with pytest.raises(ValueError):
            pkg.Plan.hpss(plan, bad)
    for kw in (dict(kernel_size=(31, 64)), dict(power=0), dict(margin=(1, float("nan"))),
               dict(y_h=False, y_p=False)):
        with pytest.raises(ValueError):
            pkg.Plan.hpss(plan, x, **kw)


def test_tensors_overlap(pkg):
    import torch
    base = torch.zeros(64)
    a, b, c = base[:32], base[32:], base[31:40]
    assert not pkg._tensors_overlap(a, b)
    assert pkg._tensors_overlap(a, c) and pkg._tensors_overlap(c, b) and pkg._tensors_overlap(base, a)
    assert not pkg._tensors_overlap(a, base[:0])
    rows = base.view(8, 8)
    assert pkg._tensors_overlap(rows[:, :4], rows[:, 4:])  # interleaved rows: the address ranges intersect
    assert not pkg._tensors_overlap(rows[:4], rows[4:])


def test_sorted_window_equals_sort_on_cpu(tmp_path):
    """tools/hpss_window_check.cpp: the kernels' window (csrc/hpss_window.h) compiled
    for the host, against std::sort, for every capacity and odd window."""
    exe = tmp_path / "hwc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "crlot-dsp_amd", "csrc"),
                        os.path.join(ROOT, "tools", "hpss_window_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]


CPP_TU = r'''
#include "crlot_dsp.hpp"
void probe(crlot::StftEngine& e, const float* d_spec, const float* d_x, float* a, float* b) {
    crlot_hpss_desc d{31, 31, 2, 0, 1.0, 1.0};
    e.hpss_masks_device(d, d_spec, a, b, 3, 24);
    e.hpss_masks_device(d, d_spec, nullptr, b, 3, 24, 24 * 1030, 1030, 24 * 520, 520);
    d.power = CRLOT_HPSS_HARD;
    e.hpss_device(d, d_x, a, b, 3, 24 * 256, 24 * 256, 24 * 256);
    e.hpss_device(d, d_x, a, nullptr, 3, 24 * 256, 24 * 256, 24 * 256);
}
'''


def test_cpp_methods_compile(tmp_path):
    src = tmp_path / "hpss_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
