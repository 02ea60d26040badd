"""CPU tests of the noise suppressor's host side (include/crlot_dsp.h, "noise suppressor"):
every new symbol is declared, exported and bound; the new kernel ids have their names;
the descriptor and launch structs match the header; the descriptor is checked before
anything else, so every violation is CRLOT_EINVAL with no plan and no device; the null
arguments of every entry are refused; the per-bin step and the gains kernel's lane equal
the plain loop on the CPU (tools/denoise_step_check.cpp); the C++ mirror compiles.  No
GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"crlot_denoise_desc_default": 1, "crlot_denoiser_create": 4, "crlot_denoiser_destroy": 1,
               "crlot_denoiser_prepare": 1, "crlot_denoiser_reset": 1, "crlot_denoiser_info": 6,
               "crlot_denoiser_state": 2, "crlot_denoiser_set_route": 2, "crlot_denoiser_last_launch": 2,
               "crlot_denoise_gains": 11, "crlot_denoise": 8, "crlot_stream_denoise_hop": 6}
KERNELS = {53: ("CRLOT_K_DENOISE_GAINS", "k_denoise_gains"), 54: ("CRLOT_K_DENOISE_HOP", "k_stream_denoise"),
           55: ("CRLOT_K_STREAM_STFT", "k_stream_stft"), 56: ("CRLOT_K_STREAM_ISTFT", "k_stream_istft")}


def test_new_symbols_declared_exported_and_bound(pkg):
    L = pkg.lib()
    syms = pkg.header_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\b(crlot_[a-z0-9_]+)\b", out))
    for name, nargs in NEW_SYMBOLS.items():
        assert name in syms, name
        assert name in exported, name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert L.crlot_abi_version() == 2
    txt = open(pkg.HEADER_PATH).read()
    for kid, (macro, name) in KERNELS.items():
        assert pkg.kernel_name(kid) == name
        assert re.search(rf"#define {macro} {kid}\b", txt), macro
    assert "#define CRLOT_ABI_VERSION 2" in txt
    for kid in (41, 44, 46):
        assert pkg.kernel_name(kid) == "unknown"
    for member in ("gains", "denoise", "state", "reset", "set_route", "last_launch", "prepare", "frames", "close"):
        assert hasattr(pkg.Denoiser, member), member
    assert hasattr(pkg.Stream, "denoise_hop")


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
    for name, cls, size in (("crlot_denoise_desc", pkg.DenoiseDesc, 56), ("crlot_denoise_launch", pkg.DenoiseLaunch, 48)):
        want = [(n, ctypes_of[t] * k if k else ctypes_of[t]) for n, t, k in _header_fields(txt, name)]
        got = list(cls._fields_)
        assert [n for n, _ in want] == [n for n, _ in got], name
        for (_, a), (_, b) in zip(want, got):
            assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", 0) == getattr(b, "_length_", 0), name
        assert C.sizeof(cls) == size, name


def test_defaults(pkg):
    L = pkg.lib()
    d = pkg.DenoiseDesc()
    assert L.crlot_denoise_desc_default(C.byref(d)) == pkg.OK
    assert (d.alpha_s, d.alpha_p, d.alpha_d, d.delta, d.window, d.alpha_dd, d.g_min) == (0.8, 0.2, 0.95, 5.0, 64, 0.98, 0.1)
    assert L.crlot_denoise_desc_default(None) == pkg.EINVAL
    py = pkg.denoise_desc()
    assert all(getattr(py, k) == getattr(d, k) for k, _ in pkg.DenoiseDesc._fields_)
    with pytest.raises(ValueError):
        pkg.denoise_desc(alpha=0.5)


def test_descriptor_is_checked_before_the_plan_and_any_device(pkg):
    L = pkg.lib()

    def err():
        return L.crlot_last_error().decode()

    dn = C.c_void_p()
    nan, inf = float("nan"), float("inf")
    bad = [("alpha_s", v) for v in (-0.1, 1.0, 1.5, nan, inf)] + [("alpha_p", v) for v in (-1e-9, 1.0, nan)] + \
          [("alpha_d", v) for v in (-0.5, 1.0, nan)] + [("alpha_dd", v) for v in (-0.5, 1.0, inf)] + \
          [("delta", v) for v in (0.0, -1.0, nan, inf)] + [("g_min", v) for v in (-0.01, 1.01, nan)] + \
          [("window", v) for v in (0, -3)]
    for field, v in bad:
        # no plan at all: the descriptor's violation is what the call reports
        assert L.crlot_denoiser_create(None, C.byref(pkg.denoise_desc(**{field: v})), 2, C.byref(dn)) == pkg.EINVAL
        assert not dn and field in err(), (field, v, err())
    ok = [dict(), dict(alpha_s=0.0, alpha_p=0.0, alpha_d=0.0, alpha_dd=0.0), dict(g_min=0.0), dict(g_min=1.0),
          dict(window=1), dict(delta=1e-30), dict(alpha_s=0.999999)]
    for kw in ok:  # a good descriptor gets as far as the missing plan
        assert L.crlot_denoiser_create(None, C.byref(pkg.denoise_desc(**kw)), 2, C.byref(dn)) == pkg.EINVAL
        assert not dn and "plan" in err(), (kw, err())
    assert L.crlot_denoiser_create(None, None, 2, C.byref(dn)) == pkg.EINVAL and "descriptor" in err()
    assert L.crlot_denoiser_create(None, C.byref(pkg.denoise_desc()), 2, None) == pkg.EINVAL and "null" in err()


def test_null_arguments(pkg):
    L = pkg.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.crlot_denoiser_prepare(None) == pkg.EINVAL
    assert L.crlot_denoiser_reset(None) == pkg.EINVAL
    assert L.crlot_denoiser_info(None, None, None, None, None, None) == pkg.EINVAL
    assert L.crlot_denoiser_state(None, None) == pkg.EINVAL
    assert L.crlot_denoiser_set_route(None, 0) == pkg.EINVAL
    assert L.crlot_denoiser_last_launch(None, None) == pkg.EINVAL
    assert L.crlot_denoise_gains(None, p, p, 1, 1, 2, 2, 1, 1, 0, None) == pkg.EINVAL
    assert L.crlot_denoise(None, p, p, 1, 16, 16, 16, None) == pkg.EINVAL
    em = C.c_int32(7)
    assert L.crlot_stream_denoise_hop(None, None, p, p, C.byref(em), None) == pkg.EINVAL and em.value == 0
    L.crlot_denoiser_destroy(None)


def test_step_and_lane_equal_the_plain_loop_on_cpu(tmp_path):
    """tools/denoise_step_check.cpp: csrc/denoise_chain.h compiled for the host with exact-size
    buffers against a plain loop over (stream, bin, frame): L = 1, 2, 8 through several
    resets, 63 / 64 / 65 / 129 bins, zero columns, a cut and carry at every frame."""
    exe = tmp_path / "dsc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "crlot-dsp_amd", "csrc"),
                        os.path.join(ROOT, "tools", "denoise_step_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(crlot::StftEngine& eng, const float* d_x, float* d_y, const float* d_spec, float* d_mask, hipStream_t s) {
    crlot_denoise_desc d = crlot::Denoiser::defaults();
    d.window = 62;
    crlot::Denoiser dn(eng.plan(), 4, d);
    crlot::Denoiser other(eng.plan(), 2);
    dn = std::move(other);
    dn.prepare();
    dn.set_route(2);
    dn.gains_device(d_spec, d_mask, 2, 10, 10 * 514, 514, 10 * 257, 257, true, s);
    dn.denoise_device(d_x, d_y, 2, 4096, 4096, 4096, s);
    crlot::SpectralStream st(eng, 2);
    const size_t em = st.denoise_hop(dn, d_x, d_y, s);
    const crlot_denoise_launch r = dn.last_launch();
    dn.reset();
    return dn.channels() + dn.bins() + dn.frames() + r.grid[0] + r.kernel[2] + int64_t(em) + (dn.state() != nullptr) +
           (dn.get() != nullptr);
}
'''


def test_cpp_class_compiles(tmp_path):
    src = tmp_path / "denoise_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
