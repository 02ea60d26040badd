"""CPU tests of the cross-spectral estimator's host side (include/crlot_dsp.h,
"cross-spectral estimation"): every new symbol is declared, exported and bound; the new
kernel ids have their names; the launch struct matches the header; alpha is checked before
anything else, so every violation is CRLOT_EINVAL with no plan and no device; the null
arguments of every entry are refused; the per-bin arithmetic, the kernels' lanes and the
peak's lane-and-combine equal the plain loops on the CPU (tools/xspec_step_check.cpp); the
C++ mirror compiles.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"crlot_xspec_create": 4, "crlot_xspec_destroy": 1, "crlot_xspec_prepare": 1, "crlot_xspec_reset": 1,
               "crlot_xspec_info": 6, "crlot_xspec_state": 2, "crlot_xspec_last_launch": 2,
               "crlot_xspec_accumulate": 12, "crlot_xspec_derive": 11, "crlot_xspec_peak": 8,
               "crlot_xspec_estimate": 10, "crlot_xspec_delay": 8}
KERNELS = {57: ("CRLOT_K_XSPEC_ACC", "k_xspec_acc"), 58: ("CRLOT_K_XSPEC_DERIVE", "k_xspec_derive"),
           59: ("CRLOT_K_XSPEC_PEAK", "k_xspec_peak")}


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
    for kid in (41, 44, 46, 52):
        assert pkg.kernel_name(kid) == "unknown"
    for member in ("accumulate", "estimate", "derive", "coherence", "transfer", "weighted", "peak", "delay", "state",
                   "reset", "frames", "prepare", "last_launch", "close"):
        assert hasattr(pkg.CrossSpectrum, member), member


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


def test_launch_struct_matches_header(pkg):
    txt = open(pkg.HEADER_PATH).read()
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    want = [(n, ctypes_of[t] * k if k else ctypes_of[t]) for n, t, k in _header_fields(txt, "crlot_xspec_launch")]
    got = list(pkg.XspecLaunch._fields_)
    assert [n for n, _ in want] == [n for n, _ in got] == ["n_kernels", "kernel", "reserved", "grid"]
    for (_, a), (_, b) in zip(want, got):
        assert C.sizeof(a) == C.sizeof(b) and getattr(a, "_length_", 0) == getattr(b, "_length_", 0)
    assert C.sizeof(pkg.XspecLaunch) == 48 and pkg.XspecLaunch.grid.offset == 24


def test_alpha_is_checked_before_the_plan_and_any_device(pkg):
    L = pkg.lib()

    def err():
        return L.crlot_last_error().decode()

    xs = C.c_void_p()
    for alpha in (-0.1, -1e-300, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        # no plan at all: alpha's violation is what the call reports
        assert L.crlot_xspec_create(None, 2, alpha, C.byref(xs)) == pkg.EINVAL
        assert not xs and "alpha" in err(), (alpha, err())
        assert L.crlot_xspec_create(None, 2, alpha, None) == pkg.EINVAL and "alpha" in err()
    for alpha in (0.0, 0.5, 0.9, 0.999999, 1e-300):  # a good alpha gets as far as the missing plan
        assert L.crlot_xspec_create(None, 2, alpha, C.byref(xs)) == pkg.EINVAL
        assert not xs and "plan" in err(), (alpha, err())
    assert L.crlot_xspec_create(None, 2, 0.0, None) == pkg.EINVAL and "null" in err()


def test_null_arguments(pkg):
    L = pkg.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.crlot_xspec_prepare(None) == pkg.EINVAL
    assert L.crlot_xspec_reset(None) == pkg.EINVAL
    assert L.crlot_xspec_info(None, None, None, None, None, None) == pkg.EINVAL
    assert L.crlot_xspec_state(None, None) == pkg.EINVAL
    assert L.crlot_xspec_last_launch(None, None) == pkg.EINVAL
    assert L.crlot_xspec_accumulate(None, p, p, 1, 1, 2, 2, 2, 2, 0, p, None) == pkg.EINVAL
    assert L.crlot_xspec_derive(None, p, 1, 0, p, 1, p, 2, p, 2, None) == pkg.EINVAL
    assert L.crlot_xspec_peak(None, p, 8, 1, 1, p, 3, None) == pkg.EINVAL
    assert L.crlot_xspec_estimate(None, p, p, 1, 16, 16, 16, 0, p, None) == pkg.EINVAL
    assert L.crlot_xspec_delay(None, p, 1, 1, 1, p, 3, None) == pkg.EINVAL
    L.crlot_xspec_destroy(None)


def test_arithmetic_lanes_and_peak_equal_the_plain_loops_on_cpu(tmp_path):
    """tools/xspec_step_check.cpp: csrc/xspec_chain.h compiled for the host with exact-size
    buffers against plain loops: 63 / 64 / 65 / 129 bins, F = 1, 3, 4, 5, 26, both averaging
    modes, a shared reference, zero columns, padded rows with sentinels, a cut and carry at
    every frame; the peak's 64 lanes and butterfly against the serial scan."""
    exe = tmp_path / "xsc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "crlot-dsp_amd", "csrc"),
                        os.path.join(ROOT, "tools", "xspec_step_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(crlot::StftEngine& eng, const float* d_x, const float* d_spec, float* d_out, hipStream_t s) {
    crlot::CrossSpectrum xs(eng.plan(), 4, 0.9);
    crlot::CrossSpectrum other(eng.plan(), 2);
    xs = std::move(other);
    crlot::CrossSpectrum third(std::move(xs));
    third.prepare();
    third.accumulate_device(d_spec, d_spec, 2, 10, 0, 514, 10 * 514, 514, true, nullptr, s);
    third.estimate_device(d_x, d_x, 2, 4096, 0, 4096, false, d_out, s);
    third.derive_device(nullptr, 2, 1, d_out, 257, nullptr, 0, d_out + 1024, 514, s);
    third.peak_device(d_out, 512, 2, 255, d_out + 2048, 3, s);
    third.delay_device(nullptr, 2, 1, 255, d_out, 3, s);
    const crlot_xspec_launch r = third.last_launch();
    third.reset();
    return third.pairs() + third.bins() + third.frames() + r.grid[0] + r.kernel[2] + (third.state() != nullptr) +
           (third.get() != nullptr);
}
'''


def test_cpp_class_compiles(tmp_path):
    src = tmp_path / "xspec_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
