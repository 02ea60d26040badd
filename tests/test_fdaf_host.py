"""CPU tests of the adaptive filter's host side (include/crlot_dsp.h, "adaptive filter"):
every new symbol is declared, exported and bound; kernel ids 49 - 51 have their names;
crlot_fdaf_launch matches the header; crlot_fdaf_create needs no device and refuses each
bad argument and every block outside 128 / 256 / 512 / 1024; the setters refuse what the
header says they refuse; the state size is right; the update lane equals the plain
loop on the CPU (tools/fdaf_update_check.cpp); the C++ mirror compiles.  No GPU compute
here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"crlot_fdaf_create": 4, "crlot_fdaf_destroy": 1, "crlot_fdaf_prepare": 1, "crlot_fdaf_state_bytes": 1,
               "crlot_fdaf_reset": 1, "crlot_fdaf_set_layout": 2, "crlot_fdaf_info": 6, "crlot_fdaf_last_launch": 2,
               "crlot_fdaf_set_step": 4, "crlot_fdaf_set_constraint": 2, "crlot_fdaf_set_adapt": 2,
               "crlot_fdaf_set_taps": 4, "crlot_fdaf_get_taps": 3, "crlot_fdaf_state": 7, "crlot_fdaf_hop": 6,
               "crlot_fdaf_constrain": 3}


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
    assert [pkg.kernel_name(i) for i in (49, 50, 51)] == ["k_fdaf_hop", "k_fdaf_update", "k_fdaf_constrain"]
    assert pkg.kernel_name(52) == "unknown"
    txt = open(pkg.HEADER_PATH).read()
    for line in ("#define CRLOT_K_FDAF_HOP 49", "#define CRLOT_K_FDAF_UPDATE 50", "#define CRLOT_K_FDAF_CONSTRAIN 51",
                 "#define CRLOT_ABI_VERSION 2"):
        assert line in txt, line
    for member in ("push", "taps", "set_taps", "state", "reset", "prepare", "set_step", "set_constraint", "set_adapt",
                   "constrain", "last_launch", "state_bytes", "hops", "close"):
        assert hasattr(pkg.AdaptiveFilter, member), member


def test_launch_struct_matches_header(pkg):
    txt = open(pkg.HEADER_PATH).read()
    m = re.search(r"typedef struct crlot_fdaf_launch \{(.*?)\} crlot_fdaf_launch;", txt, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(pkg.FdafLaunch._fields_)
    assert C.sizeof(pkg.FdafLaunch) == 40


def test_create_and_setters_without_a_device(pkg):
    L = pkg.lib()

    def err():
        return L.crlot_last_error().decode()

    af = C.c_void_p()
    assert L.crlot_fdaf_create(128, 300, 2, None) == pkg.EINVAL and "null" in err()
    # a block no plan accepts, taps and channels out of range
    for block in (0, -128, 8193, 16384):
        assert L.crlot_fdaf_create(block, 300, 2, C.byref(af)) == pkg.EINVAL and not af and "block" in err(), block
    for taps in (0, -1, (1 << 20) + 1):
        assert L.crlot_fdaf_create(128, taps, 2, C.byref(af)) == pkg.EINVAL and not af and "taps" in err(), taps
    for channels in (0, -1):
        assert L.crlot_fdaf_create(128, 300, channels, C.byref(af)) == pkg.EINVAL and not af and "channels" in err()
    # blocks a plan accepts and the hop kernel has no instantiation for
    for block in (2048, 120, 4096):
        assert L.crlot_fdaf_create(block, 300, 2, C.byref(af)) == pkg.EUNSUPPORTED and not af, block
        assert all(size in err() for size in ("128", "256", "512", "1024")), err()
    assert L.crlot_fdaf_create(128, 1 << 20, 1, C.byref(af)) == pkg.OK and af
    L.crlot_fdaf_destroy(af)
    assert L.crlot_fdaf_create(128, 300, 2, C.byref(af)) == pkg.OK and af
    ch, b, k, p, hops = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32(), C.c_int64(-1)
    assert L.crlot_fdaf_info(af, C.byref(ch), C.byref(b), C.byref(k), C.byref(p), C.byref(hops)) == pkg.OK
    assert (ch.value, b.value, k.value, p.value, hops.value) == (2, 128, 300, 3, 0)
    assert L.crlot_fdaf_info(af, None, None, None, None, None) == pkg.OK
    assert L.crlot_fdaf_info(None, None, None, None, None, None) == pkg.EINVAL
    rec = pkg.FdafLaunch(9, 9, 9, 9, 9, 9, 9)
    assert L.crlot_fdaf_last_launch(af, C.byref(rec)) == pkg.OK
    assert [getattr(rec, n) for n, _ in pkg.FdafLaunch._fields_] == [0] * 7
    assert L.crlot_fdaf_last_launch(af, None) == pkg.EINVAL and L.crlot_fdaf_last_launch(None, C.byref(rec)) == pkg.EINVAL
    nan, inf = float("nan"), float("inf")
    for mu, lam, delta in ((-0.1, 0.9, 1e-3), (2.1, 0.9, 1e-3), (nan, 0.9, 1e-3), (inf, 0.9, 1e-3),
                           (0.5, -0.1, 1e-3), (0.5, 1.0, 1e-3), (0.5, nan, 1e-3),
                           (0.5, 0.9, 0.0), (0.5, 0.9, -1.0), (0.5, 0.9, inf), (0.5, 0.9, nan)):
        assert L.crlot_fdaf_set_step(af, mu, lam, delta) == pkg.EINVAL, (mu, lam, delta)
    for mu, lam, delta in ((0.0, 0.0, 1e-30), (2.0, 0.999, 10.0), (0.5, 0.9, 1e-3)):
        assert L.crlot_fdaf_set_step(af, mu, lam, delta) == pkg.OK, (mu, lam, delta)
    assert L.crlot_fdaf_set_step(None, 0.5, 0.9, 1e-3) == pkg.EINVAL
    for bad in (-1, 3):
        assert L.crlot_fdaf_set_constraint(af, bad) == pkg.EINVAL and "constraint" in err()
    for ok in (0, 2, 1):
        assert L.crlot_fdaf_set_constraint(af, ok) == pkg.OK
    assert L.crlot_fdaf_set_constraint(None, 1) == pkg.EINVAL
    assert L.crlot_fdaf_set_adapt(af, 0) == pkg.OK and L.crlot_fdaf_set_adapt(af, 1) == pkg.OK
    assert L.crlot_fdaf_set_adapt(None, 1) == pkg.EINVAL
    assert L.crlot_fdaf_set_layout(af, 1) == pkg.OK and L.crlot_fdaf_set_layout(None, 1) == pkg.EINVAL
    # nothing to reset: no device is touched
    assert L.crlot_fdaf_reset(af) == pkg.OK and L.crlot_fdaf_reset(None) == pkg.EINVAL
    # the argument checks of the taps, a hop and the constraint come before any device work
    taps = (C.c_float * 600)()
    assert L.crlot_fdaf_set_taps(None, taps, 1, 300) == pkg.EINVAL
    assert L.crlot_fdaf_set_taps(af, None, 1, 300) == pkg.EINVAL and "null" in err()
    for n_rows in (0, 3):
        assert L.crlot_fdaf_set_taps(af, taps, n_rows, 300) == pkg.EINVAL and "n_rows" in err()
    assert L.crlot_fdaf_set_taps(af, taps, 2, 299) == pkg.EINVAL and "ld" in err()
    taps[450] = float("inf")
    assert L.crlot_fdaf_set_taps(af, taps, 2, 300) == pkg.EINVAL and "finite" in err()
    assert L.crlot_fdaf_get_taps(None, taps, 300) == pkg.EINVAL
    assert L.crlot_fdaf_get_taps(af, None, 300) == pkg.EINVAL and L.crlot_fdaf_get_taps(af, taps, 299) == pkg.EINVAL
    blocks = (C.c_float * (4 * 256))()
    x = C.addressof(blocks)
    d, e, y = x + 4 * 256, x + 8 * 256, x + 12 * 256
    assert L.crlot_fdaf_hop(None, x, d, e, y, None) == pkg.EINVAL
    assert L.crlot_fdaf_hop(af, x, None, e, y, None) == pkg.EINVAL and "null" in err()
    assert L.crlot_fdaf_hop(af, x, d, None, y, None) == pkg.EINVAL and "null" in err()
    for args in ((x, d, x, y), (x, d, d, y), (x, d, e, x), (x, d, e, d), (x, d, e, e), (x, d, d + 4 * 255, None),
                 (None, d, e, e + 4)):
        assert L.crlot_fdaf_hop(af, *args, None) == pkg.EINVAL and "overlap" in err(), args
    for p in (-2, 3):
        assert L.crlot_fdaf_constrain(af, p, None) == pkg.EINVAL and "partition" in err()
    assert L.crlot_fdaf_constrain(None, 0, None) == pkg.EINVAL
    assert L.crlot_fdaf_prepare(None) == pkg.EINVAL
    assert L.crlot_fdaf_state(None, None, None, None, None, None, None) == pkg.EINVAL
    L.crlot_fdaf_destroy(af)
    L.crlot_fdaf_destroy(None)


@pytest.mark.parametrize("block,K,channels", [(128, 1, 1), (256, 48000, 1024), (512, 3 * 512 + 1, 7), (1024, 1025, 2)])
def test_state_bytes(pkg, block, K, channels):
    """Per channel the ring and W [P][N+2], E and G [N+2], prev [B] and pw [B+1], floats."""
    L = pkg.lib()
    af = C.c_void_p()
    assert L.crlot_fdaf_create(block, K, channels, C.byref(af)) == pkg.OK
    P, row = -(-K // block), 2 * block + 2
    assert L.crlot_fdaf_state_bytes(af) == 4 * channels * (2 * P * row + 2 * row + block + block + 1)
    assert L.crlot_fdaf_state_bytes(None) == pkg.EINVAL
    L.crlot_fdaf_destroy(af)


def test_python_object_on_the_host(pkg):
    af = pkg.AdaptiveFilter(256, 1000, 3, interleaved=True)
    assert (af.channels, af.block, af.partitions, af.taps_count, af.hops, af.interleaved) == (3, 256, 4, 1000, 0, True)
    assert af.state_bytes == 4 * 3 * (2 * 4 * 514 + 2 * 514 + 256 + 257)
    rec = af.last_launch()
    assert rec["kernels"] == [] and rec["names"] == [] and rec["hop_grid"] == 0
    af.set_step(1.0, 0.95, 1e-2)
    af.set_constraint(2)
    af.set_adapt(False)
    for call in (lambda: af.set_step(3.0), lambda: af.set_step(0.5, 1.0), lambda: af.set_step(0.5, 0.9, 0.0),
                 lambda: af.set_constraint(3)):
        with pytest.raises(ValueError):
            call()
    af.reset()
    af.close()
    af.close()
    with pytest.raises(ValueError):
        pkg.AdaptiveFilter(256, 1000, 0)
    with pytest.raises(ValueError):
        pkg.AdaptiveFilter(256, 0, 2)
    with pytest.raises(NotImplementedError):
        pkg.AdaptiveFilter(2048, 1000, 2)


def test_update_lane_equals_the_plain_loop_on_cpu(tmp_path):
    """tools/fdaf_update_check.cpp: the update kernel's lane (csrc/fdaf_chain.h) compiled for
    the host with exact-size buffers, against the plain loop over (p, b), P = 1 .. 37
    through two wraps of the ring and at both bin-block edges."""
    exe = tmp_path / "fuc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "crlot-dsp_amd", "csrc"),
                        os.path.join(ROOT, "tools", "fdaf_update_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(const float* d_x, const float* d_d, float* d_e, float* d_y, hipStream_t s) {
    crlot::AdaptiveFilter af(512, 3000, 4);
    crlot::AdaptiveFilter other(256, 100, 2, true);
    af = std::move(other);
    af.set_step(1.0, 0.9, 1e-3);
    af.set_constraint(0);
    af.set_adapt(true);
    af.prepare();
    std::vector<float> h(size_t(af.taps()), 0.001f);
    af.set_taps(h.data(), 1, af.taps());
    af.push_device(d_x, d_d, d_e, d_y, s);
    af.push_device(nullptr, d_d, d_e);
    af.constrain(-1, s);
    const std::vector<float> got = af.get_taps();
    const crlot_fdaf_launch r = af.last_launch();
    af.reset();
    return af.state_bytes() + af.hops() + af.channels() + af.partitions() + r.hop_grid + r.update_grid +
           r.constrain_grid + int64_t(got.size()) + (af.get() != nullptr);
}
'''


def test_cpp_class_compiles(tmp_path):
    src = tmp_path / "fdaf_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
