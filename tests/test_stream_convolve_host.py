"""CPU tests of the streaming convolver's host side (include/crlot_dsp.h, "streaming
convolution"): every new symbol is declared, exported and bound; the kernel ids have
their names and the unassigned ones stay unknown; crlot_sconv_launch matches the
header; crlot_stream_convolver_create needs no device, refuses each bad argument and
every block outside 128 / 256 / 512 / 1024; the state size, info and the empty launch
record are right; the Python layout checks refuse bad tensors from their plain
descriptions and a host tensor never reaches the library; the C++ mirror compiles.
No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = {"crlot_stream_convolver_create": 3, "crlot_stream_convolver_destroy": 1,
               "crlot_stream_convolver_prepare": 1, "crlot_stream_convolver_state_bytes": 1,
               "crlot_stream_convolver_reset": 1, "crlot_stream_convolver_set_layout": 2,
               "crlot_stream_convolver_set_route": 2, "crlot_stream_convolver_set_prefetch": 2,
               "crlot_stream_convolver_info": 5, "crlot_stream_convolver_last_launch": 2,
               "crlot_stream_convolve_hop": 4, "crlot_stream_convolve_prefetch": 2}


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
    assert pkg.kernel_name(47) == "k_sconv_head" and pkg.kernel_name(48) == "k_sconv_tail"
    for unassigned in (41, 44, 46):
        assert pkg.kernel_name(unassigned) == "unknown", unassigned
    txt = open(pkg.HEADER_PATH).read()
    assert "#define CRLOT_K_SCONV_HEAD 47" in txt and "#define CRLOT_K_SCONV_TAIL 48" in txt
    assert "#define CRLOT_ABI_VERSION 2" in txt
    for member in ("push", "prefetch", "reset", "prepare", "set_route", "set_prefetch", "last_launch", "state_bytes",
                   "hops", "close"):
        assert hasattr(pkg.StreamConvolver, member), member


def test_launch_struct_matches_header(pkg):
    txt = open(pkg.HEADER_PATH).read()
    m = re.search(r"typedef struct crlot_sconv_launch \{(.*?)\} crlot_sconv_launch;", txt, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(pkg.SconvLaunch._fields_)
    assert [n for n, _ in fields] == ["head_kernel", "tail_kernel", "head_grid", "tail_grid", "route", "tail_pending"]
    assert C.sizeof(pkg.SconvLaunch) == 32


def _convolver(pkg, block, K, nf=1):
    d = pkg.ConvolverDesc(block, nf, -1, 0)
    taps = np.ones((nf, K), np.float32)
    h = C.c_void_p()
    assert pkg.lib().crlot_convolver_create(C.byref(d), pkg._fptr(taps), K, K, C.byref(h)) == pkg.OK
    return h


def test_create_without_a_device(pkg):
    L = pkg.lib()

    def err():
        return L.crlot_last_error().decode()

    conv = _convolver(pkg, 128, 300)
    sc = C.c_void_p()
    assert L.crlot_stream_convolver_create(None, 2, C.byref(sc)) == pkg.EINVAL and not sc and "null" in err()
    assert L.crlot_stream_convolver_create(conv, 2, None) == pkg.EINVAL and "null" in err()
    for channels in (0, -1):
        assert L.crlot_stream_convolver_create(conv, channels, C.byref(sc)) == pkg.EINVAL and not sc
        assert "channels" in err()
    # blocks the offline convolver accepts and the hop kernels do not
    for block in (2048, 120, 4096):
        other = _convolver(pkg, block, 2 * block + 1)
        assert L.crlot_stream_convolver_create(other, 2, C.byref(sc)) == pkg.EUNSUPPORTED and not sc, block
        assert all(size in err() for size in ("128", "256", "512", "1024")), err()
        L.crlot_convolver_destroy(other)
    assert L.crlot_stream_convolver_create(conv, 2, C.byref(sc)) == pkg.OK and sc
    ch, b, p, hops = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(-1)
    assert L.crlot_stream_convolver_info(sc, C.byref(ch), C.byref(b), C.byref(p), C.byref(hops)) == pkg.OK
    assert (ch.value, b.value, p.value, hops.value) == (2, 128, 3, 0)
    assert L.crlot_stream_convolver_info(sc, None, None, None, None) == pkg.OK
    assert L.crlot_stream_convolver_info(None, None, None, None, None) == pkg.EINVAL
    rec = pkg.SconvLaunch(9, 9, 9, 9, 9, 9)
    assert L.crlot_stream_convolver_last_launch(sc, C.byref(rec)) == pkg.OK
    assert (rec.head_kernel, rec.tail_kernel, rec.head_grid, rec.tail_grid, rec.route, rec.tail_pending) == (0,) * 6
    assert L.crlot_stream_convolver_last_launch(sc, None) == pkg.EINVAL
    assert L.crlot_stream_convolver_last_launch(None, C.byref(rec)) == pkg.EINVAL
    for bad in (3, -1):
        assert L.crlot_stream_convolver_set_route(sc, bad) == pkg.EINVAL and "route" in err()
    for ok in (1, 2, 0):
        assert L.crlot_stream_convolver_set_route(sc, ok) == pkg.OK
    assert L.crlot_stream_convolver_set_route(None, 1) == pkg.EINVAL
    assert L.crlot_stream_convolver_set_prefetch(sc, 0) == pkg.OK and L.crlot_stream_convolver_set_prefetch(sc, 1) == pkg.OK
    assert L.crlot_stream_convolver_set_prefetch(None, 1) == pkg.EINVAL
    assert L.crlot_stream_convolver_set_layout(sc, 1) == pkg.OK and L.crlot_stream_convolver_set_layout(None, 1) == pkg.EINVAL
    # nothing to reset, nothing pending: no device is touched
    assert L.crlot_stream_convolver_reset(sc) == pkg.OK and L.crlot_stream_convolver_reset(None) == pkg.EINVAL
    assert L.crlot_stream_convolve_prefetch(sc, None) == pkg.OK and L.crlot_stream_convolve_prefetch(None, None) == pkg.EINVAL
    # the argument checks of a hop come before any device work
    one = (C.c_float * (2 * 128))()
    buf = C.addressof(one)
    assert L.crlot_stream_convolve_hop(None, buf, buf, None) == pkg.EINVAL
    assert L.crlot_stream_convolve_hop(sc, buf, None, None) == pkg.EINVAL and "null" in err()
    assert L.crlot_stream_convolve_hop(sc, buf, buf, None) == pkg.EINVAL and "overlap" in err()
    assert L.crlot_stream_convolve_hop(sc, buf + 4 * 255, buf, None) == pkg.EINVAL and "overlap" in err()
    assert L.crlot_stream_convolver_prepare(None) == pkg.EINVAL
    L.crlot_stream_convolver_destroy(sc)
    L.crlot_stream_convolver_destroy(None)
    L.crlot_convolver_destroy(conv)


@pytest.mark.parametrize("block,K,channels", [(128, 1, 1), (256, 48000, 1024), (1024, 3 * 1024 + 1, 7)])
def test_state_bytes(pkg, block, K, channels):
    """Per channel the ring [P][N+2], the partial chain [N+2] and the carry [B], floats."""
    L = pkg.lib()
    conv = _convolver(pkg, block, K)
    sc = C.c_void_p()
    assert L.crlot_stream_convolver_create(conv, channels, C.byref(sc)) == pkg.OK
    P, row = -(-K // block), 2 * block + 2
    assert L.crlot_stream_convolver_state_bytes(sc) == 4 * channels * (P * row + row + block)
    assert L.crlot_stream_convolver_state_bytes(None) == pkg.EINVAL
    L.crlot_stream_convolver_destroy(sc)
    L.crlot_convolver_destroy(conv)


def test_python_object_on_the_host(pkg):
    conv = pkg.Convolver(np.ones(1000, np.float32), block=256, device=0)
    sc = pkg.StreamConvolver(conv, 3, interleaved=True)
    assert (sc.channels, sc.block, sc.partitions, sc.hops, sc.interleaved) == (3, 256, 4, 0, True)
    assert sc.state_bytes == 4 * 3 * (4 * 514 + 514 + 256)
    assert sc.conv is conv
    rec = sc.last_launch()
    assert rec["head_name"] is None and rec["tail_name"] is None and rec["route"] == 0 and rec["tail_pending"] == 0
    sc.set_route(1)
    sc.set_prefetch(False)
    with pytest.raises(ValueError):
        sc.set_route(3)
    sc.reset()
    sc.close()
    sc.close()
    with pytest.raises(ValueError):
        pkg.StreamConvolver(conv, 0)
    with pytest.raises(ValueError):
        pkg.StreamConvolver(object(), 2)
    with pytest.raises(NotImplementedError):
        pkg.StreamConvolver(pkg.Convolver(np.ones(10, np.float32), block=2048), 2)


def test_hop_layouts(pkg):
    f = pkg._sconv_hop_layout
    assert f(((3, 128), (128, 1), "float32", 0), 0, 3, 128, False) == (3, 128)
    assert f(((128, 3), (3, 1), "float32", 0), 0, 3, 128, True) == (128, 3)
    assert f(((1, 128), (999, 1), "float32", 0), 0, 1, 128, False) == (1, 128)   # one row: its stride is not read
    bad = [((3, 128), (128, 1), "float64", 0), ((3, 128), (128, 1), "float32", None), ((3, 128), (128, 1), "float32", 1),
           ((128, 3), (3, 1), "float32", 0), ((3, 127), (127, 1), "float32", 0), ((2, 128), (128, 1), "float32", 0),
           ((3, 128), (256, 1), "float32", 0), ((3, 128), (1, 3), "float32", 0), ((3, 128, 1), (128, 1, 1), "float32", 0),
           ((384,), (1,), "float32", 0)]
    for layout in bad:
        with pytest.raises(ValueError):
            f(layout, 0, 3, 128, False)
    with pytest.raises(ValueError):
        f(((3, 128), (128, 1), "float32", 0), 0, 3, 128, True)


def test_torch_front_refuses_before_any_call(pkg):
    """Host tensors, wrong dtypes and shapes never reach the library (the object here has
    no handle: reaching it would not raise ValueError)."""
    import torch
    conv = object.__new__(pkg.Convolver)
    conv._h, conv._plan, conv._device = None, None, 0
    sc = object.__new__(pkg.StreamConvolver)
    sc._h, sc.conv, sc.channels, sc.block, sc.partitions, sc.interleaved = None, conv, 3, 128, 2, False
    for bad in (torch.zeros(3, 128), torch.zeros(3, 128).double(), torch.zeros(128, 3), np.zeros((3, 128), np.float32)):
        with pytest.raises(ValueError):
            pkg.StreamConvolver.push(sc, bad)
    sc.conv = None


def test_tail_chain_equals_the_plain_chain_on_cpu(tmp_path):
    """tools/sconv_tail_check.cpp: the tail kernel's lane (csrc/sconv_chain.h) compiled for
    the host with exact-size buffers, against crlot_fdl_mac's plain chain over the whole
    history, P = 1 .. 37 through two wraps of the ring and at both bin-block edges."""
    exe = tmp_path / "stc"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "crlot-dsp_amd", "csrc"),
                        os.path.join(ROOT, "tools", "sconv_tail_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:]


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(const float* d_in, float* d_out, hipStream_t s) {
    std::vector<float> h(3000, 0.001f);
    crlot::Convolver c(h, 512);
    crlot::StreamConvolver sc(c, 4);
    crlot::StreamConvolver other(c, 2, true);
    sc = std::move(other);
    sc.set_route(2);
    sc.set_prefetch(false);
    sc.prepare();
    sc.push_device(d_in, d_out, s);
    sc.prefetch(s);
    sc.push_device(nullptr, d_out);
    const crlot_sconv_launch r = sc.last_launch();
    sc.reset();
    return sc.state_bytes() + sc.hops() + r.head_grid + r.tail_grid + r.route + r.tail_pending + (sc.get() != nullptr);
}
'''


def test_cpp_class_compiles(tmp_path):
    src = tmp_path / "stream_convolve_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
