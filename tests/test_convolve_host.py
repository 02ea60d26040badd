"""CPU tests of the convolver's host side (include/crlot_dsp.h, "partitioned FFT
convolution"): every new symbol is declared, exported and bound; the kernel id has its
name; the structs match the header; crlot_convolver_create refuses each bad argument
and needs no device; info and the output length are right; the Python layout checks
refuse bad tensors from their plain descriptions, before any launch; the C++ mirror
compiles.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["crlot_convolver_create", "crlot_convolver_destroy", "crlot_convolver_info", "crlot_convolver_prepare",
               "crlot_convolver_spectra", "crlot_convolver_plan", "crlot_convolve_output_length",
               "crlot_convolver_set_chunks", "crlot_convolver_last_launch", "crlot_fdl_mac", "crlot_convolve"]


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
    assert len(L.crlot_fdl_mac.argtypes) == 11 and len(L.crlot_convolve.argtypes) == 8
    assert len(L.crlot_convolver_create.argtypes) == 5
    assert L.crlot_abi_version() == 2
    assert pkg.kernel_name(45) == "k_fdl_mac"
    assert pkg.kernel_name(46) == "unknown" and pkg.kernel_name(44) == "unknown" and pkg.kernel_name(41) == "unknown"
    txt = open(pkg.HEADER_PATH).read()
    assert "#define CRLOT_K_FDL_MAC 45" in txt and "#define CRLOT_ABI_VERSION 2" in txt
    for member in ("convolve", "fdl_mac", "output_length", "spectra", "set_chunks", "last_launch", "close", "plan"):
        assert hasattr(pkg.Convolver, member), member


@pytest.mark.parametrize("struct,name", [("ConvolverDesc", "crlot_convolver_desc"),
                                         ("ConvolverLaunch", "crlot_convolver_launch")])
def test_struct_layouts_match_header(pkg, struct, name):
    txt = open(pkg.HEADER_PATH).read()
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(getattr(pkg, struct)._fields_)
    assert C.sizeof(pkg.ConvolverDesc) == 16 and C.sizeof(pkg.ConvolverLaunch) == 32


def _create(pkg, taps, block=128, n_filters=None, K=None, ld_h=None, device=0, null_h=False):
    taps = np.ascontiguousarray(np.atleast_2d(taps), np.float32)
    nf = taps.shape[0] if n_filters is None else n_filters
    K = taps.shape[1] if K is None else K
    d = pkg.ConvolverDesc(block, nf, device, 0)
    h = C.c_void_p()
    rc = pkg.lib().crlot_convolver_create(C.byref(d), None if null_h else pkg._fptr(taps), K,
                                          taps.shape[1] if ld_h is None else ld_h, C.byref(h))
    return rc, h


def test_create_refuses_each_bad_argument_without_a_device(pkg):
    L = pkg.lib()

    def err():
        return L.crlot_last_error().decode()

    good = np.linspace(-1, 1, 300, dtype=np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        taps = np.tile(good, (2, 1))
        taps[1, 299] = bad   # the last tap of the last filter
        rc, h = _create(pkg, taps)
        assert rc == pkg.EINVAL and not h and "finite" in err(), bad
    # an N = 2B the plan refuses: odd halves' large primes, beyond 16384, zero, negative
    for block in (0, -128, 8193, 16384, 2 * 8209):
        rc, h = _create(pkg, good, block=block)
        assert rc == pkg.EINVAL and not h and "frame size" in err(), block
    for K in (0, -1, (1 << 20) + 1):
        rc, h = _create(pkg, good, K=K, ld_h=1 << 21)
        assert rc == pkg.EINVAL and not h and "K must" in err(), K
    for nf in (0, -1, 65537):
        rc, h = _create(pkg, good, n_filters=nf)
        assert rc == pkg.EINVAL and not h and "n_filters" in err(), nf
    rc, h = _create(pkg, good, ld_h=299)
    assert rc == pkg.EINVAL and not h and "ld_h" in err()
    rc, h = _create(pkg, good, null_h=True)
    assert rc == pkg.EINVAL and not h and "null" in err()
    assert L.crlot_convolver_create(None, pkg._fptr(good), 300, 300, C.byref(C.c_void_p())) == pkg.EINVAL
    rc, h = _create(pkg, good, device=-2)
    assert rc == pkg.EINVAL and "device" in err()
    # padded rows: ld_h above K is fine, and only K taps of each row are looked at
    taps = np.zeros((2, 310), np.float32)
    taps[:, 300:] = np.nan
    rc, h = _create(pkg, taps, K=300, ld_h=310)
    assert rc == pkg.OK and h
    L.crlot_convolver_destroy(h)
    L.crlot_convolver_destroy(None)


@pytest.mark.parametrize("block,K", [(128, 1), (128, 127), (128, 128), (128, 129), (128, 3 * 128 + 7), (512, 48000),
                                     (2048, 1 << 20), (120, 121), (4096, 5)])
def test_info_and_output_length(pkg, block, K):
    L = pkg.lib()
    rc, h = _create(pkg, np.ones((3, K), np.float32), block=block, device=-1)
    assert rc == pkg.OK, L.crlot_last_error()
    b, nf, k, p = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    assert L.crlot_convolver_info(h, C.byref(b), C.byref(nf), C.byref(k), C.byref(p)) == pkg.OK
    assert (b.value, nf.value, k.value, p.value) == (block, 3, K, -(-K // block))
    assert L.crlot_convolver_info(h, None, None, None, None) == pkg.OK
    assert L.crlot_convolver_info(None, None, None, None, None) == pkg.EINVAL
    for T in (0, 1, block - 1, block, 5 * block + 3, 1 << 40):
        assert L.crlot_convolve_output_length(h, T) == (0 if T == 0 else T + K - 1)
    assert L.crlot_convolve_output_length(h, -1) == pkg.EINVAL
    assert L.crlot_convolve_output_length(None, 4) == pkg.EINVAL
    assert L.crlot_convolver_set_chunks(h, -1) == pkg.EINVAL and L.crlot_convolver_set_chunks(h, 3) == pkg.OK
    rec = pkg.ConvolverLaunch()
    assert L.crlot_convolver_last_launch(h, C.byref(rec)) == pkg.OK and rec.kernel == 0 and rec.grid == 0
    # the empty calls and the argument checks ahead of any device work
    one = C.c_float()
    buf = C.addressof(one)
    assert L.crlot_convolve(h, None, None, 0, 100, 100, 100, None) == pkg.OK
    assert L.crlot_convolve(h, None, None, 4, 0, 0, 0, None) == pkg.OK
    assert L.crlot_convolve(h, buf, buf, -1, 4, 4, 4, None) == pkg.EINVAL
    assert L.crlot_convolve(h, None, buf, 1, 4, 4, 4, None) == pkg.EINVAL
    assert L.crlot_convolve(None, buf, buf, 1, 4, 4, 4, None) == pkg.EINVAL
    assert L.crlot_fdl_mac(h, None, None, 0, 3, 3, 0, 0, 0, 0, None) == pkg.OK
    assert L.crlot_fdl_mac(h, None, None, 2, 3, 0, 0, 0, 0, 0, None) == pkg.OK
    assert L.crlot_fdl_mac(h, buf, buf, 1, -1, 3, 0, 0, 0, 0, None) == pkg.EINVAL
    row = 2 * block + 2
    assert L.crlot_fdl_mac(h, buf, buf, 1, 3, 3, 3 * row, row - 2, 3 * row, row, None) == pkg.EINVAL
    assert "leading dimension" in L.crlot_last_error().decode()
    assert L.crlot_fdl_mac(h, buf, buf, 2, 3, 3, 3 * row - 2, row, 3 * row, row, None) == pkg.EINVAL
    assert L.crlot_fdl_mac(None, buf, buf, 1, 3, 3, 3 * row, row, 3 * row, row, None) == pkg.EINVAL
    L.crlot_convolver_destroy(h)


def test_python_object_on_the_host(pkg):
    c = pkg.Convolver(np.ones(1000, np.float32), block=256, device=0)
    assert (c.block, c.n_filters, c.taps, c.partitions, c.frame_size, c.bins) == (256, 1, 1000, 4, 512, 257)
    assert c.output_length(0) == 0 and c.output_length(7) == 1006 and c.device == 0
    assert c.last_launch()["name"] is None
    c.set_chunks(2)
    with pytest.raises(ValueError):
        c.set_chunks(-1)
    c.close()
    c.close()
    c2 = pkg.Convolver(np.ones((3, 5), np.float32), block=128)
    assert (c2.n_filters, c2.taps, c2.partitions) == (3, 5, 1)
    for bad in (np.ones((2, 2, 2), np.float32), np.ones((2, 0), np.float32), [np.nan, 1.0]):
        with pytest.raises(ValueError):
            pkg.Convolver(bad)
    with pytest.raises(ValueError):
        pkg.Convolver([1.0, 2.0], block=100000)


# ---- the layout checks, from plain descriptions: (shape, strides, dtype, device index or None)
def test_convolve_layouts(pkg):
    f = pkg._convolve_layouts
    x = ((3, 1000), (1000, 1), "float32", 0)
    assert f(x, None, 0, 50) == (3, 1000, 1049, 1000, 1049)
    assert f(((3, 1000), (1024, 1), "float32", 0), ((3, 1100), (1200, 1), "float32", 0), 0, 50) == \
        (3, 1000, 1049, 1024, 1200)
    assert f(((1, 1000), (1, 1), "float32", 0), ((1, 1049), (0, 1), "float32", 0), 0, 50) == (1, 1000, 1049, 1000, 1049)
    assert f(((2, 0), (0, 1), "float32", 0), None, 0, 50)[:3] == (2, 0, 0)
    bad_x = [((3, 1000), (1000, 1), "float64", 0), ((3, 1000), (1000, 1), "float32", None),
             ((3, 1000), (1000, 1), "float32", 1), ((3, 1000), (2000, 2), "float32", 0),
             ((3, 4, 1000), (4000, 1000, 1), "float32", 0), ((3, 1000), (999, 1), "float32", 0)]
    for bx in bad_x:
        with pytest.raises(ValueError):
            f(bx, None, 0, 50)
    bad_y = [((3, 1048), (1048, 1), "float32", 0), ((2, 1049), (1049, 1), "float32", 0),
             ((3, 1049), (1049, 1), "float64", 0), ((3, 1049), (1049, 1), "float32", None),
             ((3, 1049), (1049, 1), "float32", 1), ((3, 1049), (1048, 1), "float32", 0),
             ((3, 1049), (2098, 2), "float32", 0), ((3, 1049, 1), (1049, 1, 1), "float32", 0)]
    for by in bad_y:
        with pytest.raises(ValueError):
            f(x, by, 0, 50)


def test_fdl_layouts(pkg):
    f = pkg._fdl_layouts
    bins, P = 129, 4
    spec = ((3, 70, bins), (70 * bins, bins, 1), "complex64", 0)
    assert f(spec, None, 0, bins, P) == (3, 70, 73, 2 * 70 * bins, 2 * bins, None, None)
    assert f(spec, None, 0, bins, P, 50)[2] == 50
    out = ((3, 73, bins), (80 * 140, 140, 1), "complex64", 0)
    assert f(spec, out, 0, bins, P) == (3, 70, 73, 2 * 70 * bins, 2 * bins, 2 * 80 * 140, 280)
    assert f(((3, 0, bins), (0, bins, 1), "complex64", 0), None, 0, bins, P)[1:3] == (0, 0)
    bad_spec = [((3, 70, bins), (70 * bins, bins, 1), "float32", 0), ((3, 70, bins), (70 * bins, bins, 1), "complex64", None),
                ((3, 70, bins), (70 * bins, bins, 1), "complex64", 1), ((3, 70, 128), (70 * 128, 128, 1), "complex64", 0),
                ((3, 70, bins), (70 * bins, bins - 1, 1), "complex64", 0), ((3, 70, bins), (69 * bins, bins, 1), "complex64", 0),
                ((3, 70, bins), (140 * bins, 2 * bins, 2), "complex64", 0), ((70, bins), (bins, 1), "complex64", 0)]
    for bs in bad_spec:
        with pytest.raises(ValueError):
            f(bs, None, 0, bins, P)
    bad_out = [((3, 72, bins), (72 * bins, bins, 1), "complex64", 0), ((2, 73, bins), (73 * bins, bins, 1), "complex64", 0),
               ((3, 73, bins), (73 * bins, bins, 1), "complex128", 0), ((3, 73, bins), (73 * bins, bins, 1), "complex64", None),
               ((3, 73, bins), (72 * bins, bins, 1), "complex64", 0)]
    for bo in bad_out:
        with pytest.raises(ValueError):
            f(spec, bo, 0, bins, P)
    for bad_f in (-1, 2.5, True):
        with pytest.raises(ValueError):
            f(spec, None, 0, bins, P, bad_f)


def test_torch_front_refuses_before_any_call(pkg):
    """Host tensors, wrong dtypes and shapes and overlapping buffers never reach the
    library (the object here has no handle: reaching it would not raise ValueError)."""
    import torch
    c = object.__new__(pkg.Convolver)
    c._h, c._plan, c._device = None, None, 0
    c.block, c.n_filters, c.taps, c.partitions, c.frame_size, c.bins = 128, 1, 300, 3, 256, 129
    for bad in (torch.zeros(2, 1000), torch.zeros(2, 1000).double(), torch.zeros(2, 3, 1000)):
        with pytest.raises(ValueError):
            pkg.Convolver.convolve(c, bad)
    for bad in (torch.zeros(2, 8, 129, dtype=torch.complex64), torch.zeros(2, 8, 129),
                torch.zeros(2, 8, 128, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            pkg.Convolver.fdl_mac(c, bad)


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(const float* d_x, float* d_y, const float* d_spec, float* d_out) {
    std::vector<float> h(3000, 0.001f);
    crlot::Convolver c(h, 512);
    crlot::Convolver many(h.data(), 1000, 256, 3, 1000, 0);
    c = std::move(many);
    c.convolve_device(d_x, d_y, 3, 48000, 48000, c.output_length(48000));
    c.fdl_mac_device(d_spec, d_out, 3, 94, 100, 94 * 514, 514, 100 * 514, 514);
    crlot_plan* p = c.plan();
    (void)p;
    return c.taps() + c.block() + c.partitions() + c.n_filters() + int64_t(c.spectra().size());
}
'''


def test_cpp_class_compiles(tmp_path):
    src = tmp_path / "convolve_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
