"""CPU tests of the resampler's host side (include/crlot_dsp.h, "resample / pitch
shift"): the symbols are declared, exported and bound and the two kernel ids have
their names; the output length; each bad descriptor; the table against the
float64 formula; crlot_rational_approx against fractions.Fraction; null arguments
are refused before a device is touched; the Python layout checks; the C++ mirror
compiles.  An object is created without a device: its table is uploaded by the
first device call, and nothing here makes one."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import resample_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["crlot_resampler_create", "crlot_resampler_destroy", "crlot_resampler_info", "crlot_resampler_table",
               "crlot_resampler_prepare", "crlot_resample_output_length", "crlot_resampler_set_route",
               "crlot_resampler_set_tile", "crlot_resampler_last_launch", "crlot_resample", "crlot_pitch_shift",
               "crlot_rational_approx", "crlot_resample_geometry", "crlot_resample_table_host"]


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
    for kid, name in ((37, "k_resample_phase"), (38, "k_resample_any")):
        assert pkg.kernel_name(kid) == name
    for m in ("resample", "output_length", "table", "set_route", "set_tile", "last_launch"):
        assert callable(getattr(pkg.Resampler, m)), m
    assert callable(pkg.Plan.pitch_shift) and callable(pkg.rational_approx)


def test_output_length_and_geometry(pkg):
    for up, down in ((48000, 44100), (44100, 48000), (1, 2), (2, 1), (3, 1), (1, 3), (7, 5), (89, 84), (1, 64),
                     (64, 1), (1021, 1024), (4096, 4095)):
        for zeros in (1, 6, 16):
            U, D, W, K, _ = RR.geometry(up, down, zeros)
            if U * K > 2 ** 21:
                continue
            r = pkg.Resampler(up, down, zeros=zeros)
            assert (r.up, r.down, r.half_width, r.taps) == (U, D, W, K), (up, down, zeros)
            assert r.info == pkg.resample_geometry(up, down, zeros=zeros)
            for T in (0, 1, 2, 3, 5, 146, 147, 148, 1000, 1777, 480000, 2 ** 40):
                L = r.output_length(T)
                assert L == RR.output_length(T, U, D) == -(-T * U // D), (up, down, T)
            assert r.output_length(0) == 0
            for bad in (-1, 2 ** 48 + 1):
                with pytest.raises(ValueError):
                    r.output_length(bad)
            last = r.last_launch()
            assert last["kernel"] == 0 and last["name"] is None  # (no launch yet)
            r.close()
    # which shapes the phase kernel takes: taps within 104, U within one workgroup
    assert pkg.resample_geometry(48000, 44100)["phase_ok"] == 1
    assert pkg.resample_geometry(16000, 48000)["phase_ok"] == 1          # K = 102
    assert pkg.resample_geometry(1, 64, zeros=4)["phase_ok"] == 0        # K = 540
    assert pkg.resample_geometry(1021, 1024, zeros=6)["phase_ok"] == 0   # U = 1021
    r = pkg.Resampler(1, 64, zeros=4)
    r.set_route("any"), r.set_route("auto"), r.set_tile(3), r.set_tile(0)
    with pytest.raises(NotImplementedError):
        r.set_route("phase")
    with pytest.raises(ValueError):
        r.set_route(7)
    with pytest.raises(ValueError):
        r.set_tile(-1)


GOOD = dict(up=160, down=147, zeros=16, rolloff=0.95, window=0, beta=8.6, device=0)


@pytest.mark.parametrize("field,value", [
    ("up", 0), ("up", -3), ("down", 0), ("down", -1),
    ("up", 4097), ("down", 4099),                        # reduced rates beyond 4096 (both prime to 160 / 147)
    ("zeros", 0), ("zeros", 65), ("zeros", -1),
    ("rolloff", 0.49), ("rolloff", 1.01), ("rolloff", float("nan")), ("rolloff", float("inf")),
    ("window", 2), ("window", -1),
    ("device", -1),
])
def test_bad_descriptor_is_einval(pkg, field, value):
    L = pkg.lib()
    d = pkg.ResamplerDesc(GOOD["up"], GOOD["down"], GOOD["zeros"], GOOD["window"], GOOD["rolloff"], GOOD["beta"],
                          GOOD["device"], 0)
    h, g = C.c_void_p(), pkg.ResamplerGeometry()
    assert L.crlot_resampler_create(C.byref(d), C.byref(h)) == pkg.OK and h.value
    L.crlot_resampler_destroy(h)
    setattr(d, field, value)
    h = C.c_void_p()
    assert L.crlot_resampler_create(C.byref(d), C.byref(h)) == pkg.EINVAL, (field, value)
    assert not h.value
    assert L.crlot_resample_geometry(C.byref(d), C.byref(g)) == pkg.EINVAL


def test_more_bad_descriptors(pkg):
    L = pkg.lib()
    h = C.c_void_p()

    def create(**kw):
        a = dict(GOOD, **kw)
        d = pkg.ResamplerDesc(a["up"], a["down"], a["zeros"], a["window"], a["rolloff"], a["beta"], a["device"], 0)
        rc = L.crlot_resampler_create(C.byref(d), C.byref(h))
        if rc == pkg.OK:
            L.crlot_resampler_destroy(h)
        return rc

    # Kaiser's beta: finite and in [0, 20]; Hann ignores it
    for beta in (-0.1, 20.5, float("nan"), float("inf")):
        assert create(window=1, beta=beta) == pkg.EINVAL, beta
        assert create(window=0, beta=beta) == pkg.OK, beta
    assert create(window=1, beta=0.0) == pkg.OK and create(window=1, beta=20.0) == pkg.OK
    # the ratio: [1/64, 64] after reduction
    assert create(up=65, down=1) == pkg.EINVAL and create(up=1, down=65) == pkg.EINVAL
    assert create(up=64, down=1) == pkg.OK and create(up=128, down=2) == pkg.OK
    assert create(up=8192, down=8190) == pkg.OK      # 4096 / 4095 once reduced
    # The table cap (2^21 floats, CRLOT_EUNSUPPORTED) guards the arithmetic: within the other limits
    # U K = 2 U ceil(zeros D / (min(U, D) rolloff)) <= 2 * 64 * 4096 / 0.5 + 2 U < 2^20 + 2^13, so no valid
    # descriptor reaches it.  The largest tables are accepted:
    for up, down in ((4096, 4095), (1023, 4096), (2047, 4096), (4095, 4096), (1365, 4096), (64, 4096)):
        assert create(up=up, down=down, zeros=64, rolloff=0.5) == pkg.OK


@pytest.mark.parametrize("window", ["hann", "kaiser"])
def test_table_accuracy(pkg, window):
    """Every entry within 2^-23 max(|ref|, 2^-126) of the float64 formula (half an ulp
    of rounding plus double-evaluation noise); entries with |tau| >= zeros exactly +0."""
    worst = 0.0
    for up, down, zeros in ((160, 147, 16), (147, 160, 16), (2, 1, 16), (1, 2, 16), (3, 1, 6), (1, 3, 6), (7, 5, 4),
                            (89, 84, 16), (1, 64, 4), (1021, 1024, 6), (1, 1, 1), (64, 1, 64)):
        for rolloff, beta in ((0.95, 8.6), (0.5, 0.0), (1.0, 20.0)):
            ref, tau = RR.table(up, down, zeros, rolloff, window, beta)
            got = pkg.resample_table_host(up, down, zeros, rolloff, window, beta)
            assert got.shape == ref.shape and got.dtype == np.float32
            tol = 2.0 ** -23 * np.maximum(np.abs(ref), 2.0 ** -126)
            err = np.abs(got.astype(np.float64) - ref)
            worst = max(worst, float((err / tol).max()))
            assert np.all(err <= tol), (up, down, zeros, rolloff, float((err / tol).max()))
            out = np.abs(tau) >= zeros
            assert np.all(got.view(np.uint32)[out] == 0)  # +0, not -0
            r = pkg.Resampler(up, down, zeros, rolloff, window, beta)
            assert np.array_equal(r.table().view(np.uint32), got.view(np.uint32))
            r.close()
    print(f"{window}: worst entry error {worst:.3f} of the tolerance")


def test_rational_approx(pkg):
    cases = [2.0 ** (k / 12.0) for k in range(-24, 25)]
    cases += [0.75, 1.0, 3.0, 1 / 3, 160 / 147, 89 / 84, 44100 / 48000, 0.1, 1e-3, 12345.678, 2.0 ** -31, 2.0 ** 30]
    for ratio in cases:
        for max_den in (1, 12, 256, 4096):
            f = Fraction(ratio).limit_denominator(max_den)
            if f.numerator > 2 ** 31 - 1:
                continue
            assert pkg.rational_approx(ratio, max_den) == (f.numerator, f.denominator), (ratio, max_den)
    assert pkg.rational_approx(2 ** (1 / 12), 100) == (89, 84) and pkg.rational_approx(2 ** (1 / 12), 256) == (196, 185)
    L = pkg.lib()
    n, d = C.c_int32(), C.c_int32()
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert L.crlot_rational_approx(bad, 256, C.byref(n), C.byref(d)) == pkg.EINVAL, bad
    for bad in (0, -1):
        assert L.crlot_rational_approx(1.5, bad, C.byref(n), C.byref(d)) == pkg.EINVAL, bad
    assert L.crlot_rational_approx(1.5, 4, None, C.byref(d)) == pkg.EINVAL
    assert L.crlot_rational_approx(1.5, 4, C.byref(n), None) == pkg.EINVAL


def test_entries_reject_before_device(pkg):
    L = pkg.lib()
    assert L.crlot_resample(None, None, None, 1, 4, 4, 4, None) == pkg.EINVAL
    assert L.crlot_pitch_shift(None, None, None, None, 1, 4, 4, 4, None) == pkg.EINVAL
    assert L.crlot_resample_output_length(None, 4) == pkg.EINVAL
    assert L.crlot_resampler_create(None, None) == pkg.EINVAL
    h = C.c_void_p()
    assert L.crlot_resampler_create(None, C.byref(h)) == pkg.EINVAL
    assert L.crlot_resampler_info(None, None) == pkg.EINVAL
    assert L.crlot_resampler_table(None, None) == pkg.EINVAL
    assert L.crlot_resampler_prepare(None) == pkg.EINVAL
    assert L.crlot_resampler_set_route(None, 0) == pkg.EINVAL
    assert L.crlot_resampler_set_tile(None, 0) == pkg.EINVAL
    assert L.crlot_resampler_last_launch(None, None) == pkg.EINVAL
    L.crlot_resampler_destroy(None)
    r = pkg.Resampler(2, 1)
    # sizes and buffers, checked ahead of the device: negative sizes, null buffers, empty calls
    assert L.crlot_resample(r._h, None, None, -1, 4, 4, 8, None) == pkg.EINVAL
    assert L.crlot_resample(r._h, None, None, 1, -4, 4, 8, None) == pkg.EINVAL
    assert L.crlot_resample(r._h, None, None, 1, 4, 4, 8, None) == pkg.EINVAL
    assert L.crlot_resample(r._h, None, None, 0, 4, 4, 8, None) == pkg.OK
    assert L.crlot_resample(r._h, None, None, 3, 0, 0, 0, None) == pkg.OK
    assert L.crlot_pitch_shift(None, r._h, None, None, 1, 4, 4, 4, None) == pkg.EINVAL


def test_layout_checks(pkg):
    """Every bad case differs from the good one in one thing."""
    S, L = 3, 100
    assert pkg._resample_y_layout((S, L), (L, 1), "float32", 0, S, L) == L
    assert pkg._resample_y_layout((S, L + 7), (L + 7, 1), "float32", 0, S, L) == L + 7
    assert pkg._resample_y_layout((1, L), (0, 1), "float32", 0, 1, L) == L  # a size-1 dim's stride is meaningless
    for bad in (((S, L), (L, 1), "float64", 0),        # dtype
                ((S, L), (L, 1), "float32", None),     # a host tensor
                ((S, L), (2 * L, 2), "float32", 0),    # rows not contiguous
                ((S, L - 1), (L - 1, 1), "float32", 0),  # too short
                ((S + 1, L), (L, 1), "float32", 0),    # wrong stream count
                ((S, L), (L - 1, 1), "float32", 0),    # rows overlap
                ((L,), (1,), "float32", 0)):           # not 2-d
        with pytest.raises(ValueError):
            pkg._resample_y_layout(*bad, S, L)
    # the torch front: host tensors, a wrong dtype and non-contiguous rows are refused before any call
    import torch
    r = pkg.Resampler(160, 147)
    for bad in (torch.zeros(2, 4096), torch.zeros(2, 4096, dtype=torch.float64), torch.zeros(2, 4096, 2)[:, :, 0],
                torch.zeros(2, 3, 4)):
        with pytest.raises(ValueError):
            r.resample(bad)
    plan = object.__new__(pkg.Plan)
    plan.frame_size, plan.hop_size = 1024, 256
    plan.cfg = pkg.PlanConfig(device=0)
    for bad in (torch.zeros(2, 4096), torch.zeros(2, 4096, dtype=torch.float64), torch.zeros(2, 4096, 2)[:, :, 0]):
        with pytest.raises(ValueError):
            pkg.Plan.pitch_shift(plan, bad, r)
        with pytest.raises(ValueError):
            pkg.Plan.pitch_shift(plan, bad, semitones=1)
    with pytest.raises(ValueError):  # neither, and both
        pkg.Plan.pitch_shift(plan, torch.zeros(2, 4096))
    with pytest.raises(ValueError):
        pkg.Plan.pitch_shift(plan, torch.zeros(2, 4096), r, semitones=1)
    with pytest.raises(ValueError):
        pkg.Resampler(160, 147, window="blackman")


CPP_TU = r'''
#include "crlot_dsp.hpp"
int64_t probe(crlot::StftEngine& e, const float* d_x, float* d_y) {
    crlot::Resampler r(160, 147);
    crlot::Resampler k(1, 3, 6, 0.9, CRLOT_RESAMPLE_KAISER, 8.6, 0);
    crlot::Resampler moved(std::move(k));
    const int64_t L = r.output_length(10000);
    r.resample_device(d_x, d_y, 3, 10000, 10000, L);
    e.pitch_shift_device(r, d_x, d_y, 3, 10000, 10000, 10000);
    const std::pair<int, int> q = crlot::Resampler::rational_approx(1.0594630943592953, 256);
    return L + q.first + r.info().taps + int64_t(r.table().size());
}
'''


def test_cpp_methods_compile(tmp_path):
    src = tmp_path / "resample_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
