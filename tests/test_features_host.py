"""CPU tests of the spectrogram features' host side (include/crlot_dsp.h,
"spectrogram features"): the new symbols are declared, exported and bound; the
mel filterbank follows its formulas; filterbank rows reduce to the documented
spans; Features.spectrogram refuses bad tensors before anything touches a
device; the C++ mirror compiles.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["crlot_features_create", "crlot_features_destroy", "crlot_features_info", "crlot_spectrogram",
               "crlot_mel_filterbank", "crlot_filterbank_spans"]


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
    assert C.sizeof(pkg.FeaturesDesc) == 4 * 4
    for kid, name in ((32, "k_feat"), (33, "k_pair_feat"), (34, "k_feat_step")):
        assert pkg.kernel_name(kid) == name
    assert (pkg.FEAT_POWER, pkg.FEAT_MAGNITUDE) == (0, 1)
    assert (pkg.FEAT_LIN, pkg.FEAT_LN, pkg.FEAT_LOG10, pkg.FEAT_DB) == (0, 1, 2, 3)
    assert (pkg.MEL_HTK, pkg.MEL_SLANEY) == (0, 1)


# ------------------------------------------------------------------ mel filterbank
def hz_to_mel(f, scale):
    f = np.asarray(f, np.float64)
    if scale == 0:
        return 2595.0 * np.log10(1.0 + f / 700.0)
    lin = f / (200.0 / 3.0)
    log = 1000.0 / (200.0 / 3.0) + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f < 1000.0, lin, log)


def mel_to_hz(m, scale):
    m = np.asarray(m, np.float64)
    if scale == 0:
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    mb = 1000.0 / (200.0 / 3.0)
    return np.where(m < mb, m * (200.0 / 3.0), 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - mb)))


def mel_ref(n_mels, nfft, sr, fmin, fmax, scale, norm):
    """The issue's formulas restated in float64."""
    fmax = sr / 2 if fmax is None else fmax
    pts = mel_to_hz(np.linspace(hz_to_mel(fmin, scale), hz_to_mel(fmax, scale), n_mels + 2), scale)
    fb = np.arange(nfft // 2 + 1, dtype=np.float64) * sr / nfft
    W = np.zeros((n_mels, nfft // 2 + 1))
    for j in range(n_mels):
        lo, c, hi = pts[j], pts[j + 1], pts[j + 2]
        W[j] = np.maximum(0.0, np.minimum((fb - lo) / (c - lo), (hi - fb) / (hi - c)))
        if norm:
            W[j] *= 2.0 / (hi - lo)
    return W


@pytest.mark.parametrize("n_mels,nfft,sr", [(80, 1024, 16000), (40, 512, 8000), (128, 4096, 48000), (1, 256, 8000)])
@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("norm", [False, True])
def test_mel_filterbank_vs_float64_formulas(pkg, n_mels, nfft, sr, scale, norm):
    for fmin in (0.0, 20.0):
        for fmax in (None, 7600.0):
            if fmax is not None and fmax > sr / 2:
                with pytest.raises(ValueError):
                    pkg.mel_filterbank(n_mels, nfft, sr, fmin, fmax, scale, norm)
                continue
            W = pkg.mel_filterbank(n_mels, nfft, sr, fmin, fmax, scale, norm)
            assert W.dtype == np.float32 and W.shape == (n_mels, nfft // 2 + 1)
            ref = mel_ref(n_mels, nfft, sr, fmin, fmax, scale, norm)
            # float32 rounding (6e-8) with room for libm's log10 / exp last bits
            assert np.allclose(W, ref, rtol=1e-6, atol=1e-9), (fmin, fmax, float(np.max(np.abs(W - ref))))
            assert np.all(W >= 0)
            for j in range(n_mels):  # the non-zero bins of a row form one contiguous run
                nz = np.flatnonzero(W[j])
                assert nz.size == 0 or nz[-1] - nz[0] + 1 == nz.size, (j, nz)


@pytest.mark.parametrize("args", [
    (0, 1024, 16000.0, 0.0, None),      # n_mels < 1
    (80, 1023, 16000.0, 0.0, None),     # odd nfft
    (80, 0, 16000.0, 0.0, None),        # nfft < 2
    (80, 1024, 16000.0, -1.0, None),    # fmin < 0
    (80, 1024, 16000.0, 4000.0, 4000.0),  # fmin == fmax
    (80, 1024, 16000.0, 5000.0, 4000.0),  # fmin > fmax
    (80, 1024, 16000.0, 0.0, 8000.5),   # fmax > sample_rate / 2
])
def test_mel_filterbank_rejects(pkg, args):
    with pytest.raises(ValueError):
        pkg.mel_filterbank(*args)


# ------------------------------------------------------------------ spans
def test_filterbank_spans(pkg):
    bins = 129
    W = np.zeros((6, bins), np.float32)
    W[0, 17] = 0.5                      # width 1
    # row 1: all zero
    W[2, :] = 1.0                       # dense
    W[3, 10] = 1.0                      # interior zeros stay inside the span
    W[3, 20] = -2.0
    W[4, 0] = 1.0                       # touches bin 0 and bin N/2
    W[4, bins - 1] = 1.0
    W[5, bins - 1] = 3.0                # width 1 on bin N/2
    lo, hi = pkg.filterbank_spans(W)
    assert lo.tolist() == [17, 0, 0, 10, 0, bins - 1]
    assert hi.tolist() == [18, 0, bins, 21, bins, bins]
    mel = pkg.mel_filterbank(40, 256, 8000)
    lo, hi = pkg.filterbank_spans(mel)
    for j in range(40):
        nz = np.flatnonzero(mel[j])
        assert (lo[j], hi[j]) == ((nz[0], nz[-1] + 1) if nz.size else (0, 0))
    with pytest.raises(ValueError):
        pkg.filterbank_spans(np.zeros(5, np.float32))


# ------------------------------------------------------------------ argument checks before the device
def test_spectrogram_layout_checks(pkg):
    """The checks Features.spectrogram makes before anything touches a device, on
    plain descriptions (shape, strides, dtype name, device index or None), so that
    each clause is tested alone: every bad case differs from the good one in one thing."""
    T, S, F, n = 4096, 2, 16, 513
    x_ok = ((S, T), (T, 1), "float32", 0)
    assert pkg._spectrogram_x_layout(*x_ok) == (S, T)
    assert pkg._spectrogram_x_layout((S, T), (2 * T, 1), "float32", 0) == (S, T)   # padded rows are fine
    for bad in (((S, T), (T, 1), "float64", 0),        # wrong dtype
                ((S, T), (T, 1), "float32", None),     # a CPU tensor
                ((S, 3, T), (3 * T, T, 1), "float32", 0),  # wrong shape
                ((S, T), (2 * T, 2), "float32", 0)):   # rows not contiguous
        with pytest.raises(ValueError):
            pkg._spectrogram_x_layout(*bad)
    o_ok = ((S, F, n), (F * n, n, 1), "float32", 0)
    assert pkg._spectrogram_out_layout(*o_ok, S, F, n) == (F * n, n)
    assert pkg._spectrogram_out_layout((S, F, n), ((F + 2) * (n + 5), n + 5, 1), "float32", 0, S, F, n) == \
        ((F + 2) * (n + 5), n + 5)
    for bad in (((S, F, n), (F * n, n, 1), "float16", 0),
                ((S, F, n), (F * n, n, 1), "float32", None),
                ((S, F, n + 1), (F * (n + 1), n + 1, 1), "float32", 0),    # wrong n_out
                ((S, F + 1, n), ((F + 1) * n, n, 1), "float32", 0),        # wrong frame count
                ((S, F, n), (F * n, n - 1, 1), "float32", 0),              # ld_frame < n_out
                ((S, F, n), (2 * F * n, 2 * n, 2), "float32", 0)):         # rows not contiguous
        with pytest.raises(ValueError):
            pkg._spectrogram_out_layout(*bad, S, F, n)
    # the torch front of the same checks, and the stft entry they mirror: a CPU tensor and a wrong dtype
    import torch
    assert pkg._tensor_layout(torch.zeros(2, 8, dtype=torch.float64)) == ((2, 8), (8, 1), "float64", None)
    for bad in (torch.zeros(2, 4 * 1024), torch.zeros(2, 4 * 1024, dtype=torch.float64)):
        with pytest.raises(ValueError):
            pkg.Features.spectrogram(object.__new__(pkg.Features), bad)
        with pytest.raises(ValueError):
            pkg.Plan.stft(object.__new__(pkg.Plan), bad)


def test_features_create_rejects_before_device(pkg):
    """crlot_features_create validates its plan and descriptor arguments first."""
    L = pkg.lib()
    h = C.c_void_p()
    d = pkg.FeaturesDesc(0, 0, 0, 0.0)
    assert L.crlot_features_create(None, C.byref(d), None, C.byref(h)) == pkg.EINVAL
    assert b"null" in L.crlot_last_error()
    assert L.crlot_spectrogram(None, None, None, 1, 16, 16, 16, 16, None) == pkg.EINVAL
    assert L.crlot_features_info(None, None, None, None, None) == pkg.EINVAL
    L.crlot_features_destroy(None)  # a no-op


# ------------------------------------------------------------------ the C++ mirror
CPP_TU = r'''
#include "crlot_dsp.hpp"
#include <utility>
#include <vector>
int probe(crlot_plan* plan, const float* d_x, float* d_out) {
    std::vector<float> w(80 * 513, 0.0f);
    crlot_mel_filterbank(80, 1024, 16000.0, 0.0, 0.0, CRLOT_MEL_HTK, 0, w.data());
    crlot::Features a(plan, CRLOT_FEAT_POWER, w.data(), 80, CRLOT_FEAT_DB, 1e-10f);
    crlot::Features b(std::move(a));
    a = std::move(b);
    static_assert(!std::is_copy_constructible<crlot::Features>::value, "not copyable");
    a.spectrogram_device(d_x, d_out, 4, 48000, 48000, 188 * 80, 80);
    return a.n_out();
}
'''


def test_cpp_features_class_compiles(tmp_path):
    src = tmp_path / "features_tu.cpp"
    src.write_text(CPP_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
