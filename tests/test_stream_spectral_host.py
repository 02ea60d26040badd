"""Host-side surface of the per-hop spectral entries (no GPU): the C names are
declared and exported, pkg.Stream carries the methods, and crlot::SpectralStream
(include/crlot_dsp.hpp) compiles with every member instantiated."""
import os
import re
import subprocess

NAMES = ["crlot_stream_stft_hop", "crlot_stream_istft_hop", "crlot_stream_push_hop_masked"]

SPECTRAL_TU = r'''
#include "crlot_dsp.hpp"
// every member of crlot::SpectralStream, used as a caller would
size_t probe(const crlot::StftEngine& eng, const float* d_hop, float* d_out, float* d_spec, const float* d_mask,
             void* stream) {
    crlot::SpectralStream whole(eng, 2, true), split(eng, 2);
    const int64_t ld_spec = 1026, ld_mask = 513;
    size_t n = whole.push_hop(d_hop, d_out, stream);
    n += whole.push_hop_masked(d_hop, d_mask, ld_mask, d_out, stream);
    n += whole.push_hop_masked(d_hop, nullptr, 0, d_out);
    n += split.stft_hop(d_hop, d_spec, ld_spec, stream);
    split.istft_hop(d_spec, ld_spec, d_mask, 0, d_out, stream);
    split.istft_hop(d_spec, ld_spec, nullptr, 0, d_out);
    whole.reset();
    split.reset();
    crlot_stream* h = whole.handle();
    (void)h;
    static_assert(!std::is_copy_constructible<crlot::SpectralStream>::value, "single owner");
    return n;
}
'''


def test_names_declared_and_exported(pkg):
    syms = pkg.header_symbols()
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\b(crlot_[a-z0-9_]+)\b", out))
    for name in NAMES:
        assert name in syms, name
        assert name in exported, name
        assert getattr(L, name).argtypes, name  # bound with a signature
    assert L.crlot_abi_version() == 2  # additive entries: the version stays


def test_stream_has_the_methods(pkg):
    for name in ("stft_hop", "istft_hop", "push_hop_masked"):
        assert callable(getattr(pkg.Stream, name, None)), name


def test_spectral_stream_compiles(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "spectral_tu.cpp"
    src.write_text(SPECTRAL_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(root, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
