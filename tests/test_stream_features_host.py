"""Host-side surface of the per-hop feature entry (no GPU): crlot_stream_features_hop
is declared, exported and bound; pkg.Stream.features_hop exists; the binding's
layout helper accepts the good description and refuses each description that
differs from it in exactly one thing; the C entry refuses a null object before it
touches a device; crlot::SpectralStream::features_hop compiles with and without a
spectrum."""
import ctypes
import os
import re
import subprocess

import pytest

NAME = "crlot_stream_features_hop"

FEATURES_TU = r'''
#include "crlot_dsp.hpp"
size_t probe(const crlot::StftEngine& eng, const crlot::Features& f, const float* d_hop, float* d_feat,
             float* d_spec, void* stream) {
    crlot::SpectralStream st(eng, 2);
    const int64_t ld_feat = 80, ld_spec = 1026;
    size_t n = st.features_hop(f, d_hop, d_feat, ld_feat);                             // no spectrum
    n += st.features_hop(f, d_hop, d_feat, ld_feat, nullptr, 0, stream);
    n += st.features_hop(f, d_hop, d_feat, ld_feat, d_spec, ld_spec);                  // with the spectrum row
    n += st.features_hop(f, d_hop, d_feat, ld_feat, d_spec, ld_spec, stream);
    n += st.stft_hop(d_hop, d_spec, ld_spec, stream);                                  // the same counter
    st.istft_hop(d_spec, ld_spec, nullptr, 0, d_feat, stream);
    return n;
}
'''


def test_name_declared_exported_and_bound(pkg):
    L = pkg.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\b(crlot_[a-z0-9_]+)\b", out))
    assert NAME in pkg.header_symbols()
    assert NAME in exported
    assert len(getattr(L, NAME).argtypes) == 9  # bound with a signature
    assert L.crlot_abi_version() == 2           # an additive entry: the version stays


def test_stream_has_the_method(pkg):
    assert callable(getattr(pkg.Stream, "features_hop", None))


def test_layout_helper(pkg):
    """(C, n_out) float32 device rows, last stride 1, row stride >= n_out, same plan."""
    C_, n_out = 5, 80
    lay = pkg._features_hop_out_layout
    good = dict(shape=(C_, n_out), strides=(n_out, 1), dtype="float32", device_index=0, channels=C_, n_out=n_out,
                same_plan=True)
    assert lay(**good) == n_out
    assert lay(**{**good, "strides": (n_out + 7, 1)}) == n_out + 7  # padded rows
    # one channel: its row stride is meaningless
    assert lay(**{**good, "shape": (1, n_out), "strides": (3, 1), "channels": 1}) == n_out
    bad = {
        "dtype": {"dtype": "float64"},
        "dtype16": {"dtype": "float16"},
        "cpu": {"device_index": None},
        "bins": {"shape": (C_, n_out + 1)},
        "channels": {"shape": (C_ - 1, n_out)},
        "rank": {"shape": (1, C_, n_out), "strides": (C_ * n_out, n_out, 1)},
        "row stride": {"strides": (n_out - 1, 1)},
        "last stride": {"strides": (2 * n_out, 2)},
        "transposed": {"strides": (1, C_)},
        "plan": {"same_plan": False},
    }
    for what, change in bad.items():
        try:
            lay(**{**good, **change})
        except ValueError:
            continue
        pytest.fail(f"accepted a description with a wrong {what}")


def test_null_stream_is_einval(pkg):
    L = pkg.lib()
    em = ctypes.c_int32(7)
    rc = L.crlot_stream_features_hop(None, None, None, None, 0, None, 0, ctypes.byref(em), None)
    assert rc == pkg.EINVAL
    assert em.value == 0
    with pytest.raises(ValueError):
        pkg._check(rc)


def test_features_hop_compiles(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "features_tu.cpp"
    src.write_text(FEATURES_TU)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I" + os.path.join(root, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
