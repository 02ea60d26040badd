"""crlot::Convolver (include/crlot_dsp.hpp) from a C++ program: tests/cpp/convolve_dropin
convolves padded device rows with convolve_device, checks on its own that the hand
composition through the borrowed plan gives the same bits, and writes y, which must
meet the accuracy bar of tests/test_gpu_convolve.py against np.convolve in float64."""
import os
import subprocess

import numpy as np
import pytest

import convolve_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "convolve_dropin")


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,K,S,nf", [(256, 5 * 256 + 3, 3 * 256 + 7, 3, 2), (512, 511, 1, 1, 1)])
def test_convolve_dropin(tmp_path, torch_cuda, B, T, K, S, nf):
    x, h = CR.make_streams(S, T, B, seed=5), CR.make_filter(nf, K, seed=5)
    xp, hp, yp = tmp_path / "x.f32", tmp_path / "h.f32", tmp_path / "y.f32"
    x.tofile(xp)
    h.tofile(hp)
    if not os.path.exists(EXE):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "convolve_dropin.mk"], check=True)
    r = subprocess.run([EXE, str(xp), str(S), str(T), str(hp), str(nf), str(K), str(B), str(yp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    y = np.fromfile(yp, np.float32).reshape(S, T + K - 1)
    bar_l2, bar_peak = CR.bars()
    for l2, peak in CR.error_figures(y, CR.convolve_f64(x, h)):
        assert l2 <= bar_l2 and peak <= bar_peak, (l2, peak)
