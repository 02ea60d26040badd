"""CPU tests of the phase vocoder's two restatements (tests/phase_vocoder_reference.py):
the float32 / uint32 emulation of the header's contract agrees with the float64
torchaudio recurrence within float32 rounding of each element's own scale, at a
short and at a long recurrence; silence stays exact; rate 1 is the identity; the
frame count is numpy's arange length.  No GPU, no library."""
import numpy as np
import pytest

import phase_vocoder_reference as PV


@pytest.mark.parametrize("rate", PV.RATES)
def test_emulation_vs_float64_short(rate):
    X = PV.spectra(256, 40)
    out = PV.emulate(X, rate)
    assert out.shape == (1, PV.frame_count(40, rate), 129) and out.dtype == np.complex64
    rel, dead = PV.own_scale_error(out, X, rate)
    print(f"N=256 F=40 rate={rate}: worst own-scale error {rel.max():.3g}")
    assert np.all(out[dead] == 0)
    assert dead.any() or rate > 1.0   # (rates up to 1 visit the pair of silent frames)
    assert rel.max() <= 2e-6


@pytest.mark.parametrize("rate", (0.75, 2.0))
def test_emulation_vs_float64_long(rate):
    X = PV.spectra(64, 20000)
    out = PV.emulate(X, rate)
    rel, dead = PV.own_scale_error(out, X, rate)
    print(f"N=64 F=20000 rate={rate}: worst own-scale error {rel.max():.3g}, last 50 frames {rel[:, -50:].max():.3g}")
    assert np.all(out[dead] == 0)
    assert rel.max() <= 5e-5


def test_input_has_the_special_cases():
    X = PV.spectra(256, 40)[0]
    mag = np.abs(X)
    assert np.all(mag[20:22] == 0)                                # silent frames
    assert 0 < mag[7, 5] < 1e-9 and mag[7, 6] > 1e-3              # a quiet column
    assert mag[3].max() > 1e11                                    # a loud frame


def test_rate_one_is_identity():
    X = PV.spectra(256, 40)
    out = PV.emulate(X, 1.0)
    re, im = PV.sanitize(X)
    Xs = re + 1j * im
    own = np.abs(Xs.astype(np.complex128))
    err = np.abs(out.astype(np.complex128) - Xs)
    assert np.all(err[own == 0] == 0)
    worst = (err[own > 0] / own[own > 0]).max()
    print(f"rate 1: worst |emulate - X| / |X| {worst:.3g}")
    assert worst <= 4e-7


def test_frame_count_is_arange_length():
    for F in (1, 2, 7, 40, 1875):
        for rate in (0.1, 1 / 3, 0.5, 0.75, 1, 1.3, 2, 3.7, 7):
            assert PV.frame_count(F, rate) == len(np.arange(0, F, rate)), (F, rate)
    assert PV.frame_count(0, 1.3) == 0
