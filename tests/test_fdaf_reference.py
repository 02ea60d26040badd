"""CPU tests of tests/fdaf_reference.py (the adaptive filter's contract, include/crlot_dsp.h
"adaptive filter"): the float64 model identifies a K-tap system to -120 dB with the
gradient constraint (round-robin or every partition) and stays above -40 dB without it
once P >= 3 (the wrap-around of the unconstrained update is real); the float32 model
follows it; a NULL reference block is a block of zeros; reset reproduces a run; with
adaptation off and taps set, y is the convolution; the float32 steps are consistent
with the float64 ones."""
import numpy as np
import pytest

import fdaf_reference as FR
import stream_convolve_reference as SR

SHAPES = [(128, 1), (128, 3), (128, 5), (256, 4)]
HOPS = 200


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_cases = {}


def case(B, P):
    """One identification problem per shape, computed once and shared."""
    if (B, P) not in _cases:
        _cases[(B, P)] = FR.make_case(B, P, HOPS, seed=1000 * B + P)
    return _cases[(B, P)]


def misalignment(B, P, mode, cls=FR.F64Model):
    x, h, d = case(B, P)
    m = cls(B, P * B - 5, 1, mu=1.0, lam=0.9, delta=1e-3, mode=mode)
    FR.run(m, x, d)
    return FR.misalignment_db(m.taps(), h)


@pytest.mark.parametrize("B,P", SHAPES)
def test_float64_model_converges_with_the_constraint(B, P):
    for mode in (1, 2):
        db = misalignment(B, P, mode)
        print(f"B {B} P {P} mode {mode}: {db:.1f} dB")
        assert db <= -120.0, (mode, db)


@pytest.mark.parametrize("B,P", [s for s in SHAPES if s[1] >= 3])
def test_float64_model_without_the_constraint_does_not(B, P):
    db = misalignment(B, P, 0)
    print(f"B {B} P {P} mode 0: {db:.1f} dB")
    assert db > -40.0, db


@pytest.mark.parametrize("B,P", [(128, 1), (128, 3)])
def test_float32_model_follows(B, P):
    """float32 steps on numpy's transform: the float32 floor, far below any use."""
    db = misalignment(B, P, 1, FR.F32Model)
    print(f"B {B} P {P} float32 mode 1: {db:.1f} dB")
    assert db <= -120.0, db


def test_null_block_is_a_block_of_zeros():
    B, P, C = 128, 3, 2
    x, _, d = FR.make_case(B, P, 8, seed=5, channels=C)
    x[:, 3 * B:4 * B] = 0.0
    for cls in (FR.F64Model, FR.F32Model):
        a, b = cls(B, P * B - 5, C, mu=1.0), cls(B, P * B - 5, C, mu=1.0)
        for j in range(8):
            xb, db = x[:, j * B:(j + 1) * B], d[:, j * B:(j + 1) * B]
            ea, ya = a.push(None if j == 3 else xb, db)
            eb, yb = b.push(xb, db)
            assert np.array_equal(ea, eb) and np.array_equal(ya, yb), j
        assert np.array_equal(a.W, b.W)


def test_reset_reproduces_a_run():
    B, P, C = 128, 2, 2
    x, _, d = FR.make_case(B, P, 7, seed=6, channels=C)
    m = FR.F32Model(B, P * B - 5, C, mu=1.0, mode=1)
    e1, y1 = FR.run(m, x, d)
    w1 = m.W.copy()
    m.reset()
    assert not np.any(m.W) and m.k == 0
    e2, y2 = FR.run(m, x, d)
    assert np.array_equal(bits(e1), bits(e2)) and np.array_equal(bits(y1), bits(y2))
    assert np.array_equal(w1, m.W)


@pytest.mark.parametrize("B,P", [(128, 1), (128, 3), (256, 4)])
def test_frozen_filter_is_the_convolution(B, P):
    C, hops = 2, 2 * P + 3
    x, h, d = FR.make_case(B, P, hops, seed=B + P, channels=C)
    m = FR.F64Model(B, P * B - 5, C, adapt=False)
    m.set_taps(h)
    w0 = m.W.copy()
    e, y = FR.run(m, x, d)
    assert np.array_equal(w0, m.W)
    # d is rounded to float32 on the way in, y is not
    assert np.max(np.abs(y - d)) <= 1e-12 * np.max(np.abs(d))
    assert np.max(np.abs(e)) <= 2.0 ** -23 * np.max(np.abs(d))
    assert np.max(np.abs(m.taps() - h)) <= 1e-14
    f = FR.F32Model(B, P * B - 5, C, adapt=False)
    f.set_taps(h)
    _, y32 = FR.run(f, x, d)
    rel = np.linalg.norm(y32 - d, axis=1) / np.linalg.norm(d, axis=1)
    assert np.all(rel <= 1e-6), rel


def test_float32_steps_agree_with_float64():
    """chain, power, gradient and update against the same expressions in float64."""
    rng = np.random.default_rng(3)
    P, bins = 4, 129

    def spec(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)

    W, ring, E = spec(2, P, bins), spec(2, P, bins), spec(2, bins)
    cst = FR.constants(1.0, 0.9, 1e-3, P)
    assert cst[0] == np.float32(0.25) and cst[2] == np.float32(1.0 - 0.9) and cst[2] != np.float32(1.0) - np.float32(0.9)
    for k in (0, 2, 9):
        Y = FR.chain(W, ring, k)
        want = sum(W[:, k - j].astype(np.complex128) * ring[:, j % P] for j in range(max(0, k - P + 1), k + 1))
        assert np.max(np.abs(Y - want)) <= 1e-5
        pw0 = np.abs(rng.standard_normal((2, bins))).astype(np.float32)
        pw = FR.power(pw0, ring[:, k % P], k, cst)
        m = np.abs(ring[:, k % P].astype(np.complex128)) ** 2
        assert np.allclose(pw, m if k == 0 else 0.9 * pw0 + 0.1 * m, rtol=1e-6)
        G = FR.gradient(pw, E, cst)
        assert np.allclose(G, 0.25 / (pw.astype(np.float64) + 1e-3) * E, rtol=1e-6)
        W2 = FR.update(W, ring, G, k)
        for p in range(P):
            if p > k:
                assert np.array_equal(W2[:, p], W[:, p])
            else:
                want = W[:, p].astype(np.complex128) + np.conj(ring[:, (k - p) % P].astype(np.complex128)) * G
                assert np.max(np.abs(W2[:, p] - want)) <= 1e-5
    # the update is the contract's four fmaf, in order, on one bin
    x, g, w = np.complex64(1.5 - 0.25j), np.complex64(0.75 + 2.0j), np.complex64(3.0 - 1.0j)
    out = FR.update(np.full((1, 1), w), np.full((1, 1), x), np.full((1,), g), 0)[0, 0]
    re = SR.fmaf(x.imag, g.imag, SR.fmaf(x.real, g.real, w.real))
    im = SR.fmaf(-x.imag, g.real, SR.fmaf(x.real, g.imag, w.imag))
    assert out.real == re and out.imag == im
