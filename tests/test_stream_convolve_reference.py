"""CPU tests of tests/stream_convolve_reference.py: in one float32 fmaf model the per-hop
state machine of the streaming convolver (ring, partial chain, carry, NULL blocks; zero
rows where the whole-signal chain loads nothing) equals the whole-signal chain of
crlot_convolve bit for bit, on the oracle's kiss_fftr and on numpy's transform; the
flush blocks past F_out are +0; splitting the chain into the partial chain plus the
last term changes nothing; the fmaf model is exactly rounded."""
import numpy as np
import pytest

import convolve_reference as CR
import stream_convolve_reference as SR

CASES = [(128, 1), (128, 2), (128, 3), (128, 5), (256, 4)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def hostile_input(C, F, B, seed):
    """T = F B - 5 samples of CR.make_streams with a NaN, an Inf, a denormal, a value
    below the sanitize threshold and a block of -0."""
    T = F * B - 5
    x = np.array(CR.make_streams(C, T, B, seed))
    x[0, 3] = np.nan
    x[0, B + 1] = np.inf
    x[-1, 2 * B + 7] = np.float32(1e-40)
    x[-1, 2 * B + 8] = np.float32(1e-31)
    x[0, 3 * B:4 * B] = np.float32(-0.0)
    return x


def test_fmaf_is_exactly_rounded():
    rng = np.random.default_rng(7)
    a = rng.standard_normal(20000).astype(np.float32)
    b = rng.standard_normal(20000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(20000) * 1e-7)).astype(np.float32)
    got = SR.fmaf(a, b, c)
    # the exact value a b + c as a ratio of integers, rounded once (Python's Fraction -> float is
    # exact to float64; comparing neighbours in float32 decides the rounding)
    from fractions import Fraction
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = np.float32(got[i])
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        d = abs(Fraction(float(g)) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i
    # cancellation to zero is +0; a -0 product added to +0 is +0
    assert bits(SR.fmaf(np.float32(2), np.float32(3), np.float32(-6)))[()] == 0
    assert bits(SR.fmaf(np.float32(-0.0), np.float32(3), np.float32(0.0)))[()] == 0


@pytest.mark.parametrize("B,P", CASES)
@pytest.mark.parametrize("transform", ["kiss", "numpy"])
def test_hop_machine_equals_the_whole_signal_chain(oracle, B, P, transform):
    C, nf = 3, 2
    F = 2 * P + 3                      # the ring wraps twice
    K = (P - 1) * B + 7 if P > 1 else B - 3
    x = hostile_input(C, F, B, seed=B + P)
    h = CR.make_filter(nf, K, seed=P)
    T = x.shape[1]
    F_out = -(-(T + K - 1) // B)
    if transform == "kiss":
        pair = SR.KissPair(oracle, B)
        fwd, inv = pair.fwd, pair.inv
    else:
        fwd, inv = SR.np_fwd, SR.np_inv
    want = SR.whole_signal(x, h, B, F_out + 2, fwd, inv)
    assert np.any(want[:, (F_out - 1) * B:F_out * B] != 0)
    assert not np.any(bits(want[:, F_out * B:]))          # past F_out: no term, +0
    for split in (True, False):
        m = SR.HopMachine(h, B, C, split=split, fwd=fwd, inv=inv)
        assert m.P == P
        got = SR.run_hops(m, x, F_out + 2)
        assert np.array_equal(bits(got), bits(want)), split
        assert not np.any(bits(got[:, F_out * B:]))       # the two flush blocks past F_out are +0
        # reset, then the same input: the same bits
        m.reset()
        assert np.array_equal(bits(SR.run_hops(m, x, F_out + 2)), bits(want))
    # the model computes the convolution (float32 accuracy against float64)
    y64 = CR.convolve_f64(x, h)
    for l2, peak in CR.error_figures(want[:, :T + K - 1], y64):
        assert l2 <= CR.REL_L2 and peak <= CR.MAX_ABS, (l2, peak)


def test_null_block_mid_stream_is_a_block_of_zeros():
    B, P, C = 128, 3, 2
    h = CR.make_filter(1, (P - 1) * B + 7, seed=1)
    x = np.array(CR.make_streams(C, 8 * B, B, seed=4))
    x[:, 3 * B:4 * B] = 0.0
    a, b = SR.HopMachine(h, B, C), SR.HopMachine(h, B, C)
    for j in range(8):
        blk = x[:, j * B:(j + 1) * B]
        ya = a.push(None if j == 3 else blk)
        yb = b.push(blk)
        assert np.array_equal(bits(ya), bits(yb)), j
