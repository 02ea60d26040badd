"""CPU tests of tests/convolve_reference.py: the partitioned algorithm in float64 equals
np.convolve to float64 rounding at every block edge case, the chain lengths and the
error scales are what the contract says, and convolve_oracle_f32's own error on the
GPU test's inputs -- the yardstick of tests/test_gpu_convolve.py's accuracy bars."""
import numpy as np
import pytest

import convolve_reference as CR

B = 128


@pytest.mark.parametrize("K", [1, B - 1, B, B + 1, 3 * B + 7])
@pytest.mark.parametrize("T", [1, B - 1, B, B + 1, 5 * B + 3])
def test_partitioned_f64_equals_np_convolve(K, T):
    x = CR.make_streams(3, T, B, seed=K)
    h = CR.make_filter(2, K, seed=T)
    H = CR.partition_f64(h, B)
    P, F_in, L = -(-K // B), -(-T // B), T + K - 1
    F_out = -(-L // B)
    assert H.shape == (2, P, B + 1)
    xp = np.zeros((3, F_in * B))
    xp[:, :T] = x
    blocks = np.concatenate([xp.reshape(3, F_in, B), np.zeros((3, F_in, B))], axis=-1)
    X = np.fft.rfft(blocks, axis=-1)
    Y, sr, si = CR.fdl_mac_f64(X, H, F_out)
    y = CR.overlap_add_f64(Y, B, L)
    want = CR.convolve_f64(x, h)
    assert y.shape == want.shape == (3, L)
    # float64 rounding: 2B-point transforms and sums of P terms, relative to the largest output
    tol = 64 * np.finfo(np.float64).eps * max(1.0, np.log2(2 * B)) * P * np.max(np.abs(want)) + 1e-300
    assert np.max(np.abs(y - want)) <= tol, (np.max(np.abs(y - want)), tol)


def test_chain_terms_and_scales():
    assert CR.chain_terms(4, 3, 6).tolist() == [1, 2, 3, 3, 2, 1]
    assert CR.chain_terms(4, 3, 8).tolist() == [1, 2, 3, 3, 2, 1, 0, 0]
    assert CR.chain_terms(4, 1, 3).tolist() == [1, 1, 1]
    assert CR.chain_terms(2, 5, 6).tolist() == [1, 2, 2, 2, 2, 1]
    rng = np.random.default_rng(0)
    X = rng.standard_normal((2, 4, 5)) + 1j * rng.standard_normal((2, 4, 5))
    H = rng.standard_normal((2, 3, 5)) + 1j * rng.standard_normal((2, 3, 5))
    Y, sr, si = CR.fdl_mac_f64(X, H, 8)
    for s in range(2):
        for f in range(8):
            terms = [(H[s % 2, f - j], X[s, j]) for j in range(max(0, f - 2), min(f, 3) + 1)]
            assert np.allclose(Y[s, f], sum(h * x for h, x in terms) if terms else 0)
            want_r = sum(np.abs(h.real * x.real) + np.abs(h.imag * x.imag) for h, x in terms) if terms else 0
            want_i = sum(np.abs(h.real * x.imag) + np.abs(h.imag * x.real) for h, x in terms) if terms else 0
            assert np.allclose(sr[s, f], want_r) and np.allclose(si[s, f], want_i)
    assert CR.fma_bound(8) == 8 * 2.0 ** -24 / (1 - 8 * 2.0 ** -24)


def test_inputs_have_a_silent_block_and_a_level_step():
    x = CR.make_streams(3, 9 * B + 3, B)
    for s in range(3):
        assert not np.any(x[s, (s + 1) * B:(s + 2) * B]) and np.any(x[s, (s + 2) * B:(s + 3) * B])
        t = (2 * x.shape[1]) // 3
        assert np.max(np.abs(x[s, t:])) > 2.0 ** 10 * np.max(np.abs(x[s, :t]))
    z = np.array([np.nan, np.inf, 1e-31, -2.0, 0.0], np.float32)
    assert CR.sanitize(z).tolist() == [0.0, 0.0, 0.0, -2.0, 0.0]
    assert np.array_equal(CR.convolve_f64(z, [1.0, 0.5])[0], [0.0, 0.0, 0.0, -2.0, -1.0, 0.0])


@pytest.mark.parametrize("case", CR.ACCURACY_CASES, ids=lambda c: "B%d_T%d_K%d_S%d_nf%d" % c)
def test_oracle_f32_error_on_the_gpu_inputs(oracle, case, capsys):
    """The float32 CPU program's own error against np.convolve in float64 on the GPU
    test's inputs, per stream (rel-L2, max-abs over max|y64|), printed by every run.
    Recorded: B = 128, P = 37: rel-L2 1.98e-7 - 2.00e-7, peak 1.83e-7 - 2.46e-7;
    B = 512, P = 4: rel-L2 2.00e-7 - 2.12e-7, peak 1.74e-7 - 2.49e-7; B = 256, P = 2:
    rel-L2 2.05e-7, peak 1.85e-7.  Four times these stays below the project's
    1e-6 / 4e-6, so those are the device's bars on these inputs."""
    Bc, T, K, S, nf = case
    x = CR.make_streams(S, T, Bc)
    h = CR.make_filter(nf, K)
    y = CR.convolve_oracle_f32(oracle, x, h, Bc)
    y64 = CR.convolve_f64(x, h)
    assert y.shape == y64.shape == (S, T + K - 1) and y.dtype == np.float32
    figs = CR.error_figures(y, y64)
    with capsys.disabled():
        print("\noracle f32", case, " ".join("(%.2e, %.2e)" % f for f in figs))
    # a float32 program of 2B-point transforms and P-term chains: a few ulp per stage
    for l2, peak in figs:
        assert 0 < l2 < 1e-6 and 0 < peak < 4e-6, figs
    assert CR.bars(*figs[0]) == (CR.REL_L2, CR.MAX_ABS)
    assert CR.bars(1e-6, 2e-6) == (4e-6, 8e-6)
