"""CPU tests of the Griffin-Lim references (tests/griffin_lim_reference.py): the
float32 restatement of the projection against the float64 one, and the two
convergence conditions the device is held to, on the float64 recurrence.

The convergence conditions are Griffin and Lim's, so they are about the
least-squares inverse: a plan whose norm table is sum(w^2) (GL.ls_norm32,
Plan.upload_tables(norm=...)).  A default plan divides by the reference's
sum(w) table instead; its recurrence is the same one scaled by
sum(w^2) / sum(w) per sample (the projection only reads phases), so its spectral
convergence settles near 1 - sum(w^2) / sum(w) instead of falling to 0.  Measured
here with the default table: SC(y_32) / SC(y_0) = 0.45 - 0.61 at momentum 0.99;
with the least-squares table 0.06 - 0.18 (printed by the tests below).
"""
import functools

import numpy as np
import pytest

import griffin_lim_reference as GL


# ------------------------------------------------------------------ project32 against project64
def test_project32_matches_project64_within_its_rounding():
    """Bound.  u = 2^-24.  With a = fl32(alpha) = alpha (1 + d0), |d0| <= u:
        fl(a t) = alpha t (1 + d0)(1 + d1)            |error| <= 2 u alpha |t|
        c = fl(x - fl(a t))                           |error| <= 2 u alpha |t| + u |c|
    per component, so as vectors |dc| <= u (2 alpha |T| + |c|) <= 2 u kappa |c| with
    kappa = (|X| + alpha |T|) / |c| >= 1 (|c| <= |X| + alpha |T|).  The result is
    m c / (|c| + 1e-16): an error dc of c moves c / |c| by at most |dc| / |c| and
    leaves the length m |c| / (|c| + 1e-16) <= m alone to first order.  The rest is
    five roundings on the way to each output component: p (the squares and the sum:
    2 u on p, u on sqrt(p)), the sqrt, the + 1e-16, the division, the product: 5 u.
    One more u covers the second-order terms (kappa u << 1 for the kappa <= 2^12
    kept here).  So |out32 - out64| <= u |m| (6 + 2 kappa) per element."""
    rng = np.random.default_rng(11)
    S, F, bins = 3, 40, 129
    X = (rng.standard_normal((S, F, bins)) + 1j * rng.standard_normal((S, F, bins))).astype(np.complex64)
    T = (rng.standard_normal((S, F, bins)) + 1j * rng.standard_normal((S, F, bins))).astype(np.complex64)
    mag = np.abs(rng.standard_normal((S, F, bins))).astype(np.float32)
    for momentum in (0.0, 0.5, 0.99):
        a = momentum / (1.0 + momentum)
        Tm = T.copy()
        if momentum > 0:  # stream 2: near cancellation, X = alpha T (1 + 2^-8 z)
            z = (rng.standard_normal((F, bins)) + 1j * rng.standard_normal((F, bins))) * 2.0 ** -8
            Tm[2] = (X[2] / a / (1 + z)).astype(np.complex64)
        for Tuse in (None, Tm):
            o32 = GL.project32(X, mag, Tuse, momentum).astype(np.complex128)
            o64 = GL.project64(X, mag, Tuse, momentum)
            kappa = GL.conditioning(X, Tuse, momentum)
            ok = kappa <= 2.0 ** 12
            assert ok.mean() > 0.99
            err = np.abs(o32 - o64)
            bound = GL.U32 * mag.astype(np.float64) * (6 + 2 * kappa)
            worst = float(np.max(err[ok] / np.maximum(bound[ok], 1e-300)))
            print(f"momentum {momentum} tprev {Tuse is not None}: worst error / bound {worst:.3f}, "
                  f"largest kappa kept {kappa[ok].max():.1f}")
            assert np.all(err[ok] <= bound[ok])
            assert np.all(o32.imag[..., 0] == 0) and np.all(o32.imag[..., -1] == 0)


def test_project32_sanitizes_and_keeps_the_sign_of_mag():
    bins = 9
    X = np.ones((1, 2, bins), np.complex64) * (3 + 4j)
    X[0, 0, 2] = np.nan + 1j
    X[0, 0, 3] = 1e-31 + 1e-31j
    X[0, 0, 4] = np.inf
    mag = np.full((1, 2, bins), 2.0, np.float32)
    mag[0, 1] = -2.0
    mag[0, 0, 5] = np.nan
    out = GL.project32(X, mag)
    assert out[0, 0, 1] == np.complex64(1.2 + 1.6j)
    assert out[0, 0, 2] == np.complex64(2j)            # NaN real part -> 0
    assert out[0, 0, 3] == 0 and out[0, 0, 4] == 0 and out[0, 0, 5] == 0
    assert out[0, 1, 1] == np.complex64(-1.2 - 1.6j)
    assert out[0, 0, 0] == 2 and out[0, 0, -1] == 2    # bins 0 and N/2: the real part alone
    assert np.all(np.isfinite(out.view(np.float32)))


# ------------------------------------------------------------------ convergence in float64
@functools.lru_cache(maxsize=None)
def case(n, h, with_init):
    x = GL.make_signal(n, h)
    mag = GL.target_mag(x, n, h)
    mag.setflags(write=False)
    init = GL.random_phase_init(mag.shape) if with_init else None
    return mag, init


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("n,h", GL.SHAPES)
def test_spectral_convergence_never_increases_at_momentum_0(n, h, with_init):
    """Griffin and Lim's theorem, over 32 iterations, with the least-squares table."""
    mag, init = case(n, h, with_init)
    ys = GL.griffin_lim_f64(mag, n, h, 32, 0.0, init, ls=True, trace=True)
    sc = np.array([GL.spectral_convergence(y, mag, n, h) for y in ys])
    print(f"{n}/{h} init {with_init}: SC {sc[0]:.4f} -> {sc[-1]:.4f}, largest step {np.diff(sc).max():.3g}")
    assert np.all(np.diff(sc) <= 0)


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("n,h", GL.SHAPES)
def test_momentum_reaches_a_quarter_in_32_iterations(n, h, with_init):
    mag, init = case(n, h, with_init)
    sc0 = GL.spectral_convergence(GL.griffin_lim_f64(mag, n, h, 0, 0.99, init, ls=True), mag, n, h)
    sc32 = GL.spectral_convergence(GL.griffin_lim_f64(mag, n, h, 32, 0.99, init, ls=True), mag, n, h)
    dflt = [GL.spectral_convergence(GL.griffin_lim_f64(mag, n, h, k, 0.99, init), mag, n, h) for k in (0, 32)]
    print(f"{n}/{h} init {with_init}: SC(y_32) / SC(y_0) = {sc32 / sc0:.3f} "
          f"(default sum(w) table: {dflt[1] / dflt[0]:.3f})")
    assert sc32 <= 0.25 * sc0


def test_ls_norm_is_the_sum_of_squares():
    n, h = 1024, 256
    w = GL.R.window32(n).astype(np.float64)
    tbl = GL.ls_norm32(n, h)
    assert tbl.size == GL.R.O.ring_len(n, h)
    i = 300
    assert abs(tbl[i] - sum(w[(i % h) + j] ** 2 for j in range(0, n, h))) < 1e-6
    # with it the round trip of the interior is the identity (to float64 rounding)
    x = GL.make_signal(n, h).astype(np.float64)
    y = GL.istft_f64(GL.R.stft_f64(x, n, h), n, h, ls=True)
    assert np.max(np.abs(y[n:-n] - x[n:-n])) < 1e-6
