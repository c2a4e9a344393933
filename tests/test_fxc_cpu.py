"""Host side of the linear response of Vxc: the derivative table of the functional bodies (forward-mode differentiation of
csrc/xc_functionals.hpp through g++, response.fxc_table_host) against finite differences of the oracle's pointwise
functionals, and response.fxc_apply_host against the whole-matrix reference of tests/fxc_reference.py.

Pointwise reference, per component k and per variable x in (rho, sigma), with f = vrho or vsigma of
oracle.pointwise(k, rho, sigma, quirks):

    D(d) = (f(x (1 + d)) - f(x (1 - d))) / (2 x d),   R(d) = (4 D(d/2) - D(d)) / 3,   ref = R(2e-3),   bar = |R(4e-3) - R(2e-3)|

Scale of an entry: what it contributes to V1 next to the component's own local term.  For a perturbation of relative
size eta (rho1 = eta rho, sigma1 = eta sigma, g1 = eta g) and orbitals that vary on the density's length scale
(|grad phi| / phi ~ g / rho), the five terms of c0' phi + c_k' d_k phi are P_rho rho, P_sigma sigma, Q_rho sigma,
Q_sigma sigma^2 / rho and Q sigma / rho, all times eta, against u eta with u = |e| + |vrho| of the component (for PBE
correlation: of its PW92 part, which the gradient term cancels at large reduced gradients).  So

    scale(P_rho) = u / rho,  scale(P_sigma) = scale(Q_rho) = u / sigma,  scale(Q_sigma) = u rho / sigma^2,  scale(Q) = u rho / sigma

(|f| / x would be wrong for PBE correlation at large reduced gradients: its vsigma falls to 1e-20 there through a
cancellation of terms fifteen orders larger, so its rounding is not eps |f| and its difference quotient is noise
relative to |f| while being far below anything V1 can see).  The quotient's rounding at d = 1e-3 is 1e-13 of that
scale and the extrapolated truncation term O(d^4) is below it for these smooth bodies: the bar is asserted at 1e-9
(four orders of room) and the table at ten times that.
"""
import numpy as np
import pytest

import fxc_reference as fr
import oracle
from quantum_compute_dft_amd import functionals, response

BAR = 1e-9
COMPONENTS = list(functionals.COMPONENTS)
B88 = COMPONENTS.index("b88_x")


def sample():
    """Log-spaced (rho, sigma), rho in [1e-3, 10], sigma in [1e-6, 10]: away from every cut-off and clamp."""
    r, s = np.meshgrid(np.logspace(-3, 1, 12), np.logspace(-6, 1, 12), indexing="ij")
    return r.ravel(), s.ravel()


def component(k, rho, sigma, quirks):
    """(vrho, vsigma) of component k in the closed-shell form the bodies use it in (B88: per-spin arguments)."""
    if k == B88:
        p = oracle.pointwise(k, 0.5 * rho, 0.25 * sigma, quirks)
        return p[:, 1], 0.5 * p[:, 2]
    p = oracle.pointwise(k, rho, sigma, quirks)
    return p[:, 1], p[:, 2]


def richardson(f, x, d):
    D = lambda h: (f(x * (1.0 + h)) - f(x * (1.0 - h))) / (2.0 * x * h)
    return (4.0 * D(0.5 * d) - D(d)) / 3.0


@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("k", range(8))
def test_component_table_against_oracle_differences(k, quirks):
    rho, sigma = sample()
    gga = k >= 4
    w8 = np.zeros(8); w8[k] = 1.0
    tab = response.fxc_table_host(w8, rho, sigma, bool(quirks))          # P = vrho, Q = 4 vsigma of the unit mix
    vr0, vs0 = component(k, rho, sigma, bool(quirks))
    # PBE correlation is PW92 plus a gradient term that cancels it at large reduced gradients (e and vrho fall to 1e-16 of
    # terms of 1e-2): its magnitude, and its rounding, are those of the PW92 part
    p0 = oracle.pointwise(k, 0.5 * rho, 0.25 * sigma, bool(quirks)) if k == B88 else oracle.pointwise(COMPONENTS.index("pw92_c") if k == COMPONENTS.index("pbe_c") else k, rho, sigma, bool(quirks))
    u = np.abs(p0[:, 0]) + np.abs(p0[:, 1])
    scales = {"P_rho": u / rho, "P_sigma": u / sigma, "Q_rho": u / sigma, "Q_sigma": u * rho / sigma ** 2, "Q": u * rho / sigma}
    worst_bar = worst_err = 0.0
    cases = [("P_rho", 0, 0, 1.0, rho), ("P_sigma", 1, 0, 1.0, sigma), ("Q_rho", 2, 1, 4.0, rho), ("Q_sigma", 3, 1, 4.0, sigma)]
    for name, plane, which, factor, x in cases:
        if not gga and name != "P_rho":
            assert np.all(tab[plane] == 0.0), (COMPONENTS[k], name)
            continue
        wrt_rho = x is rho
        f = lambda v: factor * component(k, v if wrt_rho else rho, sigma if wrt_rho else v, bool(quirks))[which]
        fine, coarse = richardson(f, x, 2e-3), richardson(f, x, 4e-3)
        scale = scales[name]
        bar = np.max(np.abs(fine - coarse) / scale)
        err = np.max(np.abs(tab[plane] - fine) / scale)
        print(f"{COMPONENTS[k]} quirks={quirks} {name}: bar {bar:.2e} err {err:.2e}")
        worst_bar, worst_err = max(worst_bar, bar), max(worst_err, err)
        assert bar <= BAR, (COMPONENTS[k], name, bar)
        assert err <= 10.0 * BAR, (COMPONENTS[k], name, err)
    if gga:
        assert np.max(np.abs(tab[4] - 4.0 * vs0) / scales["Q"]) <= 1e-12     # Q itself: the value part
    else:
        assert np.all(tab[4] == 0.0)
    fr.record("cpu", f"pointwise {COMPONENTS[k]} quirks={quirks} (worst entry, own scale)", worst_bar, worst_err)


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", "PBE0", "BLYP"])
def test_table_is_exactly_zero_below_the_cutoffs(functional):
    rho = np.array([0.0, 1e-300, 9.9e-13, 1e-15, 5e-13])
    sigma = np.array([0.0, 1.0, 1e-3, 1e-30, 1e-10])
    for quirks in (True, False):
        tab = response.fxc_table_host(functional, rho, sigma, quirks)
        assert np.all(tab == 0.0), functional
    # a live density with sigma below ITS cut-off: finite, and the sigma-clamped pieces contribute constants only
    tab = response.fxc_table_host(functional, np.array([0.3, 2.0]), np.array([0.0, 1e-21]), True)
    assert np.all(np.isfinite(tab))
    # B88 returns zeros below the sigma cut-off (per-spin sigma / 4 < 1e-20): nothing of it in the table
    w8 = np.zeros(8); w8[B88] = 1.0
    assert np.all(response.fxc_table_host(w8, np.array([0.3, 2.0]), np.array([0.0, 3.9e-20]), True) == 0.0)


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", "PBE0", "BLYP", "SVWN-RPA", "PW92"])
@pytest.mark.parametrize("quirks", [1, 0])
def test_generic_bodies_reproduce_the_double_bodies_bit_for_bit(functional, quirks):
    """The value parts of the dual evaluation equal the double evaluation, and w P, w Q g_k equal c0..c3 of the point
    bodies the sweep's kernels run (their factors 4 and 2 are powers of two), bit for bit on the sample."""
    rho, sigma = sample()
    rng = np.random.default_rng(5)
    g = rng.standard_normal((rho.size, 3))
    g *= np.sqrt(sigma / np.einsum("gk,gk->g", g, g))[:, None]
    w = 0.05 * rng.random(rho.size) + 0.01
    pq, dual = response.pq_host(functional, rho, sigma, bool(quirks))
    assert np.array_equal(pq, dual)
    pt = response.point_host(functional, rho, sigma, g, w, bool(quirks))
    assert np.array_equal(pt[1], w * pq[0])
    gga = functionals.resolve(functional).needs_gradient
    for k in range(3):
        assert np.array_equal(pt[2 + k], (w * pq[1]) * g[:, k] if gga else np.zeros_like(rho))


@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP"])
def test_fxc_apply_host_against_the_whole_matrix_reference(functional, quirks):
    ngrid, nao, nocc = fr.SHAPES[0]
    dm0, dm1, ao, gr, w = fr.inputs(ngrid, nao, nocc)
    ref, bar = fr.reference(functional, ngrid, nao, nocc, bool(quirks))
    v1 = response.fxc_apply_host(functional, dm0, dm1, ao, w, gr if functional != "LDA" else None, bool(quirks))
    fr.check("cpu", f"fxc_apply_host {functional} quirks={quirks} {fr.SHAPES[0]}", v1, ref, bar)


@pytest.mark.parametrize("functional", ["PBE0", "BLYP"])
def test_fxc_apply_host_mix(functional):
    ngrid, nao, nocc = fr.SHAPES[1]
    dm0, dm1, ao, gr, w = fr.inputs(ngrid, nao, nocc)
    ref, bar = fr.reference(functional, ngrid, nao, nocc, True)
    fr.check("cpu", f"fxc_apply_host {functional} quirks=1 {fr.SHAPES[1]}", response.fxc_apply_host(functional, dm0, dm1, ao, w, gr, True), ref, bar)
