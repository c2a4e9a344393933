"""Host side of the triplet (spin-flip) response: the spin-resolved energy bodies of csrc/xc_spin_functionals.hpp through
g++ (response.fxc_table_host(kind=...), response.spin_energy_host), the triplet operators of excitations.py on H2O / STO-3G,
and the C-ABI's new symbols.  Helpers and references: tests/triplet_reference.py.

Bars.  Figures are relative to the largest entry of the plane compared unless said otherwise; profiles/triplet_parity.txt
holds what was measured on the host (QCDFT_WRITE_PROFILES=profiles rewrites it).

* GOLDEN_BAR, host table and energies against the 60-digit reference: measured worst 6.4e-13 (pbe_c, kind 2, Q: the
  uniform-gas part and H cancel at large reduced gradients), bar ten times that.  A wrong constant or term moves an
  entry by 1e-6 or more: PBE exchange with mu = beta pi^2 / 3 at beta = 0.066725 instead of the 0.2195149727645171 the
  closed-shell body carries (beta = 0.06672455) differs by 6e-6.
* SINGLET_BAR, kind 2 against the shipped singlet table at quirks = 0: a hundred times the measured worst, but never
  looser than 1e-9.  Measured worst 9.5e-11 (GGA, planes Q_rho and Q at rho = 1e-12, where the gradient terms of PBE
  exchange and correlation cancel to 1e-5 of their size and both tables round at 1e-16 of the terms); the other
  functionals 2e-15 .. 7e-14.  A hundred times 9.5e-11 is looser than 1e-9, so the bar is 1e-9.
* DIFF_BAR / DIFF_ERR, the table against extrapolated differences of the energy: the bound of tests/test_fxc_cpu.py
  (reference's own bar 1e-9, the table at ten times that), derived the same way one derivative order up: the mixed
  second difference of the energy needs a second extrapolation to get there (one leaves a d^4 term of 3e-9 .. 5e-8 at
  d = 8e-3 for the gradient components at reduced gradients of 1e3, and a smaller step rounds at eps / d^2 > 1e-10):
  steps 1e-2, 5e-3, 2.5e-3, the d^2 and d^4 terms removed; the bar is the difference to the same from 2e-2.  Rounding
  at the smallest step, eps / d^2 = 2e-11 times the weights of the two extrapolations (about ten): 2e-10; measured
  bars 1e-12 .. 3.1e-10.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import triplet_reference as tr
from quantum_compute_dft_amd import excitations as ex
from quantum_compute_dft_amd import functionals, inputs, response, scf
import excitation_dense as ed

GOLDEN_BAR = 6.4e-12
SINGLET_BAR = 1e-9
DIFF_BAR, DIFF_ERR = 1e-9, 1e-8
COMPONENTS = tr.COMPONENTS
LDA_C = [COMPONENTS.index(n) for n in ("vwn5_c", "vwn_rpa_c", "pw92_c")]
MIX = "0.5*pbe_x+0.3*b88_x+0.7*lyp_c+0.2*pw92_c+0.4*pbe_c+0.1*vwn5_c+0.25*slater_x+0.15*vwn_rpa_c"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def natural_scales(t0, rho, sigma):
    """Pointwise magnitudes of T1..T4 from T0 = O(e / rho^2): what an analytically vanishing plane is held against."""
    a = np.abs(t0)
    return [a, a * rho / sigma, a * rho / sigma, a * rho ** 2 / sigma ** 2, a * rho ** 2 / sigma]


# ---- 1. the independent 60-digit reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2], ids=["triplet", "singlet"])
@pytest.mark.parametrize("k", range(8))
def test_host_table_against_the_high_precision_reference(k, kind):
    g = tr.golden()
    rho, sigma = g["rho"], g["sigma"]
    assert rho.size == 24 and np.all(sigma > 1e-20)
    ref = g[f"{COMPONENTS[k]}_kind{kind}"]
    tab = response.fxc_table_host(tr.unit(k), rho, sigma, kind=kind)
    assert np.all(np.isfinite(tab))
    worst = 0.0
    for p in range(5):
        if k < 4 and p > 0:
            assert np.all(tab[p] == 0.0) and np.all(ref[p] == 0.0)        # no gradient in an LDA component
            continue
        top = np.abs(ref[p]).max()
        if top <= 1e-30 * natural_scales(ref[0], rho, sigma)[p].max():     # vanishes analytically (LYP is linear in sigma;
            err = np.max(np.abs(tab[p]) / natural_scales(ref[0], rho, sigma)[p])   # PBE correlation sees the total sigma only)
        else:
            err = np.abs(tab[p] - ref[p]).max() / top
        print(f"{COMPONENTS[k]} kind {kind} T{p}: {err:.2e}")
        worst = max(worst, err)
    tr.record(f"cpu host table against 60 digits, {COMPONENTS[k]} kind {kind}", worst, GOLDEN_BAR)
    assert worst <= GOLDEN_BAR, (COMPONENTS[k], kind, worst)


@pytest.mark.parametrize("k", range(8))
def test_host_energy_against_the_high_precision_reference(k):
    """zeta = 0, 0.3 and 1, per point relative to the magnitude of the component there (PBE correlation: of its uniform-gas
    part, which the gradient term cancels at large reduced gradients)."""
    g = tr.golden()
    rho, sigma = g["rho"], g["sigma"]
    ref = g[f"{COMPONENTS[k]}_energy"]
    mag = np.abs(g["pw92_c_energy"][0]) if COMPONENTS[k] == "pbe_c" else np.abs(ref[0])
    worst = 0.0
    for iz, z in enumerate(g["zetas"]):
        e = response.spin_energy_host(tr.unit(k), *tr.polarised(rho, sigma, z))
        worst = max(worst, float(np.max(np.abs(e - ref[iz]) / mag)))
    print(f"{COMPONENTS[k]} energy: {worst:.2e}")
    tr.record(f"cpu host energy against 60 digits, {COMPONENTS[k]} (per point)", worst, GOLDEN_BAR)
    assert worst <= GOLDEN_BAR, (COMPONENTS[k], worst)


# ---- 2. the singlet through the spin bodies ----------------------------------------------------------------------------
def random_points(n=2000, seed=0):
    """rho log-uniform in [1e-8, 100], reduced gradient uniform in [0, 3]; 100 points at sigma = 0 and 100 just above it
    (below the sigma cut-off at small rho), 20 points below the density cut-off.  B88 enters the closed-shell bodies with
    per-spin arguments (rho / 2, sigma / 4), so ITS cut-offs sit at rho = 2e-12 and sigma = 4e-20: 40 points with rho in
    [1e-12, 2e-12) and 60 with sigma in [1e-20, 4e-20), between the cut-offs of B88 and those of the other components."""
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-8, 2, n)
    s = rng.uniform(0, 3, n)
    s[:100] = 0.0
    s[100:200] *= 1e-3
    rho[:20] = 10.0 ** rng.uniform(-14, -12.1, 20)
    rho[200:240] = rng.uniform(1.0e-12, 2.0e-12, 40)
    sigma = (2.0 * np.cbrt(3.0 * np.pi ** 2 * rho) * rho * s) ** 2
    sigma[240:300] = rng.uniform(1.0e-20, 4.0e-20, 60)
    assert 100 < np.count_nonzero(sigma <= 1e-20) < 300 and np.count_nonzero(rho < 1e-12) == 20
    assert np.count_nonzero((rho >= 1e-12) & (rho < 2e-12)) >= 40 and np.count_nonzero((sigma >= 1e-20) & (sigma < 4e-20)) >= 60
    return rho, sigma


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", "BLYP", "PBE0", MIX])
def test_kind_two_reproduces_the_shipped_singlet_table(functional):
    rho, sigma = random_points()
    a = response.fxc_table_host(functional, rho, sigma, quirks=False)
    b = response.fxc_table_host(functional, rho, sigma, kind="singlet-spin")
    assert np.all(b[:, rho < 1e-12] == 0.0)
    worst = 0.0
    for p in range(5):
        top = np.abs(a[p]).max()
        if top == 0.0:
            assert np.all(b[p] == 0.0)
            continue
        worst = max(worst, float(np.abs(a[p] - b[p]).max() / top))
    print(f"{functional}: kind 2 against the singlet table {worst:.2e}")
    tr.record(f"cpu kind 2 against the shipped singlet table at quirks 0, {functional[:24]}", worst, SINGLET_BAR)
    assert worst <= SINGLET_BAR, (functional, worst)
    # and it does not care about quirks
    assert np.array_equal(b, response.fxc_table_host(functional, rho, sigma, quirks=True, kind=2))


# ---- 3. limits that touch zeta != 0 ------------------------------------------------------------------------------------
def _vwn_fit(x, A, b, c, x0):
    X = lambda y: y * y + b * y + c
    Q = np.sqrt(4.0 * c - b * b)
    at = np.arctan(Q / (2.0 * x + b))
    return A * (np.log(x * x / X(x)) + 2.0 * b / Q * at - b * x0 / X(x0) * (np.log((x - x0) ** 2 / X(x)) + 2.0 * (b + 2.0 * x0) / Q * at))


def _pw92_g(rs, A, a1, b1, b2, b3, b4):
    return -2.0 * A * (1.0 + a1 * rs) * np.log(1.0 + 1.0 / (2.0 * A * (b1 * np.sqrt(rs) + b2 * rs + b3 * rs ** 1.5 + b4 * rs ** 2)))


A_ALPHA = -1.0 / (6.0 * np.pi ** 2)
FERRO = {"vwn5_c": lambda rs: _vwn_fit(np.sqrt(rs), 0.01554535, 7.06042, 18.0578, -0.32500),
         "vwn_rpa_c": lambda rs: _vwn_fit(np.sqrt(rs), 0.01554535, 20.1231, 101.578, -0.743294),
         "pw92_c": lambda rs: _pw92_g(rs, 0.01554534543482744751, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517)}
STIFFNESS = {"vwn5_c": lambda rs: _vwn_fit(np.sqrt(rs), A_ALPHA, 1.13107, 13.0045, -0.0047584),
             "vwn_rpa_c": lambda rs: _vwn_fit(np.sqrt(rs), A_ALPHA, 1.06835, 11.4813, -0.228344),
             "pw92_c": lambda rs: -_pw92_g(rs, 0.01688686394038962731, 0.11125, 10.357, 3.6231, 0.88026, 0.49671)}
RHO_LINE = np.logspace(-6, 2, 33)


def test_lyp_vanishes_without_a_second_spin_density():
    ra = RHO_LINE
    saa = (2.0 * np.cbrt(3.0 * np.pi ** 2 * ra) * ra * 0.7) ** 2
    z = np.zeros_like(ra)
    assert np.all(response.spin_energy_host("1.0*lyp_c", ra, z, saa, z, z) == 0.0)
    assert np.all(response.spin_energy_host("1.0*lyp_c", ra, ra, saa, saa, saa) < 0.0)


@pytest.mark.parametrize("zeta", [0.0, 0.25, -0.6, 0.999, 1.0])
def test_pbe_correlation_without_a_gradient_is_pw92(zeta):
    ra, rb = 0.5 * RHO_LINE * (1.0 + zeta), 0.5 * RHO_LINE * (1.0 - zeta)
    a, b = response.spin_energy_host("1.0*pbe_c", ra, rb), response.spin_energy_host("1.0*pw92_c", ra, rb)
    assert np.all(b < 0.0) and np.abs(a - b).max() <= 1e-15 * np.abs(b).max()      # H = gamma phi^3 log(1 + 0)


@pytest.mark.parametrize("name", ["vwn5_c", "vwn_rpa_c", "pw92_c"])
def test_fully_polarised_gas_is_the_ferromagnetic_fit(name):
    """The same formula in numpy; the logarithms and the arctangent of a fit cancel to a tenth of their size: 1e-13."""
    rs = np.cbrt(3.0 / (4.0 * np.pi * RHO_LINE))
    e = response.spin_energy_host(f"1.0*{name}", RHO_LINE, np.zeros_like(RHO_LINE))
    ref = RHO_LINE * FERRO[name](rs)
    err = np.max(np.abs(e - ref) / np.abs(ref))
    print(f"{name} at zeta = 1 against its ferromagnetic fit: {err:.2e}")
    assert err <= 1e-13
    assert np.array_equal(e, response.spin_energy_host(f"1.0*{name}", np.zeros_like(RHO_LINE), RHO_LINE))


@pytest.mark.parametrize("name", ["slater_x", "pbe_x", "b88_x"])
def test_exchange_spin_scaling(name):
    """E[ra, rb] = (E[2 ra] + E[2 rb]) / 2, the closed-shell E[2 r] being the body at (r, r, s, s, s) -- and rho * exc of the
    sweep's point body at (2 r, 4 s).  sigma_ab plays no part."""
    rng = np.random.default_rng(3)
    ra, rb = 10.0 ** rng.uniform(-4, 1, 300), 10.0 ** rng.uniform(-4, 1, 300)
    saa, sbb = 10.0 ** rng.uniform(-6, 1, 300), 10.0 ** rng.uniform(-6, 1, 300)
    f = f"1.0*{name}"
    E = lambda *a: response.spin_energy_host(f, *a)
    whole = E(ra, rb, saa, rng.standard_normal(300) * np.sqrt(saa * sbb), sbb)
    halves = 0.5 * (E(ra, ra, saa, saa, saa) + E(rb, rb, sbb, sbb, sbb))
    assert np.max(np.abs(whole - halves) / np.abs(whole)) <= 4e-16
    grad = np.zeros((300, 3)); grad[:, 0] = 2.0 * np.sqrt(saa)
    closed = response.point_host(f, 2.0 * ra, 4.0 * saa, grad, np.ones(300), quirks=False)[0]
    assert np.max(np.abs(E(ra, ra, saa, saa, saa) - closed) / np.abs(closed)) <= 1e-15


@pytest.mark.parametrize("name", ["vwn5_c", "vwn_rpa_c", "pw92_c"])
def test_spin_stiffness_is_the_second_zeta_derivative(name):
    """d^2 e / d zeta^2 at zeta = 0 is rho alpha_c(rs).  Second central difference at dz = 0.01, extrapolated once: what is
    left is -dz^4 / 2 times the zeta^6 coefficient of the interpolation, (|e_F - e_P| + |alpha_c|) f''(0) / 2 and the
    sixth derivative of f over 360, together below 0.3 |alpha_c| dz^4 = 3e-9; rounding eps |e| / (dz^2 |alpha_c|) ~ 1e-11.
    Bar 1e-8."""
    rho, dz = RHO_LINE, 0.01
    E = lambda z: response.spin_energy_host(f"1.0*{name}", 0.5 * rho * (1.0 + z), 0.5 * rho * (1.0 - z))
    D = lambda h: (E(h) - 2.0 * E(0.0) + E(-h)) / (h * h)
    d2 = (4.0 * D(0.5 * dz) - D(dz)) / 3.0
    ref = rho * STIFFNESS[name](np.cbrt(3.0 / (4.0 * np.pi * rho)))
    err = np.max(np.abs(d2 - ref) / np.abs(ref))
    print(f"{name}: second zeta derivative against alpha_c {err:.2e}")
    assert err <= 1e-8


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", "BLYP", "PBE0", MIX])
def test_unpolarised_energy_is_the_point_body_energy(functional):
    """At ra = rb the bodies are rho * exc of the sweep's point bodies (quirks has no part in the energy).  Per point
    relative to sum_k |c_k e_k| (the components' own magnitudes; PBE correlation by its uniform-gas part): 1e-14, the
    rounding of a handful of operations in another order (2 ra against rho, the B88 per-spin arguments)."""
    rho, sigma = random_points(600, seed=4)
    live = rho >= 1e-12
    grad = np.zeros((rho.size, 3)); grad[:, 1] = np.sqrt(sigma)
    closed = response.point_host(functional, rho, sigma, grad, np.ones_like(rho), quirks=False)[0]
    e = response.spin_energy_host(functional, 0.5 * rho, 0.5 * rho, 0.25 * sigma, 0.25 * sigma, 0.25 * sigma)
    w8 = functionals.resolve(functional).weight_vector()
    mag = np.zeros_like(rho)
    for k, c in enumerate(w8):
        if c != 0.0:
            kk = COMPONENTS.index("pw92_c") if COMPONENTS[k] == "pbe_c" else k
            mag += abs(c) * np.abs(response.point_host(tr.unit(kk), rho, sigma, grad, np.ones_like(rho), quirks=False)[0])
    assert np.all(e[~live] == 0.0) and np.all(closed[~live] == 0.0)
    err = np.max(np.abs(e - closed)[live] / mag[live])
    print(f"{functional}: unpolarised energy against the point body {err:.2e}")
    assert err <= 1e-14


# ---- 4. the second-order type against differences of the energy --------------------------------------------------------
def diff_sample():
    r, s = np.meshgrid(np.logspace(-3, 1, 12), np.logspace(-6, 1, 12), indexing="ij")   # the sample of tests/test_fxc_cpu.py
    return r.ravel(), s.ravel()


@pytest.mark.parametrize("kind", [1, 2], ids=["triplet", "singlet"])
@pytest.mark.parametrize("k", range(8))
def test_table_against_differences_of_the_energy(k, kind):
    rho, sigma = diff_sample()
    w8 = tr.unit(k)
    tab = response.fxc_table_host(w8, rho, sigma, kind=kind)
    fine, coarse = tr.difference_table(w8, rho, sigma, kind, 1e-2), tr.difference_table(w8, rho, sigma, kind, 2e-2)
    # the scale of tests/test_fxc_cpu.py: u = |e| + |vrho| of the component (PBE correlation: of its PW92 part)
    grad = np.zeros((rho.size, 3)); grad[:, 0] = np.sqrt(sigma)
    kk = COMPONENTS.index("pw92_c") if COMPONENTS[k] == "pbe_c" else k
    pt = response.point_host(tr.unit(kk), rho, sigma, grad, np.ones_like(rho), quirks=False)
    u = np.abs(pt[0]) / rho + np.abs(pt[1])
    scales = [u / rho, u / sigma, u / sigma, u * rho / sigma ** 2, u * rho / sigma]
    worst_bar = worst_err = 0.0
    for p in range(5 if k >= 4 else 1):
        bar = np.max(np.abs(fine[p] - coarse[p]) / scales[p])
        err = np.max(np.abs(tab[p] - fine[p]) / scales[p])
        print(f"{COMPONENTS[k]} kind {kind} T{p}: bar {bar:.2e} err {err:.2e}")
        worst_bar, worst_err = max(worst_bar, bar), max(worst_err, err)
        assert bar <= DIFF_BAR, (COMPONENTS[k], p, bar)
        assert err <= DIFF_ERR, (COMPONENTS[k], p, err)
    tr.record(f"cpu table against differences of the energy, {COMPONENTS[k]} kind {kind} (own scale)", worst_err, DIFF_ERR)


# ---- 5. operator and solver --------------------------------------------------------------------------------------------
FUNCTIONALS = ["LDA", "B3LYP", "1.0*hf"]


@pytest.mark.parametrize("functional", FUNCTIONALS)
def test_triplet_matrices_are_symmetric_and_built_from_fxc_apply_host(functional):
    """A+B and A-B element by element from fxc_apply_host(kind="triplet") and the dense ERI, against the operators."""
    ops, ApB, AmB = tr.triplet_dense(functional)
    inp, res, rb = tr.state(functional)
    assert np.abs(ApB - ApB.T).max() <= 1e-12 and np.abs(AmB - AmB.T).max() <= 1e-12
    nocc, nvirt = ops.gap.shape
    N = nocc * nvirt
    P, Q = np.zeros((N, N)), np.zeros((N, N))
    w8 = functionals.resolve(tr.functional_of(functional))
    functional = tr.functional_of(functional)
    for n in range(N):
        i, a = divmod(n, nvirt)
        AB = 2.0 * np.outer(ops.Co[:, i], ops.Cv[:, a])
        Dp, Dm = AB + AB.T, AB - AB.T
        V1 = response.fxc_apply_host(functional, res["dm"], Dp, rb.ao, inp.grids.weights, rb.gr if w8.needs_gradient else None,
                                     quirks=False, kind="triplet")
        G = 0.5 * (V1 + V1.T) - 0.5 * w8.c_hf * np.einsum("ikjl,kl->ij", inp.eri, Dp)
        P[:, n] = (ops.Co.T @ G @ ops.Cv).reshape(-1)
        Q[:, n] = (-0.5 * w8.c_hf * ops.Co.T @ np.einsum("ikjl,kl->ij", inp.eri, Dm) @ ops.Cv).reshape(-1)
    P += np.diag(ops.gap.reshape(-1)); Q += np.diag(ops.gap.reshape(-1))
    assert np.abs(P - ApB).max() <= 1e-12 and np.abs(Q - AmB).max() <= 1e-12
    assert np.abs(P - P.T).max() <= 1e-12


@pytest.mark.parametrize("tda", [True, False], ids=["tda", "tddft"])
@pytest.mark.parametrize("functional", FUNCTIONALS)
def test_iterative_triplet_roots_match_the_dense_solution(functional, tda):
    inp, res, rb = tr.state(functional)
    w, _ = ed.dense_solution(*tr.triplet_dense(functional), tda)
    functional = tr.functional_of(functional)
    out = ex.excitations(inp, res, rb, functional, nroots=3, tda=tda, tol=1e-6, triplet=True)
    dw = float(np.abs(out["energies"] - w[:3]).max())
    print(f"{functional} triplet {'TDA' if tda else 'TDDFT'}: |dw| {dw:.2e}  iterations {out['iterations']}")
    assert out["converged"] and out["method"] == ("tda-triplet" if tda else "tddft-triplet") and out["multiplicity"] == 3
    assert np.all(out["residuals"] <= 1e-6) and dw <= 1e-9                      # the bounds of tests/test_excitations_cpu.py
    assert np.all(out["oscillator_strengths"] == 0.0) and np.all(out["transition_dipoles"] == 0.0)
    singlet = ex.excitations(inp, res, rb, functional, nroots=1, tda=tda)
    assert singlet["method"] == ("tda" if tda else "tddft") and singlet["multiplicity"] == 1
    assert 0.0 < out["energies"][0] < singlet["energies"][0]                    # the lowest triplet lies below the lowest singlet


def test_hartree_fock_tda_triplets_are_cis_triplets():
    """A_ia,jb = delta_ij delta_ab (e_a - e_i) - (ij|ab), from the ERI directly."""
    ops, ApB, AmB = tr.triplet_dense("1.0*hf")
    inp, _, _ = tr.state("1.0*hf")
    mo = np.einsum("mi,nj,mnls,la,sb->ijab", ops.Co, ops.Co, inp.eri, ops.Cv, ops.Cv)     # (ij|ab)
    N = ops.gap.size
    cis = np.diag(ops.gap.reshape(-1)) - mo.transpose(0, 2, 1, 3).reshape(N, N)
    assert np.abs(0.5 * (ApB + AmB) - cis).max() <= 1e-12


def test_stretched_h2_is_refused_as_a_triplet_instability(tmp_path):
    xyz = tmp_path / "h2_stretched.xyz"
    xyz.write_text("2\nH2 at 2.5 angstrom\nH 0.0 0.0 0.0\nH 0.0 0.0 2.5\n")
    inp, res, rb = tr.state("1.0*hf", 0, str(xyz))
    with pytest.raises(ValueError, match=r"triplet instability of the restricted reference") as info:
        ex.excitations(inp, res, rb, tr.HF, nroots=1, triplet=True)
    assert "lowest eigenvalue -" in str(info.value)
    assert ex.excitations(inp, res, rb, tr.HF, nroots=1)["energies"][0] > 0.0      # the singlet problem is stable


def test_quirks_refusals():
    for functional in ("LDA", "GGA"):                      # vwn5_c, pbe_c
        inp, res, rb = tr.state(functional, 1)
        with pytest.raises(ValueError, match="--quirks 0"):
            ex.excitations(inp, res, rb, functional, nroots=1, triplet=True)
    inp, res, rb = tr.state("B3LYP", 1)                    # neither component: quirks = 1 changes nothing for it
    assert ex.excitations(inp, res, rb, "B3LYP", nroots=1, triplet=True)["converged"]


# ---- 6. nothing moved --------------------------------------------------------------------------------------------------
def test_defaults_take_the_unchanged_paths():
    rho, sigma = random_points(500, seed=9)
    lib = response._load()
    for functional in ("LDA", "GGA", "B3LYP", "PBE0"):
        t, w8, _ = response._kind(functional)
        for quirks in (True, False):
            raw = np.zeros((5, rho.size))
            assert lib.qc_fxc_table(t, response._p(w8), int(quirks), rho.size, response._p(rho), response._p(sigma), response._p(raw)) == 0
            assert np.array_equal(raw, response.fxc_table_host(functional, rho, sigma, quirks))
            assert np.array_equal(raw, response.fxc_table_host(functional, rho, sigma, quirks, kind="singlet"))
    # the singlet solver: the same arrays with and without the new argument, and the roots of matrices restated here from
    # J, K and the default fxc_apply_host
    inp, res, rb = tr.state("B3LYP", 1)
    a = ex.excitations(inp, res, rb, "B3LYP", nroots=3)
    b = ex.excitations(inp, res, rb, "B3LYP", nroots=3, triplet=False)
    for key in ("energies", "oscillator_strengths", "transition_dipoles", "xpy", "xmy", "residuals"):
        assert np.array_equal(a[key], b[key]), key
    ops = ex.ResponseOperators(inp, res, rb, "B3LYP")
    nocc, nvirt = ops.gap.shape
    N = nocc * nvirt
    P, Q = np.diag(ops.gap.reshape(-1)).copy(), np.diag(ops.gap.reshape(-1)).copy()
    for n in range(N):
        i, v = divmod(n, nvirt)
        AB = 2.0 * np.outer(ops.Co[:, i], ops.Cv[:, v])
        Dp, Dm = AB + AB.T, AB - AB.T
        V1 = response.fxc_apply_host("B3LYP", res["dm"], Dp, rb.ao, inp.grids.weights, rb.gr, True)
        G = np.einsum("ijkl,kl->ij", inp.eri, Dp) + 0.5 * (V1 + V1.T) - 0.1 * np.einsum("ikjl,kl->ij", inp.eri, Dp)
        P[:, n] += (ops.Co.T @ G @ ops.Cv).reshape(-1)
        Q[:, n] += (-0.1 * ops.Co.T @ np.einsum("ikjl,kl->ij", inp.eri, Dm) @ ops.Cv).reshape(-1)
    w, f = ed.dense_solution(ops, P, Q, False)
    assert np.abs(a["energies"] - w[:3]).max() <= 1e-9 and np.abs(a["oscillator_strengths"] - f[:3]).max() <= 1e-6


# ---- 7. the C-ABI ------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_spin_entries():
    import quantum_compute_dft_amd as q
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dft_solver.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(DFT_[A-Za-z0-9]+)\s*\(", text))
    assert {"DFT_FxcPrepareSpin", "DFT_FxcApplyKind", "DFT_FxcPrepare", "DFT_FxcApply"} <= names
    lib = q.load_library(q.build_library())
    assert hasattr(lib, "DFT_FxcPrepareSpin") and hasattr(lib, "DFT_FxcApplyKind")
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5
    host = response._load()
    assert hasattr(host, "qc_fxc_table_spin") and hasattr(host, "qc_spin_energy")
    with pytest.raises(ValueError, match="unknown response kind"):
        response.fxc_table_host("LDA", np.array([0.3]), kind="quintet")
