"""The field of a density at points on the HOST (integrals.point_coulomb_field: the derivative of the one-electron Coulomb
integral with respect to the point) against the stored 100-digit reference and against a difference of the potential, and
what is built on it: properties.electric_field, properties.point_charge_forces, the driver's writers.  No GPU."""
import os
import sys

import numpy as np
import pytest

import point_field_fixtures as F
from quantum_compute_dft_amd import basis, dft, inputs, integrals, properties, scf
from scf_oracle_backend import OracleBackend

BOUND = F.BOUND
CHARGES = np.array([[3.0, 0.5, -1.0, -0.8], [-2.5, 2.0, 1.5, 0.4]])      # bohr, e: the set-up of test_point_coulomb_cpu.py


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_host_derivative_of_a_unit_charge_matches_the_reference_at_every_stored_point(name):
    """dA[c, k, mu, nu] from the contraction with D = e_mu e_nu^T, per element BOUND * max(1, max|dA[c, k]|).  The table
    of error / allowed per class (la, lb) is printed (profiles/point_field_parity.txt): the worst is 2.8e-4 for z1 (ff) and
    1.6e-2 for z3 (ps); (ff), whose table of order 7 goes past what the potential's tests pin, stays at 1.1e-3 in z3."""
    f = F.family(name)
    got = F.unit_matrix_from_contractions(lambda D: integrals.point_coulomb_field(f["sh"], f["points"], D), f["sh"])
    allowed = BOUND * np.maximum(1.0, np.abs(f["dA"]).max(axis=(2, 3)))[:, :, None, None]
    ratio = np.abs(got - f["dA"]) / allowed
    F.print_class_table(f"{name}, host: worst |dA - reference| / allowed per class over the {len(f['points'])} stored points "
                        f"(allowed = {BOUND:g} x max(1, max|dA[c, k]|))", F.class_ratios(ratio, f["sh"]))
    assert np.abs(f["dA"]).max() > 0.1                                     # a wrong sign or component shows at this size
    c, k, i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (name, c, k, i, j, got[c, k, i, j], f["dA"][c, k, i, j])
    # the host's matrix form (what the device test on a larger molecule takes its scale from): same bound
    for c, r in enumerate(f["points"]):
        M = integrals.point_coulomb_field_matrix(f["sh"], r[None, :], np.ones(1))
        assert (np.abs(M - f["dA"][c]) <= allowed[c]).all(), (name, c)
        assert np.array_equal(M, M.transpose(0, 2, 1))


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_host_field_matches_the_reference_for_a_full_and_ten_class_masked_matrices(name):
    f = F.family(name)
    refs = F.references(name)
    assert len(refs) == 11
    for label, D, ref, allowed in refs:
        G = integrals.point_coulomb_field(f["sh"], f["points"], D)
        assert G.shape == (len(f["points"]), 3)
        assert np.abs(ref).max() > 0.0 and not np.array_equal(D, D.T), label
        assert (np.abs(G - ref) <= allowed).all(), (name, label, (np.abs(G - ref) / allowed).max())


def _benzene():
    path = os.path.join(inputs.DATA_DIR, "Benzene.xyz")
    return basis.build_shells(*basis.parse_xyz(path), "def2-svp"), basis.parse_xyz(path)[1]


def test_host_field_is_the_difference_quotient_of_the_host_potential():
    """Independent of mpmath: central difference of point_coulomb_contract at h = 1e-4 on Benzene/def2-SVP, 50 points at
    least 0.1 bohr from every nucleus.  1e-6 * max(1, |G|): truncation and cancellation of the double-precision difference
    are near 1e-8, a wrong derivative is off by order 1."""
    shells, xyz = _benzene()
    rng = np.random.default_rng(50)
    pts = np.empty((0, 3))
    while len(pts) < 50:
        cand = rng.uniform(-6.0, 6.0, (200, 3)) + xyz.mean(axis=0)
        pts = np.concatenate([pts, cand[np.linalg.norm(cand[:, None] - xyz[None], axis=2).min(axis=1) >= 0.1]])[:50]
    D = rng.standard_normal((shells.nao, shells.nao))
    G = integrals.point_coulomb_field(shells, pts, D)
    h = 1e-4
    fd = np.empty_like(G)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        fd[:, k] = (integrals.point_coulomb_contract(shells, pts + e, D) - integrals.point_coulomb_contract(shells, pts - e, D)) / (2 * h)
    err = np.abs(G - fd) / np.maximum(1.0, np.abs(G))
    print(f"\nBenzene/def2-SVP, 50 points: max |G| = {np.abs(G).max():.3e}, worst |G - difference quotient| / max(1, |G|) = {err.max():.2e}")
    assert np.abs(G).max() > 1.0
    assert err.max() <= 1e-6


def test_stored_reference_is_reproduced_bit_for_bit():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_point_field_reference as gen
    f = F.family("z1")
    shells = gen.stored_shells("eri_ref_z1.npz")
    for c, k in ((4, 0), (9, 2)):                      # a centre displaced by 3e-7 bohr, a point between the centres
        assert np.array_equal(gen.derivative_double(shells, f["points"][c], k), f["dA"][c, k]), (c, k)
    x = gen.boys_arguments(shells, f["points"])
    assert {n: int(sel(x).sum()) for n, sel in gen.REGIMES} == f["meta"]["boys_regimes"]
    assert all(v > 0 for v in f["meta"]["boys_regimes"].values())
    assert f["meta"]["largest_step_disagreement"] < 1e-35


def _energy_gradient_against_force(fn, quirks, h=1e-3):
    """(Richardson-extrapolated central difference of E_tot in the position of charge 0, from h and 2h; -force on it)."""
    kw = dict(log=None, conv_e=1e-12, conv_dm=1e-9)

    def run(q):
        inp = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=q)
        res = scf.run_scf(inp, OracleBackend(inp, fn, quirks=quirks), fn, **kw)
        assert res["converged"]
        return inp, res

    inp, r0 = run(CHARGES)
    minus_f = -properties.point_charge_forces(inp, r0["dm"])[0]
    dE = np.empty(3)
    for k in range(3):
        def slope(step):
            d = np.zeros_like(CHARGES)
            d[0, k] = step
            return (run(CHARGES + d)[1]["E_tot"] - run(CHARGES - d)[1]["E_tot"]) / (2 * step)
        dE[k] = (4.0 * slope(h) - slope(2 * h)) / 3.0
    return dE, minus_f


@pytest.mark.parametrize("fn,quirks", [("LDA", False), ("B3LYP", True)])
def test_energy_gradient_in_a_charge_position_is_minus_the_force_on_it(fn, quirks):
    """Hellmann-Feynman in the position through the whole loop: dE_tot/dR_0 = -F_0 for a variational energy (no basis
    function moves with the charge).  Central differences at h = 1e-3 and 2h, Richardson-extrapolated: SCF noise of 1e-12
    over 2h is 5e-10 and the h^2 term is removed.  Measured |dE/dR_0k + F_0k| for k = x, y, z: LDA 5.9e-9, 1.1e-11,
    3.2e-12; B3LYP 1.1e-10, 8.4e-12, 8.0e-11.  The 5.9e-9 is SCF noise (one of the four displaced runs stops at cycle 12,
    the others at 15 to 17): with conv_e = 1e-14, conv_dm = 1e-11 the same component gives 5.9e-11."""
    dE, minus_f = _energy_gradient_against_force(fn, quirks)
    print(f"\n{fn}: dE/dR_0 = {dE}, -F_0 = {minus_f}, differences {np.abs(dE - minus_f)}")
    assert np.abs(minus_f).max() > 1e-3
    assert (np.abs(dE - minus_f) <= 1e-8).all()


def test_energy_gradient_test_sees_an_inconsistent_potential():
    """The reference's LDA formulas as shipped (quirks): V_xc is not dE_xc/d rho, the density is not the energy's
    stationary point, and the same comparison shows it (measured 2.9e-6, 2.5e-6, 8.8e-6)."""
    dE, minus_f = _energy_gradient_against_force("LDA", True)
    print(f"\nLDA with quirks: differences {np.abs(dE - minus_f)}")
    assert np.abs(dE - minus_f).max() > 1e-7


def test_electric_field_nuclear_term_electronic_only_and_the_nucleus_check():
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    n = inp.shells.nao
    z = [basis.atomic_number(s) for s in inp.symbols]
    pts = np.array([[0.3, 0.2, 4.0], [-1.5, 0.7, 0.4]])
    nuclear = np.array([sum(za * (r - ra) / np.linalg.norm(r - ra) ** 3 for za, ra in zip(z, inp.atom_xyz)) for r in pts])
    assert np.abs(properties.electric_field(inp, np.zeros((n, n)), pts) - nuclear).max() <= 1e-14 * np.abs(nuclear).max()
    dm = np.eye(n)
    full, el = properties.electric_field(inp, dm, pts), properties.electric_field(inp, dm, pts, electronic_only=True)
    assert full.shape == el.shape == (2, 3)
    assert np.array_equal(el, integrals.point_coulomb_field(inp.shells, pts, dm)) and np.abs(el).max() > 1e-2
    assert np.abs(full - el - nuclear).max() <= 1e-14 * np.abs(nuclear).max()
    # far away the molecule with tr(dm S) = 10 electrons looks neutral: the two parts cancel
    S_dm = np.linalg.inv(inp.S) * 10.0 / n
    far = np.array([[0.0, 0.0, 200.0]])
    assert np.abs(properties.electric_field(inp, S_dm, far)).max() < 1e-2 * np.abs(properties.electric_field(inp, S_dm, far, electronic_only=True)).max()
    with pytest.raises(ValueError):
        properties.electric_field(inp, dm, inp.atom_xyz[1:2] + np.array([0.0, 5e-9, 0.0]))
    assert np.isfinite(properties.electric_field(inp, dm, inp.atom_xyz[1:2], electronic_only=True)).all()
    with pytest.raises(ValueError):
        properties.electric_field(inp, dm, np.zeros(3))


def test_point_charge_forces_scale_with_the_charge_and_need_charges():
    bare = inputs.build("H2O", "sto-3g", 1, verbose=False)
    dm = np.eye(bare.shells.nao)
    with pytest.raises(ValueError):
        properties.point_charge_forces(bare, dm)
    emb = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=CHARGES)
    F_c = properties.point_charge_forces(emb, dm)
    assert F_c.shape == (2, 3)
    assert np.array_equal(F_c, CHARGES[:, 3:4] * properties.electric_field(emb, dm, CHARGES[:, :3]))


def test_driver_field_and_force_files_round_trip_in_both_units(tmp_path):
    pts = CHARGES[:, :3]
    E = np.array([[0.25, -0.5, 1.0e-7], [-3.0, 0.125, 42.0]])
    for unit in ("angstrom", "bohr"):
        out = tmp_path / f"field_{unit}.txt"
        dft.write_field_rows(str(out), pts, E, unit)
        back = dft.read_point_rows(str(out), 6, unit)
        assert back.shape == (2, 6) and np.abs(back[:, :3] - pts).max() <= 1e-9 and np.array_equal(back[:, 3:], E)
        out = tmp_path / f"forces_{unit}.txt"
        dft.write_charge_force_rows(str(out), CHARGES, E, unit)
        back = dft.read_point_rows(str(out), 7, unit)
        assert back.shape == (2, 7) and np.abs(back[:, :3] - pts).max() <= 1e-9
        assert np.array_equal(back[:, 3], CHARGES[:, 3]) and np.array_equal(back[:, 4:], E)
    a, b = (dft.read_point_rows(str(tmp_path / f"field_{u}.txt"), 6, "bohr") for u in ("angstrom", "bohr"))
    assert np.abs(a[:, :3] - b[:, :3] * basis.BOHR).max() <= 1e-9
