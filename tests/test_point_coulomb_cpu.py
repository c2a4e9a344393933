"""One-electron Coulomb integrals at points on the HOST (integrals.point_coulomb_matrix / point_coulomb_contract) against
the stored 100-digit reference, and what is built on them: external point charges in inputs.build, the electrostatic
potential of properties.py, the driver's file readers.  No GPU."""
import os
import sys

import numpy as np
import pytest

import point_coulomb_fixtures as F
from quantum_compute_dft_amd import basis, dft, inputs, integrals, properties, scf
from scf_oracle_backend import OracleBackend

BOUND = F.BOUND
# the set-up of the Hellmann-Feynman tests: H2O / STO-3G, grid level 1, two charges (bohr, e)
CHARGES = np.array([[3.0, 0.5, -1.0, -0.8], [-2.5, 2.0, 1.5, 0.4]])


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_host_matrix_of_a_unit_charge_matches_the_reference_at_every_stored_point(name):
    f = F.family(name)
    worst = 0.0
    for c, (r, A) in enumerate(zip(f["points"], f["A"])):
        M = integrals.point_coulomb_matrix(f["sh"], r[None, :], np.ones(1))
        err, allowed = np.abs(M - A).max(), BOUND * max(1.0, np.abs(A).max())
        worst = max(worst, err / allowed)
        assert err <= allowed, (name, c, r, err, allowed)
        assert np.array_equal(M, M.T)
    print(f"{name}: worst error / allowed = {worst:.2e}")


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_host_contraction_matches_the_reference_for_a_full_and_ten_class_masked_matrices(name):
    f = F.family(name)
    dens = F.densities(f["sh"])
    assert len(dens) == 11
    for label, D in dens:
        ref, allowed = F.contract_reference(D, f["A"])
        u = integrals.point_coulomb_contract(f["sh"], f["points"], D)
        assert np.abs(ref).max() > 0.0, label
        assert (np.abs(u - ref) <= allowed).all(), (name, label, np.abs(u - ref).max())


def test_nuclear_attraction_is_the_matrix_of_the_nuclear_charges():
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    z = np.array([basis.atomic_number(s) for s in inp.symbols], dtype=np.float64)
    assert np.abs(-integrals.point_coulomb_matrix(inp.shells, inp.atom_xyz, z) - inp.V).max() <= 1e-13


def test_stored_reference_is_reproduced_bit_for_bit():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_point_coulomb_reference as gen
    f = F.family("z1")
    shells = gen.stored_shells("eri_ref_z1.npz")
    assert np.array_equal(gen.points_of(shells, gen.Z1_EXTRA), f["points"])
    gen._init(shells, gen.R.DPS)
    for c in (4, 9):                                   # a centre displaced by 3e-7 bohr, a point between the centres
        assert np.array_equal(gen._job(f["points"][c]), f["A"][c]), c
    x = gen.boys_arguments(shells, f["points"])
    assert {k: int(sel(x).sum()) for k, sel in gen.REGIMES} == f["meta"]["boys_regimes"]
    assert all(v > 0 for v in f["meta"]["boys_regimes"].values())


def test_inputs_build_with_point_charges():
    base = inputs.build("H2O", "sto-3g", 1, verbose=False)
    none = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=None)
    assert np.array_equal(none.Hcore, base.T + base.V) and np.array_equal(none.Hcore, base.Hcore) and none.E_nuc == base.E_nuc
    assert none.point_charges is None and none.V_ext is None and none.E_nuc_ext == 0.0
    zero = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=CHARGES * np.array([1.0, 1.0, 1.0, 0.0]))
    assert np.abs(zero.Hcore - base.Hcore).max() == 0.0 and zero.E_nuc - base.E_nuc == 0.0
    emb = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=CHARGES)
    z = [basis.atomic_number(s) for s in emb.symbols]
    e_ext = sum(za * q / np.linalg.norm(ra - CHARGES[c, :3]) for za, ra in zip(z, emb.atom_xyz) for c, q in enumerate(CHARGES[:, 3]))
    assert emb.E_nuc_ext == pytest.approx(e_ext, rel=1e-14) and emb.E_nuc == pytest.approx(base.E_nuc + e_ext, rel=1e-14)
    assert np.array_equal(emb.point_charges, CHARGES)
    assert np.array_equal(emb.V_ext, -integrals.point_coulomb_matrix(emb.shells, CHARGES[:, :3], CHARGES[:, 3]))
    assert np.abs(emb.Hcore - (base.T + base.V + emb.V_ext)).max() <= 1e-15 and np.abs(emb.V_ext).max() > 1e-2
    on_nucleus = CHARGES.copy()
    on_nucleus[1, :3] = emb.atom_xyz[2] + np.array([0.0, 5e-9, 0.0])
    with pytest.raises(ValueError):
        inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=on_nucleus)
    with pytest.raises(ValueError):
        properties.electrostatic_potential(base, np.eye(base.shells.nao), base.atom_xyz[:1])
    dm = np.eye(base.shells.nao)
    r = np.array([[0.3, 0.2, 4.0]])
    full, el = properties.electrostatic_potential(base, dm, r), properties.electrostatic_potential(base, dm, r, electronic_only=True)
    assert el[0] < 0.0 and full[0] - el[0] == pytest.approx(sum(za / np.linalg.norm(ra - r[0]) for za, ra in zip(z, base.atom_xyz)), rel=1e-14)


def _energy_derivative_against_esp(fn, quirks, h):
    """(central difference of E_tot in the charge at site 0, ESP of the converged density at site 0)."""
    kw = dict(log=None, conv_e=1e-12, conv_dm=1e-9)
    run = lambda q: (lambda inp: (inp, scf.run_scf(inp, OracleBackend(inp, fn, quirks=quirks), fn, **kw)))(
        inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=q))
    dq = np.zeros_like(CHARGES)
    dq[0, 3] = h
    (_, rp), (_, rm), (inp, r0) = run(CHARGES + dq), run(CHARGES - dq), run(CHARGES)
    assert rp["converged"] and rm["converged"] and r0["converged"]
    esp = properties.electrostatic_potential(inp, r0["dm"], CHARGES[:1, :3])[0]
    return (rp["E_tot"] - rm["E_tot"]) / (2 * h), esp


@pytest.mark.parametrize("fn,quirks", [("LDA", False), ("GGA", False), ("B3LYP", True)])
def test_energy_derivative_in_a_charge_is_the_potential_at_its_site(fn, quirks):
    """Hellmann-Feynman through the whole loop: dE_tot/dq_0 = ESP(R_0) for a variational energy.  Measured 7e-11 to
    8e-11 at h = 1e-3 (truncation of the central difference); a potential that is not the derivative of its energy gives 4e-6."""
    dE, esp = _energy_derivative_against_esp(fn, quirks, 1e-3)
    print(f"{fn}: dE/dq = {dE:.12f}, ESP = {esp:.12f}, difference {abs(dE - esp):.2e}")
    assert abs(esp) > 1e-3
    assert abs(dE - esp) <= 1e-8


def test_energy_derivative_test_sees_an_inconsistent_potential():
    """The reference's LDA formulas as shipped (quirks): V_xc is not dE_xc/d rho, and the same comparison shows it."""
    dE, esp = _energy_derivative_against_esp("LDA", True, 1e-3)
    print(f"LDA with quirks: difference {abs(dE - esp):.2e}")
    assert abs(dE - esp) > 1e-6


def test_driver_point_files_in_angstrom_and_bohr_give_the_same_core_hamiltonian(tmp_path):
    """The driver itself needs a GPU; its readers and the unit conversion do not."""
    a, b = tmp_path / "q_angstrom.txt", tmp_path / "q_bohr.txt"
    b.write_text("# x y z q\n" + "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in CHARGES))
    a.write_text("".join(" ".join(repr(float(v)) for v in (*(row[:3] * basis.BOHR), row[3])) + "\n\n" for row in CHARGES))
    qa, qb = dft.read_point_rows(str(a), 4, "angstrom"), dft.read_point_rows(str(b), 4, "bohr")
    assert qa.shape == qb.shape == (2, 4) and np.array_equal(qb, CHARGES) and np.abs(qa - qb).max() <= 1e-15
    ha = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=qa).Hcore
    hb = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=qb).Hcore
    assert np.abs(ha - hb).max() <= 1e-14
    with pytest.raises(ValueError):
        dft.read_point_rows(str(b), 3, "bohr")
    out = tmp_path / "esp.txt"
    dft.write_esp_rows(str(out), qb[:, :3], np.array([0.25, -0.5]), "angstrom")
    back = dft.read_point_rows(str(out), 4, "angstrom")
    assert np.abs(back[:, :3] - qb[:, :3]).max() <= 1e-9 and np.array_equal(back[:, 3], [0.25, -0.5])
