"""scf.run_uks and inputs.build(charge, spin) on the host, with tests/uks_host_backend.py (dense ERI, numpy J / K,
response.xc_spin_host on the oracle's AO planes).

* spin = 0 on H2O / STO-3G against scf._run_scf with the oracle backend at quirks 0, LDA and B3LYP: 1e-9 Ha, the bound
  tests/test_gpu_scf_tail.py holds one loop against another.
* H atom with exact exchange alone (no sweep): E = the lowest eigenvalue of (Hcore, S) to 1e-10 Ha -- one electron has
  no interaction with itself, J[D] = K[D_alpha].
* H2O+ doublet, B3LYP / STO-3G: converges, 0.75 <= <S^2> < 0.80, and the Fock matrices of the converged densities commute
  with D_s S.
* inputs.build: charge and spin that do not fit the electron count, and the defaults.
"""
import numpy as np
import pytest
from scipy.linalg import eigh

import spin_reference as sr
import triplet_reference as tr
from quantum_compute_dft_amd import inputs, scf
from scf_oracle_backend import OracleBackend
from uks_host_backend import UksHostBackend

KW = dict(log=None, conv_e=1e-11, conv_dm=1e-8)


def test_spin_inputs_fail_on_a_closed_shell_only_tree():
    """What the project could not do before: an odd electron count."""
    inp = inputs.build("H2O", "sto-3g", grid_level=1, verbose=False, charge=1, spin=1)
    assert (inp.nelec, inp.nalpha, inp.nbeta, inp.nocc, inp.charge, inp.spin) == (9, 5, 4, 4, 1, 1)


def test_defaults_are_the_closed_shell():
    inp = inputs.build("H2O", "sto-3g", grid_level=1, verbose=False)
    assert (inp.nelec, inp.nocc, inp.nalpha, inp.nbeta, inp.charge, inp.spin) == (10, 5, 5, 5, 0, 0)
    trip = inputs.build("H2O", "sto-3g", grid_level=1, verbose=False, spin=2)
    assert (trip.nalpha, trip.nbeta, trip.nocc) == (6, 4, 4)
    for f in ("S", "Hcore", "eri"):
        assert np.array_equal(getattr(inp, f), getattr(trip, f))
    # a constructor call as every caller wrote it before the new fields existed
    old = inputs.SCFInputs(inp.symbols, inp.atom_xyz, inp.shells, inp.grids, inp.S, inp.T, inp.V, inp.Hcore, inp.eri, inp.E_nuc, inp.nocc, inp.nelec)
    assert old.nalpha is None and old.nbeta is None and old.spin == 0 and old.charge == 0


@pytest.mark.parametrize("kw,text", [
    (dict(spin=1), "--spin"),                      # even electron count, odd spin
    (dict(charge=1), "--spin"),                    # odd electron count without a spin: the message names the flag
    (dict(spin=-2), "does not fit"),
    (dict(spin=12), "does not fit"),
    (dict(charge=10), "no electrons"),
    (dict(charge=-4, spin=14), "basis functions"),   # 14 electrons, all alpha, in 7 functions
])
def test_charge_and_spin_that_do_not_fit(kw, text):
    with pytest.raises(ValueError, match=text):
        inputs.build("H2O", "sto-3g", grid_level=1, verbose=False, **kw)


@pytest.fixture(scope="module")
def h2o():
    return inputs.build("H2O", "sto-3g", grid_level=1, verbose=False)


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_spin_zero_reproduces_the_restricted_loop(h2o, functional):
    rks = scf._run_scf(h2o, OracleBackend(h2o, functional, quirks=False), functional, 200, KW["conv_e"], KW["conv_dm"], None)
    uks = scf.run_uks(h2o, UksHostBackend(h2o, functional), functional, **KW)
    assert rks["converged"] and uks["converged"] and uks["uks"]
    print(f"{functional}: RKS {rks['E_tot']:.12f}  UKS {uks['E_tot']:.12f}  diff {uks['E_tot'] - rks['E_tot']:+.2e}  cycles {rks['cycles']} / {uks['cycles']}")
    sr.record(f"cpu uks spin 0 against rks {functional} (Ha)", abs(uks["E_tot"] - rks["E_tot"]), 1e-9)
    assert abs(uks["E_tot"] - rks["E_tot"]) <= 1e-9
    assert np.abs(uks["dm"] - rks["dm"]).max() <= 1e-6
    assert np.abs(uks["dm_a"] - uks["dm_b"]).max() <= 1e-10      # no symmetry breaking from a symmetric guess
    assert abs(uks["s_squared"]) <= 1e-9
    assert np.abs(uks["mo_energy_a"] - rks["mo_energy"]).max() <= 1e-6


def test_hydrogen_atom_with_exact_exchange_alone(tmp_path):
    xyz = tmp_path / "H.xyz"
    xyz.write_text("1\nhydrogen atom\nH 0.0 0.0 0.0\n")
    inp = inputs.build(str(xyz), "def2-svp", grid_level=1, verbose=False, spin=1)
    assert (inp.nalpha, inp.nbeta) == (1, 0) and inp.shells.nao > 1
    be = UksHostBackend(inp, tr.HF)
    assert not be.sweep
    res = scf.run_uks(inp, be, tr.HF, **KW)
    e0 = eigh(inp.Hcore, inp.S, eigvals_only=True)[0]
    print(f"H atom: E {res['E_tot']:.12f}  lowest eigenvalue {e0:.12f}  cycles {res['cycles']}")
    assert res["converged"]
    assert abs(res["E_tot"] - e0) <= 1e-10
    assert abs(res["s_squared"] - 0.75) <= 1e-12
    assert np.all(res["dm_b"] == 0.0) and abs(res["mo_energy_a"][0] - e0) <= 1e-9


def test_water_cation_doublet():
    inp = inputs.build("H2O", "sto-3g", grid_level=1, verbose=False, charge=1, spin=1)
    be = UksHostBackend(inp, "B3LYP")
    res = scf.run_uks(inp, be, "B3LYP", **KW)
    assert res["converged"] and res["nalpha"] == 5 and res["nbeta"] == 4
    print(f"H2O+ B3LYP/STO-3G: E {res['E_tot']:.10f}  <S^2> {res['s_squared']:.6f}  cycles {res['cycles']}")
    assert 0.75 <= res["s_squared"] < 0.80
    # electrons of each spin, and the neutral molecule lies below its cation
    assert abs(np.sum(res["dm_a"] * inp.S) - 5.0) <= 1e-10 and abs(np.sum(res["dm_b"] * inp.S) - 4.0) <= 1e-10
    neutral = inputs.build("H2O", "sto-3g", grid_level=1, verbose=False)
    e_n = scf.run_uks(neutral, UksHostBackend(neutral, "B3LYP"), "B3LYP", **KW)["E_tot"]
    assert 0.2 < res["E_tot"] - e_n < 0.6                       # an ionisation energy of some eV
    # The converged F_s commutes with D_s S.  The loop stopped when the densities moved by less than conv_dm = 1e-8
    # (Frobenius) in a step; the commutator is linear in the distance of D_s from the fixed point, with a factor of the
    # order 2 |F|_2 |S|_2 (about 2 x 20 x 2 here: the oxygen 1s level): 1e-6.
    F = be.fock(res["dm_a"], res["dm_b"], 0.2)
    for Fs, Ds in zip(F, (res["dm_a"], res["dm_b"])):
        comm = Fs @ Ds @ inp.S - inp.S @ Ds @ Fs
        print(f"  max|F D S - S D F| {np.abs(comm).max():.2e}")
        assert np.abs(comm).max() <= 1e-6
