"""The host engine's derivative integrals (csrc/integrals.c: qc_grad2e, qc_grad2e_spin, qc_grad1e) against a reference
that shares no code and no formulation with them: central differences, step 1e-30 bohr, of energies formed in
100-digit arithmetic from oracle/eri_reference.py (Rys-Dupuis-King two-dimensional integrals, mpmath's incomplete gamma
function), stored rounded to double in tests/golden/grad_ref_g{1,2,3}.npz (tests/golden/make_grad_reference.py).

Every family is four shells on four different centres, so the quartets with three or four shells of l >= 2 -- which in
the molecules of the other gradient tests sit on one atom, with X_AB = X_CD = 0, P = Q and a Boys argument of exactly
zero -- are four-centre here: g1 = s p d f (every bra and ket class), g2 = d d d d, g3 = f f f f (L = 13 with the
derivative).  Both orders of the shells, so that the (l_a < l_b) classes and the ket order C >= D come both ways.

Bound: |host - ref| <= 1e-12 max|ref| of the compared (4, 3) array, every row (grad_fixtures.BOUND).  Measured worst
figures (profiles/grad2e_reference_parity.txt): two-electron rows g1 3.0e-14, g2 1.7e-14, g3 1.5e-14; one-electron rows
<= 2.1e-15: a factor 30 or more under the bound in every family.  The device's turn is
tests/test_gpu_grad2e_reference.py."""
import os
import sys

import numpy as np
import pytest

import grad_fixtures as G
from quantum_compute_dft_amd import integrals

CASES = [(n, r) for n in G.FAMILIES for r in (False, True)]
IDS = [f"{n}{'-reversed' if r else ''}" for n, r in CASES]


# ------------------------------------------------------------------------------------------ the stored values
def test_fixtures_are_small_and_say_how_they_were_checked():
    for n in G.FAMILIES:
        assert os.path.getsize(os.path.join(G.F.GOLDEN, f"grad_ref_{n}.npz")) <= 64 * 1024
        m = G.family(n)["meta"]
        assert m["dps"] == 100 and m["step"] == "1e-30" and m["bound"] == G.BOUND
        assert float(m["step_check"]) <= 1e-40 and float(m["net_force"]) <= 1e-30


@pytest.mark.parametrize("name", G.FAMILIES)
def test_stored_rows_obey_what_the_generator_did_not_impose(name):
    """Every shell was displaced on its own, so translational invariance is a property of the values, not of their
    making: the two-electron rows, -tr(W dS) and tr(D dT) sum to zero over the shells to the rounding of the stored doubles
    (tr(D dV) does not: the charges stay).  Without exchange the spin rows are the closed-shell rows, bit for bit."""
    f = G.family(name)
    assert [int(l) for l in f["sh"].l] == {"g1": [0, 1, 2, 3], "g2": [2] * 4, "g3": [3] * 4}[name]
    assert len(np.unique(f["sh"].xyz, axis=0)) == 4 and sorted(f["sh"].atom) == [0, 1, 2, 3]
    for key in ("D", "M", "W"):
        assert np.array_equal(f[key], f[key].T)
    for rows in (*f["g2e"], *f["g2e_spin"], f["g1e"][0], f["g1e"][1]):
        assert np.abs(rows).min() > 0.0
        assert np.abs(rows.sum(axis=0)).max() <= 4 * np.finfo(float).eps * np.abs(rows).max()
    assert np.abs(f["g1e"][2].sum(axis=0)).max() > 1e-3 * np.abs(f["g1e"][2]).max()
    assert np.array_equal(f["g2e"][0], f["g2e_spin"][0]) and not np.array_equal(f["g2e"][1], f["g2e_spin"][1])
    assert not np.array_equal(f["g2e"][0], f["g2e"][1])


@pytest.mark.parametrize("name", G.FAMILIES)
def test_stored_parts_add_up_to_the_stored_coordinate(name):
    """The coordinate (shell 0, x) is stored a second time, one unique shell quartet at a time (34 contain the shell):
    the parts, rounded one by one, add up to the stored rows to the rounding of the parts and of their (pairwise) sum,
    8 eps sum|part| -- far below what the bound of the engine tests resolves."""
    f = G.family(name)
    s, k = f["meta"]["part_coordinate"]
    q, v = f["part_quartets"], f["part_values"]
    assert q.shape == (34, 4) and v.shape == (34, 3) and all(s in row for row in q) and len({tuple(r) for r in q}) == 34
    J, KD, KM = v.sum(axis=0)
    slack = 8 * np.finfo(float).eps * np.abs(v).sum()
    for i, c in enumerate(f["c_hf"]):
        assert abs(J / 2 - c / 4 * KD - f["g2e"][i, s, k]) <= slack
        assert abs(J / 2 - c / 4 * (KD + KM) - f["g2e_spin"][i, s, k]) <= slack
    assert slack <= 0.1 * G.BOUND * np.abs(f["g2e"]).max()


def test_stored_values_are_what_the_reference_computes():
    """g1, the s shell's x coordinate, recomputed now in one process: the three one-electron values and the parts of six
    shell quartets of the two-electron sum -- (ss|ss) to (fd|ps), mixed classes, one with a repeated pair -- equal the stored
    doubles bit for bit.  (The whole two-electron coordinate, 34 quartets, takes 8 s: the parts are stored so that this
    test stays within the 3 s of test_eri_reference_cpu's slowest; the test above ties the parts to the rows.)"""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_grad_reference as gen
    f = G.family("g1")
    s, k = f["meta"]["part_coordinate"]
    assert (s, k) == gen.PART_COORD
    only = [(0, 0, 0, 0), (1, 0, 1, 0), (2, 1, 0, 0), (3, 0, 2, 0), (3, 2, 1, 0), (3, 3, 0, 0)]
    stored = {tuple(int(x) for x in q): v for q, v in zip(f["part_quartets"], f["part_values"])}
    parts = {}
    key = (s, k, gen.STEP_EXP)
    q = gen.derivatives(gen.family("g1"), [key], workers=1, parts=parts, only=only)[key]
    assert np.array_equal(gen.stored_rows(q)[2], f["g1e"][:, s, k])
    assert [qt for qt, _ in parts[key]] == only
    for qt, v in parts[key]:
        assert np.array_equal(gen.R.to_double(np.array(v, dtype=object)), stored[qt]), qt


# ------------------------------------------------------------------------------------------ the host engine
@pytest.mark.parametrize("name,reverse", CASES, ids=IDS)
def test_host_two_electron_rows(name, reverse):
    f = G.family(name, reverse)
    for i, c_hf in enumerate(f["c_hf"]):
        G.check("cpu", G.label(f, f"grad2e c_hf {c_hf:g}"), integrals.grad2e(f["sh"], f["D"], c_hf, per_shell=True), f["g2e"][i])
        G.check("cpu", G.label(f, f"grad2e_spin c_hf {c_hf:g}"),
                integrals.grad2e_spin(f["sh"], f["D"], f["M"], c_hf, per_shell=True), f["g2e_spin"][i])


@pytest.mark.parametrize("name,reverse", CASES, ids=IDS)
def test_host_one_electron_rows(name, reverse):
    """grad1e returns rows per atom; shell_table numbers the atoms by np.unique of the centres, one shell each."""
    f = G.family(name, reverse)
    sh = f["sh"]
    got = integrals.grad1e(sh, f["charge_xyz"], f["charge_z"], f["D"], f["W"])
    assert got.shape == (3, 4, 3)
    for t, term in enumerate(("-tr(W dS)", "tr(D dT)", "tr(D dV)")):
        G.check("cpu", G.label(f, f"grad1e {term}"), got[t][np.asarray(sh.atom)], f["g1e"][t])
