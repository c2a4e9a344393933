"""integrals.grad2e_spin (integrals.c::qc_grad2e_spin): the two-electron gradient term of an open-shell state, one pass with
the density quartet 2 f D_ab D_cd - c_hf [D_ac D_bd + M_ac M_bd + (C != D)(D_ad D_bc + M_ad M_bc)], D the total and M the
spin density.

The energy is linear in the pair (D D, M M), so the pass must equal grad2e(D, c) + grad2e(M, c) - grad2e(M, 0) of the
closed-shell routine (the last two leave -c/4 d[sum M M (ab|cd)]).  Yardstick: grad2e_helper's, the host engine's own
spread between the two orders of the atoms (10 bar <= 1e-11, difference <= max(10 bar, 1e-13) of max|g|)."""
import numpy as np
import pytest

import grad2e_helper as gh
from quantum_compute_dft_amd import integrals

C_HF = 0.25


def spin_density(nao):
    """A random symmetric M of the size of gh.random_density's D, from a generator of its own."""
    return gh.random_density(nao, seed=23)


@pytest.fixture(scope="module")
def ch():
    c = gh.ch_case(C_HF)
    return c, np.ascontiguousarray(spin_density(c["shells"].nao))


def test_one_pass_equals_the_closed_shell_routine_by_linearity(ch):
    """CH/def2-TZVP: every class s-f on bra and ket, per shell."""
    c, M = ch
    sh, D = c["shells"], c["D"]
    got = integrals.grad2e_spin(sh, D, M, C_HF, per_shell=True)
    ref = c["per_shell"] + integrals.grad2e(sh, M, C_HF, per_shell=True) - integrals.grad2e(sh, M, 0.0, per_shell=True)
    assert got.shape == (sh.nshell, 3)
    gh.check("cpu grad2e_spin CH/def2-TZVP c_hf 0.25 per shell against linearity", got, ref, c["bar"])
    per_atom = integrals.grad2e_spin(sh, D, M, C_HF)
    err = np.abs(gh.sum_per_atom(sh, got) - per_atom).max() / np.abs(per_atom).max()
    print(f"cpu grad2e_spin CH/def2-TZVP: per-shell rows summed against per-atom {err:.2e}")
    assert err <= 1e-13


def test_without_a_spin_density_it_is_the_closed_shell_term(ch):
    c, M = ch
    sh, D = c["shells"], c["D"]
    got = integrals.grad2e_spin(sh, D, 0.0 * M, C_HF, per_shell=True)
    err = np.abs(got - c["per_shell"]).max() / np.abs(c["per_shell"]).max()
    print(f"cpu grad2e_spin(D, 0, c) against grad2e(D, c): {err:.2e}")
    assert err <= 1e-14


def test_without_exact_exchange_the_spin_density_plays_no_part(ch):
    c, M = ch
    sh, D = c["shells"], c["D"]
    ref = gh.ch_case(0.0)["per_shell"]
    got = integrals.grad2e_spin(sh, D, M, 0.0, per_shell=True)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"cpu grad2e_spin(D, M, 0) against grad2e(D, 0): {err:.2e}")
    assert err <= 1e-14


def test_translational_invariance(ch):
    c, M = ch
    rows = integrals.grad2e_spin(c["shells"], c["D"], M, C_HF, per_shell=True)
    net = np.abs(rows.sum(axis=0)).max() / np.abs(rows).max()
    print(f"cpu grad2e_spin CH/def2-TZVP c_hf 0.25: |sum over shells| / max|row| {net:.2e}")
    assert net <= 1e-10


def test_refusals(ch):
    c, M = ch
    skew = np.array(M)
    skew[0, 1] += 1e-3
    with pytest.raises(ValueError, match="symmetric"):
        integrals.grad2e_spin(c["shells"], c["D"], skew, C_HF)
    with pytest.raises(ValueError, match="same shape"):
        integrals.grad2e_spin(c["shells"], c["D"], M[:5, :5], C_HF)
