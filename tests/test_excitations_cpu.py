"""excitations.excitations (TDDFT / TDA) on the host: H2O / STO-3G, grid level 1, the SCF on the oracle backend and the
response parts from response.HostResponse -- 5 occupied and 2 virtual orbitals, 10 pairs.

* Full spectrum: the sum over states 2 sum_n mu_n mu_n^T / w_n equals the CPKS polarizability, which applies the same
  (A+B).  One identity checks A+B, A-B, the normalisation (X+Y)^T (X-Y) = 1 and the transition dipoles.  Bound:
  4 max_k |D_k|_F max(CPKS residual), what the CPKS solve carries to alpha (test_response_cpu.py), plus 1e-10.
* Iterative against dense: the operators applied to unit vectors give A+B and A-B as matrices, LAPACK solves them.  At
  tol = 1e-6 the eigenvalue error is second order in the residual, r^2 / gap ~ 1e-12 / 0.05: bound 1e-9 Ha.
"""
import functools
import types

import numpy as np
import pytest

from quantum_compute_dft_amd import excitations as ex
from quantum_compute_dft_amd import inputs, response, scf
import excitation_dense as ed
from excitation_dense import dense_matrices
from scf_oracle_backend import OracleBackend


@functools.lru_cache(maxsize=None)
def state(functional, quirks, basis="sto-3g"):
    inp = inputs.build("H2O", basis, grid_level=1, verbose=False)
    be = OracleBackend(inp, functional, quirks=bool(quirks))
    res = scf.run_scf(inp, be, functional, conv_e=1e-12, conv_dm=1e-9, log=None)
    assert res["converged"]
    return inp, res, response.HostResponse(inp, functional, be, be.ao, be.gr, quirks=bool(quirks))


@functools.lru_cache(maxsize=None)
def dense(functional, quirks, basis="sto-3g"):
    """(ops, A+B, A-B as (N, N) matrices)."""
    inp, res, rb = state(functional, quirks, basis)
    ops = ex.ResponseOperators(inp, res, rb, functional)
    return (ops,) + dense_matrices(ops)


def dense_solution(functional, quirks, tda):
    return ed.dense_solution(*dense(functional, quirks), tda)


@pytest.mark.parametrize("functional,quirks", [("LDA", 0), ("LDA", 1), ("GGA", 0), ("B3LYP", 1)])
def test_full_spectrum_sums_to_the_cpks_polarizability(functional, quirks):
    inp, res, rb = state(functional, quirks)
    out = ex.excitations(inp, res, rb, functional, nroots=10)
    pol = response.polarizability(inp, res, rb, functional)
    w, mu = out["energies"], out["transition_dipoles"]
    sos = 2.0 * np.einsum("nk,nl,n->kl", mu, mu, 1.0 / w)
    err = float(np.abs(sos - pol["alpha"]).max())
    bound = 4.0 * max(np.linalg.norm(pol["dipole_integrals"][k]) for k in range(3)) * max(pol["residual"]) + 1e-10
    print(f"SOS {functional} quirks={quirks}: |sos - alpha| {err:.2e}  bound {bound:.2e}")
    assert out["converged"] and w.shape == (10,) and mu.shape == (10, 3)
    assert err <= bound, (err, bound)
    assert np.all(out["oscillator_strengths"] >= 0.0)
    assert np.all(np.diff(w) >= 0.0) and w[0] > 0.0
    assert np.abs(np.einsum("nia,mia->nm", out["xpy"], out["xmy"]) - np.eye(10)).max() <= 1e-10


@pytest.mark.parametrize("tda", [True, False], ids=["tda", "tddft"])
@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_iterative_roots_match_the_dense_solution(functional, tda):
    inp, res, rb = state(functional, 1)
    out = ex.excitations(inp, res, rb, functional, nroots=3, tda=tda, tol=1e-6)
    w, f = dense_solution(functional, 1, tda)
    dw, df = float(np.abs(out["energies"] - w[:3]).max()), float(np.abs(out["oscillator_strengths"] - f[:3]).max())
    print(f"{functional} {'TDA' if tda else 'TDDFT'}: |dw| {dw:.2e}  |df| {df:.2e}  iterations {out['iterations']}  builds {out['sigma_builds']}")
    assert out["converged"] and out["method"] == ("tda" if tda else "tddft") and np.all(out["residuals"] <= 1e-6)
    assert dw <= 1e-9 and df <= 1e-6
    if tda:
        assert np.array_equal(out["xpy"], out["xmy"])


@pytest.mark.parametrize("tda", [True, False], ids=["tda", "tddft"])
def test_a_collapsed_space_reaches_the_same_roots(tda):
    """H2O / def2-SVP (95 pairs), three roots in a space of at most 12: it collapses onto the current roots and grows again."""
    inp, res, rb = state("LDA", 1, "def2-svp")
    seen = []
    out = ex.excitations(inp, res, rb, "LDA", nroots=3, tda=tda, max_space=12, log=seen.append)
    w, f = ed.dense_solution(*dense("LDA", 1, "def2-svp"), tda)
    sizes = [int(line.split("space ")[1].split(",")[0]) for line in seen]
    print(f"space per iteration {sizes}, trial vectors {out['sigma_builds']}")
    assert out["converged"] and max(sizes) <= 12 and any(b < a for a, b in zip(sizes, sizes[1:])) and out["sigma_builds"] > 12
    assert np.abs(out["energies"] - w[:3]).max() <= 1e-9 and np.abs(out["oscillator_strengths"] - f[:3]).max() <= 1e-6


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_lowest_tddft_root_is_below_the_lowest_tda_root(functional):
    _, ApB, AmB = dense(functional, 1)
    assert np.linalg.eigvalsh(0.5 * (ApB + ApB.T))[0] > 0.0 and np.linalg.eigvalsh(0.5 * (AmB + AmB.T))[0] > 0.0
    inp, res, rb = state(functional, 1)
    w = ex.excitations(inp, res, rb, functional, nroots=1)["energies"][0]
    w_tda = ex.excitations(inp, res, rb, functional, nroots=1, tda=True)["energies"][0]
    assert 0.0 < w <= w_tda


def test_b3lyp_operators_are_symmetric_and_k_of_the_antisymmetric_density_is_the_einsum():
    ops, ApB, AmB = dense("B3LYP", 1)
    assert np.abs(AmB - AmB.T).max() <= 1e-12 and np.abs(ApB - ApB.T).max() <= 1e-12
    assert np.abs(AmB - np.diag(ops.gap.reshape(-1))).max() > 1e-3        # exact exchange does enter A-B
    inp, _, rb = state("B3LYP", 1)
    Z = np.random.default_rng(5).standard_normal((2,) + ops.gap.shape)
    Bs = 2.0 * np.einsum("na,kia->kni", ops.Cv, Z)
    _, M, _ = rb.excitation_parts(ops.Co, Bs, True)
    for k in range(2):
        AB = ops.Co @ Bs[k].T
        Dm = AB - AB.T
        ref = np.einsum("ikjl,kl->ij", inp.eri, Dm)
        assert np.abs((M[k] - M[k].T) - ref).max() <= 1e-13 * np.abs(ref).max()
        ref = np.einsum("ikjl,kl->ij", inp.eri, AB + AB.T)
        assert np.abs((M[k] + M[k].T) - ref).max() <= 1e-13 * np.abs(ref).max()


def test_pure_functionals_request_no_exchange():
    ops, _, AmB = dense("LDA", 1)
    assert not ops.want_k and np.array_equal(AmB, np.diag(ops.gap.reshape(-1)))


def test_refusals():
    inp, res, rb = state("LDA", 1)
    with pytest.raises(ValueError, match="10 occupied-virtual pairs"):
        ex.excitations(inp, res, rb, "LDA", nroots=11)
    with pytest.raises(ValueError, match="--quirks 0"):
        ex.excitations(inp, res, response.HostResponse(inp, "GGA", rb.scf, rb.ao, rb.gr, quirks=True), "GGA", nroots=1)
    # an unstable reference: one gap of the (otherwise untouched) operators negated makes A-B = diag(gap) indefinite
    ops, _, _ = dense("LDA", 1)
    gap = ops.gap.copy()
    gap.reshape(-1)[np.argmin(gap)] *= -1.0
    bad = types.SimpleNamespace(gap=gap, dip=ops.dip, builds=0,
                                apply=lambda Z: tuple(x + (gap - ops.gap)[None] * Z for x in ops.apply(Z)))
    with pytest.raises(ValueError, match="unstable"):
        ex.solve(bad, nroots=2)
    with pytest.raises(ValueError, match="unstable"):
        ex.solve(bad, nroots=2, tda=True)
