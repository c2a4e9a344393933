"""Reader of tests/golden/point_field_ref_*.npz (written by tests/golden/make_point_field_reference.py) and what the CPU and
GPU tests of the field of a density at points share.  Needs neither mpmath nor the oracle package."""
import functools

import numpy as np

import eri_fixtures
import point_coulomb_fixtures as PF
from point_coulomb_fixtures import BOUND, class_masks, densities  # noqa: F401  (re-exported)


@functools.lru_cache(maxsize=None)
def family(name):
    """dict: sh (ShellTable of eri_ref_<name>.npz), points (P, 3), dA (P, 3, nao, nao), meta."""
    d = eri_fixtures._load(f"point_field_ref_{name}.npz")
    pot = PF.family(name)
    sh = pot["sh"]
    assert d["dA"].shape == (len(d["points"]), 3, sh.nao, sh.nao)
    assert np.array_equal(d["points"], pot["points"][d["point_index"]])
    for a in (d["points"], d["dA"]):
        a.setflags(write=False)
    return dict(sh=sh, points=d["points"], dA=d["dA"], meta=d["meta"])


def contract_reference(D, dA):
    """(values (P, 3), allowed error per point and component): einsum against the stored derivatives;
    BOUND * max(1, sum |D| |dA[c, k]|)."""
    return np.einsum("ij,ckij->ck", D, dA), BOUND * np.maximum(1.0, np.einsum("ij,ckij->ck", np.abs(D), np.abs(dA)))


@functools.lru_cache(maxsize=None)
def references(name):
    """[(label, D, reference (P, 3), allowed (P, 3))] for the full and the ten class-masked matrices; computed once."""
    f = family(name)
    out = []
    for label, D in densities(f["sh"]):
        ref, allowed = contract_reference(D, f["dA"])
        for a in (D, ref, allowed):
            a.setflags(write=False)
        out.append((label, D, ref, allowed))
    return out


def unit_matrix_from_contractions(field, sh):
    """dA[c, k, mu, nu] (symmetric in mu, nu) out of a contraction `field(D) -> (P, 3)`: D = e_mu e_nu^T, mu >= nu."""
    n = sh.nao
    got = None
    for i in range(n):
        for j in range(i + 1):
            D = np.zeros((n, n))
            D[i, j] = 1.0
            g = field(D)
            if got is None:
                got = np.zeros(g.shape + (n, n))
            got[:, :, i, j] = got[:, :, j, i] = g
    return got


def class_ratios(err_over_allowed, sh):
    """{(la, lb): max of an (..., nao, nao) array of error / allowed over the class's blocks}."""
    return {k: float(err_over_allowed[..., m].max()) for k, m in class_masks(sh).items()}


def print_class_table(title, ratios):
    print(f"\n{title}")
    for (la, lb), r in sorted(ratios.items()):
        print(f"  ({'spdf'[la]}{'spdf'[lb]})  {r:.2e}")
