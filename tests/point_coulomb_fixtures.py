"""Reader of tests/golden/point_coulomb_ref_*.npz (written by tests/golden/make_point_coulomb_reference.py) and the
inputs the CPU and GPU tests of the point-Coulomb integrals share.  Needs neither mpmath nor the oracle package."""
import functools

import numpy as np

import eri_fixtures
from eri_fixtures import BOUND  # noqa: F401  (the project's bound, re-exported)


@functools.lru_cache(maxsize=None)
def family(name):
    """dict: sh (ShellTable of eri_ref_<name>.npz), points (P, 3), A (P, nao, nao), meta."""
    d = eri_fixtures._load(f"point_coulomb_ref_{name}.npz")
    sh = {"z1": eri_fixtures.z1, "z3": eri_fixtures.z3}[name]()["sh"]
    assert d["A"].shape == (len(d["points"]), sh.nao, sh.nao)
    for a in (d["points"], d["A"]):
        a.setflags(write=False)
    return dict(sh=sh, points=d["points"], A=d["A"], meta=d["meta"])


def shell_of_function(sh):
    return np.repeat(np.arange(sh.nshell), 2 * np.asarray(sh.l) + 1)


def class_masks(sh):
    """{(la, lb), la >= lb: (nao, nao) bool} -- the blocks whose two shells have these angular momenta, both triangles.
    Ten classes for s-f."""
    lf = np.asarray(sh.l)[shell_of_function(sh)]
    out = {}
    for la in range(4):
        for lb in range(la + 1):
            m = ((lf[:, None] == la) & (lf[None, :] == lb)) | ((lf[:, None] == lb) & (lf[None, :] == la))
            if m.any():
                out[la, lb] = m
    return out


def densities(sh):
    """[(label, D)]: one seeded random NON-symmetric matrix, then one per class (la, lb), non-zero in its blocks only."""
    D = np.random.default_rng(20261017).standard_normal((sh.nao, sh.nao))
    return [("full", D)] + [(f"class {la}{lb}", D * m) for (la, lb), m in class_masks(sh).items()]


def contract_reference(D, A):
    """(values, allowed error per point): einsum against the stored integrals; BOUND * max(1, sum |D| |A[c]|)."""
    return np.einsum("ij,cij->c", D, A), BOUND * np.maximum(1.0, np.einsum("ij,cij->c", np.abs(D), np.abs(A)))


def class_errors(got, ref, sh):
    """{(la, lb): max |got - ref| over the class's blocks}."""
    return {k: float(np.abs(got - ref)[m].max()) for k, m in class_masks(sh).items()}
