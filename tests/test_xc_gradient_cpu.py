"""Host counterparts of the XC gradient kernels (quantum_compute_dft_amd/gradients.py) against finite differences of the
oracle (tests/xc_gradient_reference.py): ao_hessian_host against Richardson differences of oracle.eval_ao(deriv=1) for
every shell type s-f, xc_gradient_host against the differences of the oracle's Exc under the column replacement that
defines G.  Central differences at h and 2 h, Richardson-extrapolated, bar = |D_R - D(h)|; both assertions of
xc_gradient_reference.check_fd in every case.
"""
import numpy as np
import pytest

import oracle
import xc_gradient_reference as xr
from quantum_compute_dft_amd import basis, gradients

MOLECULES = {
    "H2O/def2-SVP": ("O 0 0 0.1173; H 0 0.7572 -0.4692; H 0 -0.7572 -0.4692", "def2-svp"),          # s, p, d
    "CH4/def2-TZVP": ("C 0 0 0; H 0.629 0.629 0.629; H -0.629 -0.629 0.629; H -0.629 0.629 -0.629; H 0.629 -0.629 -0.629",
                      "def2-tzvp"),                                                                   # s, p, d, f: 55 functions
}


def shells_of(name):
    geom, bname = MOLECULES[name]
    syms, xyz = basis.parse_xyz(geom)
    return basis.build_shells(syms, xyz, bname)


@pytest.mark.parametrize("name", list(MOLECULES))
def test_ao_hessian_matches_differences_of_the_oracle_gradient(name):
    """hess[xk] = d(grad_x phi) / d(point_k).  h = 1e-5 bohr: the tightest primitives that reach a random point of the
    box (|r - R_A| > 0.1 for every atom) leave a t^2 term ~1e-8 of the plane maximum, the rounding of the quotient 1e-11."""
    sh = shells_of(name)
    assert sorted(set(int(l) for l in sh.l)) == ([0, 1, 2] if "SVP" in name else [0, 1, 2, 3])
    rng = np.random.default_rng(11)
    pts = rng.uniform(-3.0, 3.0, (400, 3))
    pts = pts[np.min(np.linalg.norm(pts[:, None, :] - sh.xyz[None, :, :], axis=2), axis=1) > 0.1][:200]
    assert len(pts) == 200
    hs = gradients.ao_hessian_host(sh, pts)
    h = 1e-5
    D = {}
    for step in (h, 2.0 * h):
        out = np.zeros((3, 3) + hs.shape[1:])
        for k in range(3):
            d = np.zeros(3); d[k] = step
            out[:, k] = (oracle.eval_ao(sh, pts + d, deriv=1)[1] - oracle.eval_ao(sh, pts - d, deriv=1)[1]) / (2.0 * step)
        D[step] = out
    ref = (4.0 * D[h] - D[2.0 * h]) / 3.0
    bar = float(np.abs(ref - D[h]).max())
    full = np.stack([np.stack([hs[gradients.HESS_INDEX[x][k]] for k in range(3)]) for x in range(3)])
    xr.check_fd("cpu", f"ao_hessian_host {name}", full, ref, bar)
    for l in sorted(set(int(v) for v in sh.l)):      # every shell type is held on its own scale too
        cols = np.concatenate([np.arange(sh.ao[s], sh.ao[s] + 2 * l + 1) for s in range(sh.nshell) if sh.l[s] == l])
        xr.check_fd("cpu", f"ao_hessian_host {name} l={l}", full[..., cols], ref[..., cols], float(np.abs(ref - D[h])[..., cols].max()))


def test_ao_hessian_is_symmetric_and_traceless_where_it_must_be():
    """A single s primitive exp(-a r^2): Laplacian (4 a^2 r^2 - 6 a) phi, from the six planes."""
    basis.register_basis("one-s", {"H": [(0, [(0.8, 1.0)])]})
    sh = basis.build_shells(["H"], np.zeros((1, 3)), "one-s")
    pts = np.random.default_rng(5).uniform(-2, 2, (50, 3))
    hs = gradients.ao_hessian_host(sh, pts)
    phi = oracle.eval_ao(sh, pts)[:, 0]
    r2 = np.sum(pts * pts, axis=1)
    assert np.allclose(hs[0, :, 0] + hs[3, :, 0] + hs[5, :, 0], (4 * 0.64 * r2 - 6 * 0.8) * phi, rtol=1e-13, atol=1e-15)


CASES = [("LDA", False), ("GGA", False), ("B3LYP", False), ("B3LYP", True), ("PBE0", False)]


@pytest.mark.parametrize("functional,quirks", CASES)
@pytest.mark.parametrize("shape", [(333, 24), (333, 114)])
def test_xc_gradient_host_matches_differences_of_the_oracle_energy(shape, functional, quirks):
    dm, ao, gr, w, hs = xr.inputs(*shape)
    cols, ref, bar = xr.reference(functional, *shape, quirks)
    G = gradients.xc_gradient_host(functional, dm, ao, w, gr, None if functional == "LDA" else hs, quirks)
    assert G.shape == (shape[1], 3)
    xr.check_fd("cpu", f"xc_gradient_host {functional} quirks={int(quirks)} {shape}", G[list(cols)], ref, bar)


def test_xc_gradient_host_sees_only_the_symmetric_part_of_dm():
    dm, ao, gr, w, hs = xr.inputs(333, 24)
    a = np.random.default_rng(2).standard_normal(dm.shape)
    G0 = gradients.xc_gradient_host("GGA", dm, ao, w, gr, hs, False)
    G1 = gradients.xc_gradient_host("GGA", dm + (a - a.T), ao, w, gr, hs, False)
    assert np.abs(G1 - G0).max() <= 1e-12 * np.abs(G0).max()


def test_refusals():
    dm, ao, gr, w, hs = xr.inputs(333, 24)
    with pytest.raises(ValueError, match="ao_grad is needed"):
        gradients.xc_gradient_host("LDA", dm, ao, w, None)
    with pytest.raises(ValueError, match="ao_hess is needed"):
        gradients.xc_gradient_host("GGA", dm, ao, w, gr, None)


def test_sum_over_atoms_follows_the_shell_table():
    sh = shells_of("H2O/def2-SVP")
    G = np.random.default_rng(1).standard_normal((sh.nao, 3))
    g = gradients.sum_over_atoms(sh, G)
    assert g.shape == (3, 3) and np.allclose(g.sum(axis=0), G.sum(axis=0))
    n_o = 14      # def2-SVP O: 3s 2p 1d
    assert np.allclose(g[0], G[:n_o].sum(axis=0)) and np.allclose(g[1], G[n_o:n_o + 5].sum(axis=0))
