"""gradients.xc_gradient_spin_host, the host counterpart of DFT_ComputeXCGradientSpin, against finite differences of the
open-shell energy it differentiates, and against the closed-shell routine in the closed-shell limit.

G[mu, x] is d/dt of the Exc response.xc_spin_host(dm_a, dm_b) returns when, in column mu only, ao[:, mu] -> ao[:, mu] -
t ao_grad[x][:, mu] and ao_grad[k][:, mu] -> ao_grad[k][:, mu] - t ao_hess[xk][:, mu].  The reference is that derivative by
central differences at h and 2 h, Richardson-extrapolated, with the method, the step, the columns and the two assertions
of tests/xc_gradient_reference.py (check_fd: |G - D_R| <= max(10 bar, 1e-9 scale) and 10 bar <= 1e-6 scale).  Planes:
xc_gradient_reference.inputs; spin densities: spin_reference.spin_inputs (random orbitals), an unequal pair and the fully
polarised case (no beta electron at all).
"""
import functools

import numpy as np
import pytest

import spin_reference as sr
import xc_gradient_reference as xr
from quantum_compute_dft_amd import gradients, response

FUNCTIONALS = ["LDA", "GGA", "B3LYP", "BLYP"]
# (ngrid, nao, nalpha, nbeta)
CASES = [(333, 24, 5, 3), (333, 24, 3, 0), (333, 114, 9, 7)]


def spin_case(ngrid, nao, na, nb):
    """(dm_a, dm_b, ao, ao_grad, w, ao_hess): the planes of xc_gradient_reference.inputs, the densities of spin_inputs."""
    _, ao, gr, w, hs = xr.inputs(ngrid, nao)
    dm_a, dm_b = sr.spin_inputs(ngrid, nao, na, nb)[:2]
    return dm_a, dm_b, ao, gr, w, hs


@functools.lru_cache(maxsize=None)
def reference(functional, ngrid, nao, na, nb):
    """(columns, D_R (len(columns), 3), bar), as xc_gradient_reference.reference with xc_spin_host's Exc."""
    dm_a, dm_b, ao, gr, w, hs = spin_case(ngrid, nao, na, nb)
    cols = xr.COLUMNS[nao]
    a, g = ao.copy(), gr.copy()
    D = {}
    for h in (xr.H, 2.0 * xr.H):
        out = np.zeros((len(cols), 3))
        for i, mu in enumerate(cols):
            for x in range(3):
                e = []
                for t in (h, -h):
                    a[:, mu] = ao[:, mu] - t * gr[x][:, mu]
                    for k in range(3):
                        g[k][:, mu] = gr[k][:, mu] - t * hs[xr.HESS_INDEX[x][k]][:, mu]
                    e.append(response.xc_spin_host(functional, dm_a, dm_b, a, w, g)[0])
                out[i, x] = (e[0] - e[1]) / (2.0 * h)
            a[:, mu] = ao[:, mu]
            g[:, :, mu] = gr[:, :, mu]
        D[h] = out
    ref = (4.0 * D[xr.H] - D[2.0 * xr.H]) / 3.0
    return cols, ref, float(np.abs(ref - D[xr.H]).max())


@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("case", CASES)
def test_host_gradient_matches_differences_of_the_open_shell_energy(case, functional):
    dm_a, dm_b, ao, gr, w, hs = spin_case(*case)
    if case[3] == 0:
        assert not np.any(dm_b)
    cols, ref, bar = reference(functional, *case)
    G = gradients.xc_gradient_spin_host(functional, dm_a, dm_b, ao, w, gr, None if functional == "LDA" else hs)
    assert G.shape == (case[1], 3)
    xr.check_fd("cpu", f"xc_gradient_spin_host {functional} {case}", G[list(cols)], ref, bar)


@pytest.mark.parametrize("functional", FUNCTIONALS + ["PBE0"])
@pytest.mark.parametrize("shape", [(333, 24), (333, 114)])
def test_closed_shell_limit(shape, functional):
    dm, ao, gr, w, hs = xr.inputs(*shape)
    hess = None if functional == "LDA" else hs
    ref = gradients.xc_gradient_host(functional, dm, ao, w, gr, hess, False)
    G = gradients.xc_gradient_spin_host(functional, 0.5 * dm, 0.5 * dm, ao, w, gr, hess)
    err = float(np.abs(G - ref).max() / np.abs(ref).max())
    print(f"cpu xc_gradient_spin_host {functional} {shape} at dm/2, dm/2 against xc_gradient_host(quirks 0): {err:.2e}")
    assert err <= 1e-13


def test_only_the_symmetric_parts_count():
    dm_a, dm_b, ao, gr, w, hs = spin_case(333, 24, 5, 3)
    a = np.random.default_rng(2).standard_normal(dm_a.shape)
    G0 = gradients.xc_gradient_spin_host("GGA", dm_a, dm_b, ao, w, gr, hs)
    G1 = gradients.xc_gradient_spin_host("GGA", dm_a + (a - a.T), dm_b - (a - a.T), ao, w, gr, hs)
    assert np.abs(G1 - G0).max() <= 1e-12 * np.abs(G0).max()


def test_refusals():
    dm_a, dm_b, ao, gr, w, hs = spin_case(333, 24, 5, 3)
    with pytest.raises(ValueError, match="ao_grad is needed"):
        gradients.xc_gradient_spin_host("LDA", dm_a, dm_b, ao, w, None)
    with pytest.raises(ValueError, match="ao_hess is needed"):
        gradients.xc_gradient_spin_host("GGA", dm_a, dm_b, ao, w, gr, None)
