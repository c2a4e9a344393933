"""Expected values of a mixed functional, composed in numpy from the oracle's own pieces
(TEST INFRASTRUCTURE: lives under tests/).

    rho, grad rho   from oracle.compute_xc(1, ..., want_density=True) (type 0 for an LDA-class mix)
    per component   oracle.pointwise(k, rho, sigma, quirks); B88 closed shell: pointwise(6, rho/2, sigma/4), vsigma halved
    sums            e = sum c_k e_k, vrho = sum c_k vrho_k, vsigma = sum c_k vsigma_k; zero where rho < 1e-12
    Exc = sum w rho e,   B = w vrho phi + 4 w vsigma (grad rho . grad phi),   V = B^T phi    (one-sided, GGA convention)
"""
import time

import numpy as np

import oracle
from quantum_compute_dft_amd import functionals

RHO_CUT = 1e-12
B88 = functionals.COMPONENTS.index("b88_x")


def weight_vector(spec):
    """Eight weights in ABI order from a spec string, a Functional, or a sequence of eight numbers."""
    if isinstance(spec, (str, functionals.Functional)):
        return np.array(functionals.resolve(spec).weight_vector())
    w = np.asarray(spec, dtype=np.float64)
    assert w.shape == (len(functionals.COMPONENTS),)
    return w


def density(dm, ao, weights, ao_grad, gga):
    """(rho, grad rho (ngrid, 3), sigma) as the oracle computes them."""
    if gga:
        _, _, rho, grad = oracle.compute_xc(1, dm, ao, weights, ao_grad, want_density=True)
        return rho, grad, np.sum(grad * grad, axis=1)
    _, _, rho, _ = oracle.compute_xc(0, dm, ao, weights, None, want_density=True)
    return rho, None, np.zeros_like(rho)


def pointwise_mix(wvec, rho, sigma, quirks=True):
    """(e, vrho, vsigma) per point of the weighted sum."""
    out = np.zeros((rho.size, 3))
    for k, c in enumerate(wvec):
        if c == 0.0:
            continue
        if k == B88:
            p = oracle.pointwise(k, 0.5 * rho, 0.25 * sigma, quirks).copy()
            p[:, 2] *= 0.5
        else:
            p = oracle.pointwise(k, rho, sigma, quirks)
        out += c * p
    out[rho < RHO_CUT] = 0.0
    return out


def compute_xc_mix(spec, dm, ao, weights, ao_grad=None, quirks=True):
    """(Exc, V one-sided) of a mix: the reference for DFT_ComputeXC on a mix solver."""
    wvec = weight_vector(spec)
    gga = bool(np.any(wvec[4:] != 0.0))
    assert not gga or ao_grad is not None
    rho, grad, sigma = density(dm, ao, weights, ao_grad, gga)
    p = pointwise_mix(wvec, rho, sigma, quirks)
    exc = float(np.sum(weights * rho * p[:, 0]))
    B = (weights * p[:, 1])[:, None] * ao
    if gga:
        gphi = grad[:, 0, None] * ao_grad[0] + grad[:, 1, None] * ao_grad[1] + grad[:, 2, None] * ao_grad[2]
        B = B + (4.0 * weights * p[:, 2])[:, None] * gphi
    return exc, B.T @ ao


class MixBackend:
    """scf.run_scf backend (the set_dm / jk / xc interface of scf_oracle_backend.OracleBackend) for any mix."""

    def __init__(self, inp, spec, quirks=True):
        self.inp, self.wvec, self.q = inp, weight_vector(spec), quirks
        self.ao, self.gr = oracle.eval_ao(inp.shells, inp.grids.coords, deriv=1)

    def set_dm(self, dm):
        self.dm = np.ascontiguousarray(dm)

    def jk(self, want_k):
        return oracle.coulomb(self.inp.eri, self.dm), (oracle.exchange(self.inp.eri, self.dm) if want_k else None)

    def xc(self):
        t0 = time.time()
        e, v = compute_xc_mix(self.wvec, self.dm, self.ao, self.inp.grids.weights, self.gr, quirks=self.q)
        return e, v, time.time() - t0
