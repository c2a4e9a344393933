"""Host counterparts of the meta-GGA sweeps (DFT_ComputeTau / DFT_ComputeXCMeta and their open-shell forms): the bodies of csrc/xc_meta_functionals.hpp
through lib/libqcfxc.so (g++), the contractions in numpy.  The CPU tests hold these against a 60-digit reference, exact
constraints and finite differences; the GPU tests hold the device against these.

tau(g) = 1/2 sum_k sum_mu,nu D[mu, nu] (d_k phi_mu)(g) (d_k phi_nu)(g); the closed shell evaluates the spin-resolved bodies at
(rho/2, rho/2, sigma/4, sigma/4, sigma/4, tau/2, tau/2).
"""
import ctypes

import numpy as np

from . import functionals
from .build import fxc_host_library_path

_lib = None


def _load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(fxc_host_library_path())
        dp = ctypes.POINTER(ctypes.c_double)
        L.qc_meta_point.restype = ctypes.c_int
        L.qc_meta_point.argtypes = [dp, dp, ctypes.c_longlong, dp, dp, dp, dp, dp]
        L.qc_meta_energy_spin.restype = ctypes.c_int
        L.qc_meta_energy_spin.argtypes = [dp, dp, ctypes.c_longlong] + [dp] * 9
        L.qc_meta_point_spin.restype = ctypes.c_int
        L.qc_meta_point_spin.argtypes = [dp, dp, ctypes.c_longlong] + [dp] * 8
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


def _weights(functional):
    """(eight weights, two meta weights) of a functional name / expression / Functional, or of a pair of sequences."""
    if isinstance(functional, (tuple, list)) and len(functional) == 2 and not isinstance(functional[0], str):
        w8, w2 = (np.ascontiguousarray(x, dtype=np.float64) for x in functional)
        if w8.shape != (len(functionals.COMPONENTS),) or w2.shape != (len(functionals.META_COMPONENTS),):
            raise ValueError("weights: eight component weights and two meta weights")
        return w8, w2
    f = functionals.resolve(functional)
    return np.array(f.weight_vector()), np.array(f.meta_weight_vector())


def _c(x, shape=None):
    x = np.asarray(x, dtype=np.float64)
    if shape is not None:
        x = np.broadcast_to(x, shape)
    return np.ascontiguousarray(x)


def point_meta_host(functional, rho, grad, tau, weights):
    """One closed-shell point per entry, xc::meta_point as the device's pointwise kernel runs it.  rho (n,), grad (n, 3) = grad
    rho, tau (n,), weights (n,).  Returns a dict: e (energy per volume, no weight), coef (4, n) = c0..c3 (c0 = w e_rho,
    c_k = 4 w e_sigma grad_k rho), ct = w e_tau / 2, and the bare derivatives vrho, vsigma, vtau."""
    w8, w2 = _weights(functional)
    rho = _c(np.atleast_1d(rho))
    n = rho.size
    grad, tau, weights = _c(grad, (n, 3)), _c(tau, (n,)), _c(weights, (n,))
    out = np.zeros((10, n))
    if _load().qc_meta_point(_p(w8), _p(w2), n, _p(rho), _p(grad), _p(tau), _p(weights), _p(out)) != 0:
        raise ValueError("point_meta_host: bad arguments")
    return {"e": out[0], "coef": out[1:5], "ct": out[5], "vrho": out[6], "vsigma": out[7], "vtau": out[8]}


def meta_energy_host(functional, ra, rb, saa, sab, sbb, ta, tb, grad=False):
    """(n,): the energy per volume of the functional's components (no exact exchange) at any polarisation, the
    spin-resolved bodies in double.  grad=True: (e, de) with de (7, n) the derivatives by (ra, rb, saa, sab, sbb, ta, tb);
    a variable of a spin channel below the density cut-off is not differentiated (its entry is exactly 0)."""
    w8, w2 = _weights(functional)
    ra = _c(np.atleast_1d(ra))
    n = ra.size
    a = [ra] + [_c(x, (n,)) for x in (rb, saa, sab, sbb, ta, tb)]
    out = np.zeros(n)
    de = np.zeros((7, n)) if grad else None
    if _load().qc_meta_energy_spin(_p(w8), _p(w2), n, *(_p(x) for x in a), _p(out), _p(de)) != 0:
        raise ValueError("meta_energy_host: bad arguments")
    return (out, de) if grad else out


def tau_host(dm, ao_grad):
    """(ngrid,): tau of dm (its symmetric part) from the three gradient planes ao_grad (3, ngrid, nao)."""
    ds = 0.5 * (dm + dm.T)
    return 0.5 * sum(np.einsum("gm,gm->g", ao_grad[k] @ ds, ao_grad[k]) for k in range(3))


def density_host(dm, ao, ao_grad):
    """rho (ngrid,), grad rho (ngrid, 3) and tau (ngrid,) of dm (its symmetric part)."""
    ds = 0.5 * (dm + dm.T)
    x = ao @ ds
    rho = np.einsum("gm,gm->g", x, ao)
    grad = np.stack([2.0 * np.einsum("gm,gm->g", x, ao_grad[k]) for k in range(3)], axis=1)
    return rho, grad, tau_host(dm, ao_grad)


def xc_meta_host(functional, dm, ao, weights, ao_grad):
    """(Exc, V) of DFT_ComputeXCMeta in numpy: V = AO^T diag(c0) AO + sum_k (c_k AO)^T (d_k AO) (one-sided, the mix solver's
    convention) + sum_k (d_k AO)^T diag(ct) (d_k AO); (V + V^T)/2 is dExc/dD."""
    rho, grad, tau = density_host(dm, ao, ao_grad)
    p = point_meta_host(functional, rho, grad, tau, weights)
    exc = float(np.sum(weights * p["e"]))
    c = p["coef"]
    q = c[0][:, None] * ao + sum(c[1 + k][:, None] * ao_grad[k] for k in range(3))
    v = q.T @ ao
    v += sum((p["ct"][:, None] * ao_grad[k]).T @ ao_grad[k] for k in range(3))
    return exc, v


# ---- open shell (DFT_ComputeTauSpin / DFT_ComputeXCMetaSpin) -------------------------------------------------------------------
def point_meta_spin_host(functional, ra, rb, grad_a, grad_b, ta, tb, weights):
    """One point per entry at any polarisation, xc::meta_spin_point as the device's pointwise kernel runs it.  ra, rb, ta, tb,
    weights (n,), grad_a, grad_b (n, 3).  Returns a dict: e (energy per volume, no weight), coef_a / coef_b (4, n) = c0..c3 of
    each spin (c0_s = w e_rho_s, c_s,k = 2 w (2 e_sigma_ss grad rho_s + e_sigma_ab grad rho_s')_k), ct_a / ct_b = w e_tau_s / 2,
    and de (7, n), the bare derivatives by (ra, rb, saa, sab, sbb, ta, tb).  A spin channel below the density cut-off is
    absent: exact zeros in everything of its own."""
    w8, w2 = _weights(functional)
    ra = _c(np.atleast_1d(ra))
    n = ra.size
    rb, ta, tb, weights = (_c(x, (n,)) for x in (rb, ta, tb, weights))
    grad_a, grad_b = _c(grad_a, (n, 3)), _c(grad_b, (n, 3))
    out = np.zeros((18, n))
    if _load().qc_meta_point_spin(_p(w8), _p(w2), n, _p(ra), _p(rb), _p(grad_a), _p(grad_b), _p(ta), _p(tb), _p(weights), _p(out)) != 0:
        raise ValueError("point_meta_spin_host: bad arguments")
    return {"e": out[0], "coef_a": out[1:5], "coef_b": out[5:9], "ct_a": out[9], "ct_b": out[10], "de": out[11:18]}


def density_spin_host(dm_a, dm_b, ao, ao_grad):
    """(rho_a, grad_a, tau_a, rho_b, grad_b, tau_b): density_host of each spin's matrix."""
    return density_host(dm_a, ao, ao_grad) + density_host(dm_b, ao, ao_grad)


def xc_meta_spin_host(functional, dm_a, dm_b, ao, weights, ao_grad):
    """(Exc, V_a, V_b) of DFT_ComputeXCMetaSpin in numpy: V_s = AO^T diag(c0_s) AO + sum_k (c_s,k AO)^T (d_k AO) (one-sided) +
    sum_k (d_k AO)^T diag(ct_s) (d_k AO); (V_s + V_s^T)/2 is dExc/dD_s."""
    ra, ga, ta, rb, gb, tb = density_spin_host(dm_a, dm_b, ao, ao_grad)
    p = point_meta_spin_host(functional, ra, rb, ga, gb, ta, tb, weights)
    exc = float(np.sum(weights * p["e"]))
    out = []
    for c, ct in ((p["coef_a"], p["ct_a"]), (p["coef_b"], p["ct_b"])):
        q = c[0][:, None] * ao + sum(c[1 + k][:, None] * ao_grad[k] for k in range(3))
        v = q.T @ ao
        v += sum((ct[:, None] * ao_grad[k]).T @ ao_grad[k] for k in range(3))
        out.append(v)
    return exc, out[0], out[1]
