"""Linear response: the XC kernel applied to a perturbed density, and the static polarizability from it.

    V1[dm1] = d/dt Vxc(dm0 + t dm1) at t = 0, in the convention DFT_ComputeXC writes Vxc in for the functional

On the device that is DFT_FxcPrepare / DFT_FxcApply (csrc/xc_response.hip; solver.fxc_prepare / fxc_apply).  Here is the
host counterpart -- the same functional bodies through g++ (lib/libqcfxc.so, csrc/xc_response_host.cpp), the rest in numpy
from AO planes the caller supplies -- and `polarizability`, the closed-shell coupled-perturbed Kohn-Sham equations for
a uniform field, which takes J, K and V1 of a trial dm1 from a backend: scf.HipBackend.response_parts on the device,
HostResponse here.  With option quirks = 1 the shipped vrho is not the derivative of the energy; V1 differentiates the
shipped formulas, so the response is that of the SCF equations the loop actually solves.
"""
import ctypes

import numpy as np
from scipy.linalg import eigh

from . import functionals, integrals
from .build import fxc_host_library_path

_lib = None


def _load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(fxc_host_library_path())
        dp = ctypes.POINTER(ctypes.c_double)
        L.qc_fxc_table.restype = ctypes.c_int
        L.qc_fxc_table.argtypes = [ctypes.c_int, dp, ctypes.c_int, ctypes.c_longlong, dp, dp, dp]
        L.qc_fxc_pq.restype = ctypes.c_int
        L.qc_fxc_pq.argtypes = [ctypes.c_int, dp, ctypes.c_int, ctypes.c_longlong, dp, dp, dp, dp]
        L.qc_xc_point.restype = ctypes.c_int
        L.qc_xc_point.argtypes = [ctypes.c_int, dp, ctypes.c_int, ctypes.c_longlong, dp, dp, dp, dp, dp]
        L.qc_fxc_table_spin.restype = ctypes.c_int
        L.qc_fxc_table_spin.argtypes = [ctypes.c_int, dp, ctypes.c_int, ctypes.c_longlong, dp, dp, dp]
        L.qc_spin_energy.restype = ctypes.c_int
        L.qc_spin_energy.argtypes = [dp, ctypes.c_longlong, dp, dp, dp, dp, dp, dp]
        L.qc_xc_point_spin.restype = ctypes.c_int
        L.qc_xc_point_spin.argtypes = [ctypes.c_int, dp, ctypes.c_longlong, dp, dp, dp, dp, dp, dp]
        L.qc_fxc_table_pol.restype = ctypes.c_int
        L.qc_fxc_table_pol.argtypes = [ctypes.c_int, dp, ctypes.c_longlong, dp, dp, dp, dp, dp, dp]
        _lib = L
    return _lib


# Which response table: None the shipped vrho / vsigma formulas differentiated (DFT_FxcPrepare, the default everywhere),
# "triplet" the spin-flip response of the spin-resolved energy bodies, "singlet-spin" the singlet response through the same
# bodies (DFT_FxcPrepareSpin kinds 1 and 2; independent of quirks).
SPIN_KINDS = {"triplet": 1, "singlet-spin": 2}


def spin_kind(kind):
    """0 for None / "singlet" (the shipped table), else the DFT_FxcPrepareSpin kind of a name or of 1 / 2 itself."""
    if kind is None or kind == "singlet" or kind == 0:
        return 0
    if kind in SPIN_KINDS:
        return SPIN_KINDS[kind]
    if kind in (1, 2):
        return int(kind)
    raise ValueError(f"unknown response kind {kind!r} (singlet, {', '.join(SPIN_KINDS)})")


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _kind(functional):
    """(library type 0 LDA / 1 GGA / 2 B3LYP / 3 mix, the eight weights, reads sigma) of a name, an expression, a
    Functional or a sequence of eight weights."""
    if isinstance(functional, (str, functionals.Functional)):
        f = functionals.resolve(functional)
        w = np.array(f.weight_vector(), dtype=np.float64)
        t = 3 if f.builtin_type is None else int(f.builtin_type)
    else:
        w = np.ascontiguousarray(functional, dtype=np.float64)
        if w.shape != (len(functionals.COMPONENTS),):
            raise ValueError(f"expected {len(functionals.COMPONENTS)} component weights, got shape {w.shape}")
        t = 3
    return t, w, bool(np.any(w[4:] != 0.0))


def fxc_table_host(functional, rho, sigma=None, quirks=True, kind=None):
    """(5, n): P_rho, P_sigma, Q_rho, Q_sigma, Q of the functional at (rho, sigma), where c0 = w P and c_k = w Q g_k are
    the coefficients the sweep contracts with the AO planes (no weight here).  Exactly zero below the density cut-off;
    planes 1..4 are zero for an LDA-class functional.  kind "triplet" / "singlet-spin": the same five planes from the
    spin-resolved energy bodies (csrc/xc_spin_functionals.hpp) at rho_a = rho_b -- the response of the alpha potential
    to a spin-flip / a symmetric perturbation; `quirks` plays no part there."""
    t, w, gga = _kind(functional)
    rho = np.ascontiguousarray(np.atleast_1d(rho), dtype=np.float64)
    sigma = np.zeros_like(rho) if sigma is None else np.ascontiguousarray(np.atleast_1d(sigma), dtype=np.float64)
    if sigma.shape != rho.shape or rho.ndim != 1:
        raise ValueError("rho and sigma: one-dimensional arrays of one length")
    out = np.zeros((5, rho.size))
    k = spin_kind(kind)
    if k:
        rc = _load().qc_fxc_table_spin(t, _p(w), k, rho.size, _p(rho), _p(sigma), _p(out))
    else:
        rc = _load().qc_fxc_table(t, _p(w), 1 if quirks else 0, rho.size, _p(rho), _p(sigma), _p(out))
    if rc != 0:
        raise ValueError("fxc_table_host: bad arguments")
    return out


def spin_energy_host(functional, ra, rb, saa=None, sab=None, sbb=None):
    """(n,): the energy per volume of the functional's components (no exact exchange) at the spin densities ra, rb and
    sigma_aa = |grad ra|^2, sigma_ab = grad ra . grad rb, sigma_bb, any polarisation: the spin-resolved bodies in double."""
    _, w, _ = _kind(functional)
    ra = np.ascontiguousarray(np.atleast_1d(ra), dtype=np.float64)
    a = [ra] + [np.zeros_like(ra) if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), ra.shape))
                for x in (rb, saa, sab, sbb)]
    if ra.ndim != 1:
        raise ValueError("spin_energy_host: one-dimensional arrays of one length")
    out = np.zeros(ra.size)
    if _load().qc_spin_energy(_p(w), ra.size, *(_p(x) for x in a), _p(out)) != 0:
        raise ValueError("spin_energy_host: bad arguments")
    return out


def pq_host(functional, rho, sigma, quirks=True):
    """((2, n) P and Q evaluated in double, (2, n) the value parts of the dual evaluation): for the tests that hold the
    two instantiations of the functional bodies against each other."""
    t, w, _ = _kind(functional)
    rho = np.ascontiguousarray(rho, dtype=np.float64); sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    out, dual = np.zeros((2, rho.size)), np.zeros((2, rho.size))
    if _load().qc_fxc_pq(t, _p(w), 1 if quirks else 0, rho.size, _p(rho), _p(sigma), _p(out), _p(dual)) != 0:
        raise ValueError("pq_host: bad arguments")
    return out, dual


def point_host(functional, rho, sigma, grad, weights, quirks=True):
    """(5, n): exc, c0..c3 of the point body the sweep's kernel runs for this functional, compiled for the host."""
    t, w, _ = _kind(functional)
    a = [np.ascontiguousarray(x, dtype=np.float64) for x in (rho, sigma, grad, weights)]
    out = np.zeros((5, a[0].size))
    if _load().qc_xc_point(t, _p(w), 1 if quirks else 0, a[0].size, *(_p(x) for x in a), _p(out)) != 0:
        raise ValueError("point_host: bad arguments")
    return out


def _density(dm, ao, ao_grad):
    """rho (n,) and grad rho (n, 3) of any matrix (its symmetric part counts), as the density kernels define them."""
    ds = 0.5 * (dm + dm.T)
    x = ao @ ds
    rho = np.einsum("gi,gi->g", x, ao)
    if ao_grad is None:
        return rho, None
    return rho, 2.0 * np.stack([np.einsum("gi,gi->g", x, ao_grad[k]) for k in range(3)], axis=1)


def point_spin_host(functional, ra, rb, grad_a=None, grad_b=None, weights=None):
    """(14, n): one point of the spin-resolved sweep as k_xc_points_spin evaluates it (xc::spin_potential_point compiled for
    the host): row 0 the energy per volume e (no weight), rows 1..4 the alpha coefficients c0..c3, rows 5..8 the beta ones
    (c0_s = scale w e_rho_s, c_s,k = 2 scale w (2 e_sigma_ss grad rho_s + e_sigma_ab grad rho_s')_k, scale = 1/2 for B3LYP),
    rows 9..13 the bare derivatives of e by rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb.  grad_a / grad_b (n, 3) (zeros if
    None), weights (n,) (ones if None).  A channel below the density cut-off is absent: zeros in its rows and columns."""
    t, w8, gga = _kind(functional)
    ra = np.ascontiguousarray(np.atleast_1d(ra), dtype=np.float64)
    rb = np.ascontiguousarray(np.broadcast_to(np.asarray(rb, dtype=np.float64), ra.shape))
    if ra.ndim != 1:
        raise ValueError("point_spin_host: one-dimensional arrays of one length")
    ga, gb = (np.zeros((ra.size, 3)) if g is None else np.ascontiguousarray(g, dtype=np.float64) for g in (grad_a, grad_b))
    w = np.ones(ra.size) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if ga.shape != (ra.size, 3) or gb.shape != (ra.size, 3) or w.shape != ra.shape:
        raise ValueError("point_spin_host: gradients (n, 3) and weights (n,) for n points")
    out = np.zeros((14, ra.size))
    if _load().qc_xc_point_spin(t, _p(w8), ra.size, _p(ra), _p(rb), _p(ga), _p(gb), _p(w), _p(out)) != 0:
        raise ValueError("point_spin_host: bad arguments")
    return out


def xc_spin_host(functional, dm_a, dm_b, ao, weights, ao_grad=None):
    """(Exc, V_alpha, V_beta) of the spin density matrices from AO planes in numpy, element for element what
    DFT_ComputeXCSpin leaves: one-sided for GGA-type functionals and mixes ((V + V^T)/2 is the potential), M + M^T with
    the halved coefficients for B3LYP, symmetric for LDA.  The spin-resolved bodies: no `quirks`."""
    t, _, gga = _kind(functional)
    if gga and ao_grad is None:
        raise ValueError("ao_grad is needed for a gradient-corrected functional")
    ao = np.ascontiguousarray(ao, dtype=np.float64)
    gr = np.ascontiguousarray(ao_grad, dtype=np.float64) if gga else None
    w = np.asarray(weights, dtype=np.float64)
    ra, ga = _density(np.asarray(dm_a, dtype=np.float64), ao, gr)
    rb, gb = _density(np.asarray(dm_b, dtype=np.float64), ao, gr)
    p = point_spin_host(functional, ra, rb, ga, gb, w)
    out = []
    for c in (p[1:5], p[5:9]):
        B = c[0][:, None] * ao
        if gga:
            for k in range(3):
                B += c[1 + k][:, None] * gr[k]
        M = B.T @ ao
        out.append(M + M.T if t == 2 else M)
    return float(w @ p[0]), out[0], out[1]


def fxc_table_pol_host(functional, ra, rb, grad_a=None, grad_b=None):
    """(H (5, 5, n), g (5, n)): the bare second and first derivatives of the energy per volume by x = (rho_a, rho_b,
    sigma_aa, sigma_ab, sigma_bb) at any polarisation -- the table of DFT_FxcPrepareSpinPol without the weight and without
    the factor of the built-in type, xc::spin_hessian_entry compiled for the host.  H[i, j] is evaluated with x_i as the
    first direction (the potential's variable) and x_j as the second (the perturbation): symmetric except at a sigma
    cut-off of PBE exchange or correlation.  grad_a / grad_b (n, 3), zeros if None.  A channel below the density cut-off is
    absent: exact zeros in its rows, columns and g.  An LDA-class functional leaves the sigma rows and columns zero."""
    t, w8, gga = _kind(functional)
    ra = np.ascontiguousarray(np.atleast_1d(ra), dtype=np.float64)
    rb = np.ascontiguousarray(np.broadcast_to(np.asarray(rb, dtype=np.float64), ra.shape))
    if ra.ndim != 1:
        raise ValueError("fxc_table_pol_host: one-dimensional arrays of one length")
    ga, gb = (np.zeros((ra.size, 3)) if g is None else np.ascontiguousarray(g, dtype=np.float64) for g in (grad_a, grad_b))
    if ga.shape != (ra.size, 3) or gb.shape != (ra.size, 3):
        raise ValueError("fxc_table_pol_host: gradients (n, 3) for n points")
    H, g1 = np.zeros((5, 5, ra.size)), np.zeros((5, ra.size))
    if _load().qc_fxc_table_pol(t, _p(w8), ra.size, _p(ra), _p(rb), _p(ga), _p(gb), _p(H), _p(g1)) != 0:
        raise ValueError("fxc_table_pol_host: bad arguments")
    return H, g1


class HostFxcSpin:
    """DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol on the host: the table at (dm0_a, dm0_b) once, then (V1_a, V1_b) of any
    number of perturbations (dm1_a, dm1_b), in numpy -- element for element what the device entries leave."""

    def __init__(self, functional, dm0_a, dm0_b, ao, weights, ao_grad=None):
        self.type, self.w8, self.gga = _kind(functional)
        if self.gga and ao_grad is None:
            raise ValueError("ao_grad is needed for a gradient-corrected functional")
        self.ao = np.ascontiguousarray(ao, dtype=np.float64)
        self.gr = np.ascontiguousarray(ao_grad, dtype=np.float64) if self.gga else None
        self.ra, self.ga = _density(np.asarray(dm0_a, dtype=np.float64), self.ao, self.gr)
        self.rb, self.gb = _density(np.asarray(dm0_b, dtype=np.float64), self.ao, self.gr)
        H, g = fxc_table_pol_host(functional, self.ra, self.rb, self.ga, self.gb)
        sw = (0.5 if self.type == 2 else 1.0) * np.asarray(weights, dtype=np.float64)      # B3LYP: the library's M + M^T
        self.H, self.g = H * sw, g * sw

    def apply(self, dm1_a, dm1_b):
        ra1, ga1 = _density(np.asarray(dm1_a, dtype=np.float64), self.ao, self.gr)
        rb1, gb1 = _density(np.asarray(dm1_b, dtype=np.float64), self.ao, self.gr)
        H = self.H
        if not self.gga:
            c = [H[0, 0] * ra1 + H[0, 1] * rb1, H[1, 0] * ra1 + H[1, 1] * rb1]
            return tuple((ck * self.ao.T) @ self.ao for ck in c)
        dot = lambda u, v: np.einsum("gk,gk->g", u, v)
        x1 = np.stack([ra1, rb1, 2.0 * dot(self.ga, ga1), dot(self.ga, gb1) + dot(self.gb, ga1), 2.0 * dot(self.gb, gb1)])
        t = np.einsum("ijg,jg->ig", H, x1)
        g2, g3, g4 = self.g[2], self.g[3], self.g[4]
        ca = 2.0 * ((2.0 * t[2])[:, None] * self.ga + (2.0 * g2)[:, None] * ga1 + t[3][:, None] * self.gb + g3[:, None] * gb1)
        cb = 2.0 * ((2.0 * t[4])[:, None] * self.gb + (2.0 * g4)[:, None] * gb1 + t[3][:, None] * self.ga + g3[:, None] * ga1)
        out = []
        for c0, ck in ((t[0], ca), (t[1], cb)):
            B = c0[:, None] * self.ao
            for k in range(3):
                B += ck[:, k, None] * self.gr[k]
            M = B.T @ self.ao
            out.append(M + M.T if self.type == 2 else M)
        return out[0], out[1]


def fxc_apply_spinpol_host(functional, dm0_a, dm0_b, dm1_a, dm1_b, ao, weights, ao_grad=None):
    """(V1_a, V1_b) = d/dt of xc_spin_host(dm0_a + t dm1_a, dm0_b + t dm1_b)'s potentials at t = 0, from AO planes in
    numpy and in xc_spin_host's conventions: what DFT_FxcApplySpinPol leaves."""
    return HostFxcSpin(functional, dm0_a, dm0_b, ao, weights, ao_grad).apply(dm1_a, dm1_b)


class HostFxc:
    """fxc_prepare / fxc_apply on the host: the table at dm0 once, then V1 of any number of perturbations."""

    def __init__(self, functional, dm0, ao, weights, ao_grad=None, quirks=True, kind=None):
        self.type, self.w8, self.gga = _kind(functional)
        if self.gga and ao_grad is None:
            raise ValueError("ao_grad is needed for a gradient-corrected functional")
        self.ao = np.ascontiguousarray(ao, dtype=np.float64)
        self.gr = np.ascontiguousarray(ao_grad, dtype=np.float64) if self.gga else None
        rho, self.g0 = _density(np.asarray(dm0, dtype=np.float64), self.ao, self.gr)
        sigma = np.einsum("gk,gk->g", self.g0, self.g0) if self.gga else None
        self.table = fxc_table_host(functional, rho, sigma, quirks, kind) * np.asarray(weights, dtype=np.float64)[None, :]

    def apply(self, dm1):
        rho1, g1 = _density(np.asarray(dm1, dtype=np.float64), self.ao, self.gr)
        T = self.table
        if not self.gga:
            return (T[0] * rho1 * self.ao.T) @ self.ao
        s1 = 2.0 * np.einsum("gk,gk->g", self.g0, g1)
        B = (T[0] * rho1 + T[1] * s1)[:, None] * self.ao
        ck = (T[2] * rho1 + T[3] * s1)[:, None] * self.g0 + T[4][:, None] * g1
        for k in range(3):
            B += ck[:, k, None] * self.gr[k]
        M = B.T @ self.ao
        return M + M.T if self.type == 2 else M      # B3LYP: the library's M + M^T with the halved vrho


def fxc_apply_host(functional, dm0, dm1, ao, weights, ao_grad=None, quirks=True, kind=None):
    """V1 = d/dt Vxc(dm0 + t dm1) at t = 0 from AO planes, in numpy: one-sided for GGA-type functionals and mixes, M + M^T
    with the halved vrho for B3LYP, symmetric for LDA -- element for element what DFT_FxcApply leaves.  kind "triplet":
    d/dt of the alpha-spin potential under dm_alpha, dm_beta = dm0/2 +- t dm1/2, in the same conventions (what
    DFT_FxcApplyKind leaves for kind 1); "singlet-spin": the singlet V1 through the spin-resolved bodies."""
    return HostFxc(functional, dm0, ao, weights, ao_grad, quirks, kind).apply(dm1)


class HostResponse:
    """Response backend on the host for `polarizability`: J and K of dm1 from the dense ERI of `inp`, V1 from HostFxc
    on the AO planes given.  `scf_backend` (set_dm / jk / xc, what the SCF ran on) supplies the ground-state Fock parts."""

    def __init__(self, inp, functional, scf_backend, ao, ao_grad=None, quirks=True):
        if inp.eri is None:
            raise ValueError("HostResponse needs the dense ERI")
        self.inp, self.functional, self.scf, self.q = inp, functional, scf_backend, quirks
        self.quirks = bool(quirks)
        self.ao, self.gr, self.fxc, self.fxc_spin = ao, ao_grad, None, {}

    def ground_state_parts(self, dm, cocc, want_k):
        self.scf.set_dm(dm)
        J, K = self.scf.jk(want_k)
        _, V, _ = self.scf.xc()
        return J, K, V

    def response_prepare(self, dm0, cocc=None, kind=None):
        k = spin_kind(kind)
        if k:
            self.fxc_spin[k] = HostFxc(self.functional, dm0, self.ao, self.inp.grids.weights, self.gr, self.q, k)
        else:
            self.fxc = HostFxc(self.functional, dm0, self.ao, self.inp.grids.weights, self.gr, self.q)

    def response_parts(self, dm1, want_k, factors=None):
        J = np.einsum("ijkl,kl->ij", self.inp.eri, dm1)
        K = np.einsum("ikjl,kl->ij", self.inp.eri, dm1) if want_k else None
        return J, K, self.fxc.apply(dm1)

    def excitation_parts(self, A, Bs, want_k, kind=None):
        """(J, M or None, V1), each (nvec, nao, nao), of the trials D_k = A B_k^T + B_k A^T: J[D_k], the unsymmetrised
        M_k = K[A B_k^T] (K[D]_mn = sum_ls (ml|ns) D_ls, so K[A B_k^T +- B_k A^T] = M_k +- M_k^T) and V1[D_k].
        kind "triplet": V1 from the spin-flip table (response_prepare(kind="triplet") first) and no J (None)."""
        A, Bs = np.asarray(A, dtype=np.float64), np.asarray(Bs, dtype=np.float64)
        AB = np.einsum("mi,kni->kmn", A, Bs)
        Dp = AB + AB.transpose(0, 2, 1)
        k = spin_kind(kind)
        if k and k not in self.fxc_spin:
            raise ValueError(f"excitation_parts: response_prepare(kind={kind!r}) has not run")
        fxc = self.fxc_spin[k] if k else self.fxc
        J = np.einsum("ijkl,nkl->nij", self.inp.eri, Dp) if k != 1 else None
        M = np.einsum("ikjl,nkl->nij", self.inp.eri, AB) if want_k else None
        return J, M, np.stack([fxc.apply(d) for d in Dp])


class HostUksResponse:
    """Open-shell response backend on the host: uks_response_prepare / uks_excitation_parts as scf.HipBackend offers them,
    from the dense ERI of `inp` and HostFxcSpin on the AO planes given.  `scf_backend` (uks_parts, what run_uks ran on)
    supplies the ground-state Fock parts.  A functional without a density-functional component has V1 = 0."""

    def __init__(self, inp, functional, scf_backend, ao=None, ao_grad=None, quirks=False):
        if inp.eri is None:
            raise ValueError("HostUksResponse needs the dense ERI")
        self.inp, self.functional, self.scf, self.quirks = inp, functional, scf_backend, bool(quirks)
        self.ao, self.gr, self.fxc = ao, ao_grad, None
        self.sweep = bool(functionals.resolve(functional).weights)
        if self.sweep and ao is None:
            raise ValueError("HostUksResponse needs the AO planes for a functional with a density-functional component")

    def uks_parts(self, dm_a, dm_b, cocc_a, cocc_b, want_k):
        return self.scf.uks_parts(dm_a, dm_b, cocc_a, cocc_b, want_k)

    def uks_response_prepare(self, dm_a, dm_b):
        if self.sweep:
            self.fxc = HostFxcSpin(self.functional, dm_a, dm_b, self.ao, self.inp.grids.weights, self.gr)

    def uks_excitation_parts(self, A_a, Bs_a, A_b, Bs_b, want_k):
        """(J, M_a, M_b, V1_a, V1_b), each (nvec, nao, nao) (M_s None without want_k), of the trials D_s,k = A_s B_s,k^T +
        B_s,k A_s^T: J[D_a,k + D_b,k], the unsymmetrised M_s,k = K[A_s B_s,k^T], and the raw V1_s of the pair."""
        AB = [np.einsum("mi,kni->kmn", np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))
              for A, B in ((A_a, Bs_a), (A_b, Bs_b))]
        Dp = [x + x.transpose(0, 2, 1) for x in AB]
        J = np.einsum("ijkl,nkl->nij", self.inp.eri, Dp[0] + Dp[1])
        M = [np.einsum("ikjl,nkl->nij", self.inp.eri, x) if want_k else None for x in AB]
        if self.sweep:
            if self.fxc is None:
                raise ValueError("uks_excitation_parts: uks_response_prepare has not run")
            V = [self.fxc.apply(da, db) for da, db in zip(Dp[0], Dp[1])]
            V1a, V1b = np.stack([v[0] for v in V]), np.stack([v[1] for v in V])
        else:
            V1a, V1b = np.zeros_like(J), np.zeros_like(J)
        return J, M[0], M[1], V1a, V1b


_PBE_C = functionals.COMPONENTS.index("pbe_c")
_VWN5_C = functionals.COMPONENTS.index("vwn5_c")


def uks_orbitals(inp, uks_result, backend, functional=None):
    """Canonical orbitals of a converged run_uks state for the open-shell response: one eigh(F_s, S) per spin of the Fock
    matrices of the converged densities (backend.uks_parts), then backend.uks_response_prepare.  Returns (f, spins) with
    f the resolved functional and spins a list of two dicts {Co (nao, n_s), Cv (nao, nv_s), gap (n_s, nv_s)}."""
    f = functionals.resolve(functional if functional is not None else backend.functional)
    functionals.refuse_meta(f, "open-shell response")
    wv = f.weight_vector()
    if bool(getattr(backend, "quirks", False)) and (wv[_VWN5_C] != 0.0 or wv[_PBE_C] != 0.0):
        raise ValueError("open-shell response: the spin-resolved kernel is the second derivative of the energy, but with quirks = 1 the "
                         "shipped vwn5_c / pbe_c potentials are not the derivatives of their energies; run with --quirks 0")
    for k in ("dm_a", "dm_b", "nalpha", "nbeta"):
        if k not in uks_result:
            raise ValueError("open-shell response needs a scf.run_uks result (dm_a, dm_b, nalpha, nbeta)")
    want_k = f.c_hf != 0.0
    S = inp.S
    dms = [np.ascontiguousarray(uks_result[k], dtype=np.float64) for k in ("dm_a", "dm_b")]
    ns = [int(uks_result["nalpha"]), int(uks_result["nbeta"])]
    coccs = []
    for dm, n in zip(dms, ns):      # dm_s S is the projector on the occupied orbitals of spin s
        e0, C0 = eigh(S @ dm @ S, S)
        coccs.append(np.ascontiguousarray(C0[:, ::-1][:, :n] * np.sqrt(np.maximum(e0[::-1][:n], 0.0))))
    J, Ka, Kb, _, Va, Vb = backend.uks_parts(dms[0], dms[1], coccs[0], coccs[1], want_k)
    spins = []
    for V, K, n in ((Va, Ka, ns[0]), (Vb, Kb, ns[1])):
        F = inp.Hcore + J + 0.5 * (V + V.T) - (f.c_hf * K if want_k else 0.0)
        e, C = eigh(F, S)
        gap = np.ascontiguousarray(e[None, n:] - e[:n, None])
        if gap.size and gap.min() <= 1e-6:
            raise ValueError("open-shell response: no gap between the occupied and the virtual orbitals of one spin")
        spins.append({"Co": np.ascontiguousarray(C[:, :n]), "Cv": np.ascontiguousarray(C[:, n:]), "gap": gap})
    if not (spins[0]["gap"].size + spins[1]["gap"].size):
        raise ValueError("open-shell response: no occupied-virtual pairs")
    backend.uks_response_prepare(dms[0], dms[1])
    return f, spins


def _polarizability_uks(inp, uks_result, backend, functional, tol, max_iter, log):
    """The unrestricted CPKS equations (occupation 1, K enters with c_hf): per spin s

        (e_a - e_i) U_s,ai + [C_vs^T G_s C_os]_ai = -[C_vs^T D_k C_os]_ai,     dm1_s = C_vs U_s C_os^T + transpose
        G_s = J[dm1_a + dm1_b] + (V1_s + V1_s^T)/2 - c_hf K[dm1_s],             alpha_kl = -tr((dm1_a + dm1_b)(l) D_k)

    on the stacked unknown (U_a, U_b), every step through one backend.uks_excitation_parts call with one trial."""
    f, sp = uks_orbitals(inp, uks_result, backend, functional)
    c_hf, want_k = f.c_hf, f.c_hf != 0.0
    D = integrals.dipole(inp.shells)
    shapes = [(s["Cv"].shape[1], s["Co"].shape[1]) for s in sp]
    na = shapes[0][0] * shapes[0][1]
    gaps = [s["gap"].T for s in sp]                                              # (nv_s, n_s)

    def split(u):
        return [u[:na].reshape(shapes[0]), u[na:].reshape(shapes[1])]

    def dms_of(u):
        Bs = [s["Cv"] @ U for s, U in zip(sp, split(u))]                        # (nao, n_s)
        out = []
        for s, B in zip(sp, Bs):
            M = B @ s["Co"].T
            out.append(M + M.T)
        return out, Bs

    def apply_a(u):
        _, Bs = dms_of(u)
        J, Ma, Mb, Va, Vb = backend.uks_excitation_parts(sp[0]["Co"], Bs[0][None], sp[1]["Co"], Bs[1][None], want_k)
        out = []
        for s, V, M, gap in zip(sp, (Va, Vb), (Ma, Mb), gaps):
            G = J[0] + 0.5 * (V[0] + V[0].T) - (c_hf * (M[0] + M[0].T) if want_k else 0.0)
            out.append(((s["Cv"].T @ G @ s["Co"]) / gap).reshape(-1))
        return np.concatenate(out)

    alpha, its, ress, dm1s = np.zeros((3, 3)), [], [], []
    for l in range(3):
        b = -np.concatenate([((s["Cv"].T @ D[l] @ s["Co"]) / gap).reshape(-1) for s, gap in zip(sp, gaps)])
        u, n, r = _gmres(apply_a, b, tol, max_iter)
        d, _ = dms_of(u)
        dm1 = d[0] + d[1]
        alpha[:, l] = -np.einsum("kij,ji->k", D, dm1)
        its.append(n); ress.append(r); dm1s.append(dm1)
        if log:
            log(f"CPKS direction {'xyz'[l]}: {n} iterations, residual {r:.2e}")
    return {"alpha": alpha, "cpks_iterations": its, "residual": ress, "dipole_integrals": D, "dm1": dm1s}


def _gmres(apply_a, b, tol, max_iter):
    """x with |(1 + A) x - b|_2 <= tol by GMRES without restarts: (x, matrix-vector products, final residual norm)."""
    beta = float(np.linalg.norm(b))
    if beta <= tol:
        return np.zeros_like(b), 0, beta
    Q, H = [b / beta], np.zeros((max_iter + 1, max_iter))
    y, res = np.zeros(0), beta
    for j in range(max_iter):
        w = Q[j] + apply_a(Q[j])
        for _ in range(2):                      # Gram-Schmidt, twice
            for i in range(j + 1):
                h = float(Q[i] @ w)
                H[i, j] += h
                w = w - h * Q[i]
        H[j + 1, j] = float(np.linalg.norm(w))
        rhs = np.zeros(j + 2); rhs[0] = beta
        y = np.linalg.lstsq(H[:j + 2, :j + 1], rhs, rcond=None)[0]
        res = float(np.linalg.norm(rhs - H[:j + 2, :j + 1] @ y))
        if res <= tol or H[j + 1, j] <= 1e-300:
            break
        Q.append(w / H[j + 1, j])
    return sum(c * q for c, q in zip(y, Q)), len(y), res


def polarizability(inp, scf_result, backend, functional=None, tol=1e-8, max_iter=60, log=None):
    """Static dipole polarizability alpha (3, 3) in a.u. of the converged closed-shell state `scf_result` (scf.run_scf),
    by the coupled-perturbed Kohn-Sham equations for the three directions of a uniform field:

        (e_a - e_i) U_ai + [C_v^T G[dm1(U)] C_o]_ai = -[C_v^T D_k C_o]_ai,    dm1 = 2 (C_v U C_o^T + C_o U^T C_v^T)
        G[dm1] = J[dm1] - c_hf/2 K[dm1] + (V1 + V1^T)/2 [dm1],               alpha_kl = -tr(dm1(l) D_k)

    Canonical orbitals come from one eigh(F, S) of the Fock matrix of the converged density.  Each direction is solved
    by GMRES on the equations divided by e_a - e_i, to a residual 2-norm `tol`; every step takes J, K and V1 of one
    symmetric dm1 from `backend` (response_prepare / response_parts; ground_state_parts for the Fock matrix).  Returns
    {"alpha", "cpks_iterations" (per direction), "residual" (per direction), "dipole_integrals", "dm1" (per direction)}.

    A scf.run_uks result (uks = True) is solved by the unrestricted equations (_polarizability_uks) through
    backend.uks_parts / uks_response_prepare / uks_excitation_parts; the same fields come back."""
    if scf_result.get("uks"):
        return _polarizability_uks(inp, scf_result, backend, functional, tol, max_iter, log)
    f = functionals.resolve(functional if functional is not None else backend.functional)
    functionals.refuse_meta(f, "polarizability (CPKS)")
    c_hf, want_k = f.c_hf, f.c_hf != 0.0
    S, nocc = inp.S, inp.nocc
    dm0 = np.ascontiguousarray(scf_result["dm"], dtype=np.float64)
    # occupied orbitals of the converged density (dm0 S is the projector on them, doubled), for the ground-state parts
    e0, C0 = eigh(inp.S @ dm0 @ inp.S, S)
    cocc0 = np.ascontiguousarray(C0[:, ::-1][:, :nocc] * np.sqrt(np.maximum(e0[::-1][:nocc], 0.0)))
    J, K, Vraw = backend.ground_state_parts(dm0, cocc0, want_k)
    F = inp.Hcore + J + 0.5 * (Vraw + Vraw.T) - (0.5 * c_hf * K if want_k else 0.0)
    e, C = eigh(F, S)
    Co, Cv = np.ascontiguousarray(C[:, :nocc]), np.ascontiguousarray(C[:, nocc:])
    gap = e[nocc:, None] - e[None, :nocc]
    if gap.min() <= 1e-6:
        raise ValueError("polarizability: no gap between the occupied and the virtual orbitals")
    backend.response_prepare(dm0, cocc0)
    D = integrals.dipole(inp.shells)
    nv = Cv.shape[1]

    def dm_of(u):
        A = 2.0 * (Cv @ u.reshape(nv, nocc))
        M = A @ Co.T
        return M + M.T, (A, Co)

    def apply_a(u):
        dm1, fac = dm_of(u)
        J1, K1, V1 = backend.response_parts(dm1, want_k, fac)
        G = J1 + 0.5 * (V1 + V1.T) - (0.5 * c_hf * K1 if want_k else 0.0)
        return ((Cv.T @ G @ Co) / gap).reshape(-1)

    alpha, its, ress, dm1s = np.zeros((3, 3)), [], [], []
    for l in range(3):
        b = -((Cv.T @ D[l] @ Co) / gap).reshape(-1)
        u, n, r = _gmres(apply_a, b, tol, max_iter)
        dm1, _ = dm_of(u)
        alpha[:, l] = -np.einsum("kij,ji->k", D, dm1)
        its.append(n); ress.append(r); dm1s.append(dm1)
        if log:
            log(f"CPKS direction {'xyz'[l]}: {n} iterations, residual {r:.2e}")
    return {"alpha": alpha, "cpks_iterations": its, "residual": ress, "dipole_integrals": D, "dm1": dm1s}
