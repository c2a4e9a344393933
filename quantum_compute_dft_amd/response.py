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
    {"alpha", "cpks_iterations" (per direction), "residual" (per direction), "dipole_integrals", "dm1" (per direction)}."""
    f = functionals.resolve(functional if functional is not None else backend.functional)
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
