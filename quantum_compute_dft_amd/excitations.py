"""Singlet and triplet excitation energies of a closed-shell state, with the oscillator strengths of the singlets: TDDFT
(the full coupled problem) and its Tamm-Dancoff approximation, by a reduced-space iteration on top of a response backend.

Canonical orbitals Co, Cv and gaps D_ia = e_a - e_i come from one eigh(F, S) of the converged Fock matrix, as in
response.polarizability.  For a trial Z (nocc, nvirt) with A = Co, B = 2 Cv Z^T and D+- = A B^T +- B A^T

    (A+B) Z = D o Z + Co^T ( J[D+] + (V1 + V1^T)/2 [D+] - c_hf/2 K[D+] ) Cv
    (A-B) Z = D o Z - c_hf/2 Co^T K[D-] Cv                  (= D o Z without exact exchange: no K is requested)
    K[D]_mn = sum_ls (ml|ns) D_ls,    K[D+-] = M +- M^T,    M = K[A B^T]

J, M and V1 of all trials of an iteration come from ONE backend.excitation_parts call (scf.HipBackend on the device:
DFT_ComputeJKFactorizedResponse or DFT_ComputeJK, and DFT_FxcApply; response.HostResponse on the host).  (A+B) is the
operator response.polarizability applies: the sum over states 2 sum_n mu_n mu_n^T / w_n of the full spectrum equals
its alpha.  TDA solves A X = w X with A = ((A+B) + (A-B))/2 and X^T X = 1; TDDFT solves
(A-B)(A+B)(X+Y) = w^2 (X+Y) with (X+Y)^T (X-Y) = 1.  Transition dipole mu_n = sqrt(2) sum_ia (Co^T D_k Cv)_ia (X+Y)_ia,
oscillator strength f_n = 2/3 w_n |mu_n|^2.  With option quirks = 1 the operator is the response of the shipped
formulas, the SCF equations the loop actually solves -- the choice the polarizability made.

Triplets (triplet=True): the spin-flip perturbation dm_alpha, dm_beta = dm0/2 +- t D/2 induces no Coulomb potential, and
its XC response V1_T is the spin-flip kernel at zero polarisation (DFT_FxcPrepareSpin / DFT_FxcApplyKind, kind 1;
csrc/xc_spin_functionals.hpp):

    (A+B)_T Z = D o Z + Co^T ( (V1_T + V1_T^T)/2 [D+] - c_hf/2 K[D+] ) Cv       (no J is requested)
    (A-B)_T Z = (A-B) Z

A triplet carries no transition dipole from the singlet ground state: oscillator strengths are reported as 0.  The
spin-flip kernel is a second derivative of the ENERGY, so with quirks = 1 and vwn5_c or pbe_c in the functional (whose
shipped potentials are not the derivatives of their energies) the triplet operator would not belong to the ground
state the loop solved: refused, run with --quirks 0.  A reduced (A+B)_T that is not positive definite is a triplet
instability of the restricted reference (the classic test of a closed-shell solution) and is reported as one.
"""
import numpy as np
from scipy.linalg import eigh

from . import functionals, integrals

HARTREE_EV = 27.211386245988
NM_PER_HARTREE = 45.56335252907954        # h c / (1 Ha) in nm
_PBE_C = functionals.COMPONENTS.index("pbe_c")
_VWN5_C = functionals.COMPONENTS.index("vwn5_c")


class ResponseOperators:
    """(A+B) and (A-B) of a converged closed-shell state as maps on (nvec, nocc, nvirt) arrays: `apply`.  Fields: Co,
    Cv, gap (nocc, nvirt), dip = Co^T D_k Cv (3, nocc, nvirt), c_hf, builds (trial vectors applied so far)."""

    def __init__(self, inp, scf_result, backend, functional=None, triplet=False):
        f = functionals.resolve(functional if functional is not None else backend.functional)
        functionals.refuse_meta(f, "excitations (TDDFT / TDA)")
        quirks = bool(getattr(backend, "quirks", True))
        self.triplet = bool(triplet)
        if self.triplet and quirks and (f.weight_vector()[_VWN5_C] != 0.0 or f.weight_vector()[_PBE_C] != 0.0):
            raise ValueError("excitations: the triplet (spin-flip) kernel is the second derivative of the energy, but with quirks = 1 the "
                             "ground state solved the shipped vwn5_c / pbe_c potentials, which are not the derivatives of their energies; "
                             "run with --quirks 0")
        if quirks and f.weight_vector()[_PBE_C] != 0.0:
            raise ValueError("excitations: with quirks = 1 the shipped PBE correlation potential is not the derivative of "
                             "its energy and the response operator is not symmetric; run with --quirks 0")
        self.c_hf, self.want_k = f.c_hf, f.c_hf != 0.0
        S, nocc = inp.S, inp.nocc
        dm0 = np.ascontiguousarray(scf_result["dm"], dtype=np.float64)
        e0, C0 = eigh(S @ dm0 @ S, S)
        cocc0 = np.ascontiguousarray(C0[:, ::-1][:, :nocc] * np.sqrt(np.maximum(e0[::-1][:nocc], 0.0)))
        J, K, Vraw = backend.ground_state_parts(dm0, cocc0, self.want_k)
        F = inp.Hcore + J + 0.5 * (Vraw + Vraw.T) - (0.5 * self.c_hf * K if self.want_k else 0.0)
        e, C = eigh(F, S)
        self.Co, self.Cv = np.ascontiguousarray(C[:, :nocc]), np.ascontiguousarray(C[:, nocc:])
        self.gap = np.ascontiguousarray(e[None, nocc:] - e[:nocc, None])
        if self.gap.size == 0 or self.gap.min() <= 1e-6:
            raise ValueError("excitations: no gap between the occupied and the virtual orbitals")
        if self.triplet:
            backend.response_prepare(dm0, cocc0, kind="triplet")
        else:
            backend.response_prepare(dm0, cocc0)
        self.backend = backend
        self.dip = np.einsum("mi,kmn,na->kia", self.Co, integrals.dipole(inp.shells), self.Cv)
        self.builds = 0

    def apply(self, Z):
        """((A+B) Z_k, (A-B) Z_k) for Z (nvec, nocc, nvirt), through one excitation_parts call."""
        Z = np.asarray(Z, dtype=np.float64)
        Bs = np.ascontiguousarray(2.0 * np.einsum("na,kia->kni", self.Cv, Z))
        if self.triplet:
            _, M, V1 = self.backend.excitation_parts(self.Co, Bs, self.want_k, kind="triplet")
            G = 0.5 * (V1 + V1.transpose(0, 2, 1))                  # no Coulomb response to a spin flip
        else:
            J, M, V1 = self.backend.excitation_parts(self.Co, Bs, self.want_k)
            G = J + 0.5 * (V1 + V1.transpose(0, 2, 1))
        self.builds += Z.shape[0]
        dz = self.gap[None] * Z
        if not self.want_k:
            return dz + np.einsum("mi,kmn,na->kia", self.Co, G, self.Cv), dz
        Mt = M.transpose(0, 2, 1)
        plus = dz + np.einsum("mi,kmn,na->kia", self.Co, G - 0.5 * self.c_hf * (M + Mt), self.Cv)
        minus = dz - 0.5 * self.c_hf * np.einsum("mi,kmn,na->kia", self.Co, M - Mt, self.Cv)
        return plus, minus


class UksResponseOperators:
    """(A+B) and (A-B) of a converged unrestricted state (scf.run_uks) on the stacked space of the n_a nv_a + n_b nv_b
    spin-conserving occupied-virtual pairs, as maps on flat (nvec, size) arrays: `apply`.  UKS convention: D_s = C_os
    C_os^T with occupation 1, K enters with c_hf.  For Z = (Z_a, Z_b), A_s = C_os and B_s = C_vs Z_s^T,

        [(A+B) Z]_s = gap_s o Z_s + C_os^T ( J[D+_a + D+_b] + (V1_s + V1_s^T)/2 - c_hf (M_s + M_s^T) ) C_vs
        [(A-B) Z]_s = gap_s o Z_s - c_hf C_os^T (M_s - M_s^T) C_vs

    with J, M_s and V1_s of all trials from ONE backend.uks_excitation_parts call (DFT_FxcApplySpinPol for V1).  Fields:
    spins (per spin Co, Cv, gap), size, gap_flat, dip_flat (3, size), builds."""

    flat = True
    triplet = False

    def __init__(self, inp, uks_result, backend, functional=None):
        from . import response
        f, self.spins = response.uks_orbitals(inp, uks_result, backend, functional)
        self.c_hf, self.want_k = f.c_hf, f.c_hf != 0.0
        self.backend = backend
        self.shapes = [s["gap"].shape for s in self.spins]
        self.na = self.shapes[0][0] * self.shapes[0][1]
        self.size = self.na + self.shapes[1][0] * self.shapes[1][1]
        self.gap_flat = np.concatenate([s["gap"].reshape(-1) for s in self.spins])
        D = integrals.dipole(inp.shells)
        self.dip_flat = np.concatenate([np.einsum("mi,kmn,na->kia", s["Co"], D, s["Cv"]).reshape(3, -1) for s in self.spins], axis=1)
        self.builds = 0

    def split(self, Z):
        Z = np.asarray(Z, dtype=np.float64)
        return [Z[:, :self.na].reshape((Z.shape[0],) + self.shapes[0]), Z[:, self.na:].reshape((Z.shape[0],) + self.shapes[1])]

    def apply(self, Z):
        """((A+B) Z_k, (A-B) Z_k) for Z (nvec, size)."""
        Zs = self.split(Z)
        Bs = [np.ascontiguousarray(np.einsum("na,kia->kni", s["Cv"], z)) for s, z in zip(self.spins, Zs)]
        J, Ma, Mb, Va, Vb = self.backend.uks_excitation_parts(self.spins[0]["Co"], Bs[0], self.spins[1]["Co"], Bs[1], self.want_k)
        self.builds += Zs[0].shape[0]
        plus, minus = [], []
        for s, z, M, V in zip(self.spins, Zs, (Ma, Mb), (Va, Vb)):
            dz = s["gap"][None] * z
            G = J + 0.5 * (V + V.transpose(0, 2, 1))
            if self.want_k:
                Mt = M.transpose(0, 2, 1)
                G = G - self.c_hf * (M + Mt)
                minus.append((dz - self.c_hf * np.einsum("mi,kmn,na->kia", s["Co"], M - Mt, s["Cv"])).reshape(z.shape[0], -1))
            else:
                minus.append(dz.reshape(z.shape[0], -1))
            plus.append((dz + np.einsum("mi,kmn,na->kia", s["Co"], G, s["Cv"])).reshape(z.shape[0], -1))
        return np.concatenate(plus, axis=1), np.concatenate(minus, axis=1)


def _orthonormal_additions(basis, cands, drop=1e-8):
    """Rows of `cands`, orthogonalised against the rows of `basis` and each other (Gram-Schmidt, twice), normalised;
    a candidate that loses all but `drop` of its norm is left out."""
    out = []
    for c in cands:
        n0 = np.linalg.norm(c)
        if n0 == 0.0:
            continue
        c = c / n0
        for _ in range(2):
            c = c - basis.T @ (basis @ c)
            for o in out:
                c = c - o * (o @ c)
        n = np.linalg.norm(c)
        if n > drop:
            out.append(c / n)
    return np.array(out).reshape(len(out), basis.shape[1])


def _sqrt_spd(M, what, triplet=False, uks=False):
    w, U = np.linalg.eigh(M)
    if w[0] <= 0.0 and uks:
        raise ValueError(f"excitations: the reduced {what} is not positive definite (lowest eigenvalue {w[0]:.3e}): "
                         "the unrestricted reference is unstable")
    if w[0] <= 0.0 and triplet and what == "A+B":
        raise ValueError(f"excitations: the reduced triplet A+B is not positive definite (lowest eigenvalue {w[0]:.3e}): "
                         "triplet instability of the restricted reference")
    if w[0] <= 0.0:
        raise ValueError(f"excitations: the reduced {what} is not positive definite (lowest eigenvalue {w[0]:.3e}): "
                         "the reference state is unstable")
    return (U * np.sqrt(w)) @ U.T, (U / np.sqrt(w)) @ U.T


def solve(ops, nroots=5, tda=False, tol=1e-6, max_iter=60, max_space=None, log=None):
    """The lowest `nroots` roots of `ops` (a ResponseOperators, or a UksResponseOperators on its flat stacked space): the
    dict `excitations` returns."""
    uks = bool(getattr(ops, "flat", False))
    if uks:
        N, gap, dip = ops.size, ops.gap_flat, ops.dip_flat
        to_ops, from_flat = (lambda v: v), (lambda v: v)
    else:
        nocc, nvirt = ops.gap.shape
        N, gap, dip = nocc * nvirt, ops.gap.reshape(-1), ops.dip.reshape(3, nocc * nvirt)
        to_ops, from_flat = (lambda v: v.reshape(-1, nocc, nvirt)), (lambda v: v.reshape(-1, nocc, nvirt))
    if not 1 <= nroots <= N:
        raise ValueError(f"excitations: nroots = {nroots}, but there are {N} occupied-virtual pairs")
    max_space = min(N, max_space if max_space else max(8 * nroots, 40))
    max_space = max(max_space, min(N, 3 * nroots))           # room for a collapsed space (two vectors a root) to grow
    b = np.zeros((0, N))
    new = np.zeros((min(N, 2 * nroots), N))
    new[np.arange(new.shape[0]), np.argsort(gap, kind="stable")[:new.shape[0]]] = 1.0
    Pb, Qb = np.zeros((0, N)), np.zeros((0, N))
    builds0 = ops.builds
    triplet = bool(getattr(ops, "triplet", False))
    converged, it = False, 0
    for it in range(1, max_iter + 1):
        P, Q = ops.apply(to_ops(new))
        b = np.vstack([b, new]); Pb = np.vstack([Pb, P.reshape(-1, N)]); Qb = np.vstack([Qb, Q.reshape(-1, N)])
        Mp, Mm = b @ Pb.T, b @ Qb.T
        Mp, Mm = 0.5 * (Mp + Mp.T), 0.5 * (Mm + Mm.T)
        if tda:
            w, T = np.linalg.eigh(0.5 * (Mp + Mm))
            if w[0] <= 0.0 and uks:
                raise ValueError(f"excitations: the lowest Tamm-Dancoff root is {w[0]:.3e} Ha: the unrestricted reference is unstable")
            if w[0] <= 0.0 and triplet:
                raise ValueError(f"excitations: the lowest triplet Tamm-Dancoff root is {w[0]:.3e} Ha: triplet instability of the "
                                 "restricted reference")
            if w[0] <= 0.0:
                raise ValueError(f"excitations: the lowest Tamm-Dancoff root is {w[0]:.3e} Ha: the reference state is unstable")
            w, R, L = w[:nroots], T[:, :nroots], T[:, :nroots]                 # X+Y = X-Y = X
            res1 = R.T @ (0.5 * (Pb + Qb)) - w[:, None] * (R.T @ b)
            res2 = res1
        else:
            Sm, Smi = _sqrt_spd(Mm, "A-B", uks=uks)
            _sqrt_spd(Mp, "A+B", triplet, uks=uks)
            w2, T = np.linalg.eigh(Sm @ Mp @ Sm)
            w = np.sqrt(w2[:nroots])
            R = (Sm @ T[:, :nroots]) / np.sqrt(w)                               # X+Y in the basis
            L = (Smi @ T[:, :nroots]) * np.sqrt(w)                              # X-Y
            res1 = R.T @ Pb - w[:, None] * (L.T @ b)
            res2 = L.T @ Qb - w[:, None] * (R.T @ b)
        rn = np.maximum(np.linalg.norm(res1, axis=1), np.linalg.norm(res2, axis=1))
        if log:
            log(f"excitations iteration {it}: space {b.shape[0]}, lowest root {w[0]:.8f} Ha, largest residual {rn.max():.2e}")
        if np.all(rn <= tol):
            converged = True
            break
        if it == max_iter:
            break
        cands = []
        for n in np.nonzero(rn > tol)[0]:
            den = gap - w[n]
            den = np.where(np.abs(den) < 1e-4, 1e-4, den)
            cands.append(res1[n] / den)
            if not tda:
                cands.append(res2[n] / den)
        if b.shape[0] + len(cands) > max_space:
            # collapse onto the current roots: linear combinations of the basis, so the products follow without a build
            C = np.linalg.qr(np.hstack([R, L]) if not tda else R)[0]
            b, Pb, Qb = C.T @ b, C.T @ Pb, C.T @ Qb
        new = _orthonormal_additions(b, cands)
        if new.shape[0] == 0:
            break                                                               # nothing left to add: the space is exhausted
    xpy, xmy = R.T @ b, L.T @ b
    mu = (1.0 if uks else np.sqrt(2.0)) * np.einsum("kx,nx->nk", dip, xpy)       # UKS: both spins are in the vector, no sqrt(2)
    if triplet:
        mu = np.zeros_like(mu)                       # spin-forbidden from the singlet ground state
    return {"energies": w, "oscillator_strengths": (2.0 / 3.0) * w * np.einsum("nk,nk->n", mu, mu),
            "transition_dipoles": mu, "xpy": from_flat(xpy), "xmy": from_flat(xmy),
            "residuals": rn, "iterations": it, "sigma_builds": ops.builds - builds0, "converged": converged,
            "method": ("tda" if tda else "tddft") + ("-uks" if uks else "-triplet" if triplet else ""),
            "multiplicity": None if uks else 3 if triplet else 1}


def excitations(inp, scf_result, backend, functional=None, nroots=5, tda=False, tol=1e-6, max_iter=60, max_space=None, log=None,
                triplet=False):
    """The lowest `nroots` singlet (triplet=True: triplet) excitations of the converged closed-shell state `scf_result` (scf.run_scf) by a
    Davidson-type iteration on one orthonormal trial basis b: every iteration applies (A+B) and (A-B) to the new vectors
    through one backend.excitation_parts call, solves the reduced problem M-^(1/2) M+ M-^(1/2) T = w^2 T (TDA: the
    symmetric b^T A b), and extends b by the residuals (A+B)(X+Y) - w (X-Y) and (A-B)(X-Y) - w (X+Y) divided by
    D - w, starting from unit vectors at the smallest gaps; a root is converged when both residual 2-norms are <= tol.
    The space is collapsed onto the current roots when it would exceed `max_space`.

    Returns {"energies" (Ha, ascending), "oscillator_strengths", "transition_dipoles" (nroots, 3), "xpy", "xmy"
    (nroots, nocc, nvirt; equal for TDA), "residuals", "iterations", "sigma_builds", "converged", "method" ("tddft", "tda",
    "tddft-triplet", "tda-triplet"), "multiplicity" (1 or 3)}; a triplet's oscillator strengths and transition dipoles
    are zero.  ValueError: nroots above nocc nvirt, no gap, a reduced A+B or A-B that is not positive definite (an
    unstable reference; for triplets: a triplet instability of the restricted reference), quirks = 1 with PBE
    correlation (a non-symmetric operator; use quirks 0), or triplets at quirks = 1 with vwn5_c or pbe_c.

    A scf.run_uks result (uks = True): the spin-conserving excitations of the unrestricted reference on the stacked space of
    both spins' pairs (UksResponseOperators); "method" is "tddft-uks" / "tda-uks", "multiplicity" None, xpy / xmy are flat
    (nroots, n_a nv_a + n_b nv_b), alpha pairs first; transition dipole sum_s sum_ia (C_os^T D_k C_vs)_ia (X+Y)_s,ia (no
    sqrt(2): the restricted singlet vector (Z, Z)/sqrt(2) recovers the closed-shell formula), f = 2/3 w |mu|^2.  A reduced
    A+B or A-B that is not positive definite: "the unrestricted reference is unstable"; triplet=True is refused."""
    if scf_result.get("uks"):
        if triplet:
            raise ValueError("excitations: triplet=True asks for the spin-flip kernel of a closed-shell reference; from an unrestricted "
                             "reference only the spin-conserving excitations are solved (spin-flip excitations are out of scope)")
        return solve(UksResponseOperators(inp, scf_result, backend, functional), nroots, tda, tol, max_iter, max_space, log)
    return solve(ResponseOperators(inp, scf_result, backend, functional, triplet=triplet), nroots, tda, tol, max_iter, max_space, log)
