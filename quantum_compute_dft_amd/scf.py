"""The SCF loop of the reference driver (dft.py:181-266) with the device work behind a backend.

Loop contract kept exactly: core guess `eigh(Hcore, S)`; per cycle J (compute_coulomb), XC
(compute_xc), `Vxc = (V + V^T)/2` (dft.py:212), for B3LYP K and `F = H + J + Vxc - 0.5*0.2*K`
(dft.py:217-221), DIIS on (S, dm, F), `eigh(F, S)`, energies from the NEW density with J/K/Exc of
the old one (dft.py:230-236), convergence |dE| < 1e-8 and ||d dm||_F < 1e-6 (dft.py:243),
200 cycles.  Differences: J and K come from ONE pass over the ERI (DFT_ComputeJK), AO values
are evaluated on the device.  The loop stands four times, three closed-shell forms that `run_scf` chooses between
by two flags of the backend, and the open-shell one:

* fused (`_run_scf_fused`, `backend.fused`: `HipBackend(fused_tail=True)`, or by default where the rotation solver
  is in use and scf_tail.supported(nao, nocc)): the end of the cycle -- Fock assembly, DIIS, rotation, density,
  energy traces -- is a handful of launches of libdft.so behind the cycle's J / K / Vxc (scf_tail.py), and the host
  waits once per cycle for the energy and convergence scalars;
* device-resident (`_run_scf_device`, `backend.device_resident`: from `device_from` = 200 functions, or
  `HipBackend(device_resident=True)`, where the fused form is not chosen): dm, cocc, J, K, Vxc, F, the DIIS history,
  the eigenproblem and dm = 2 C_occ C_occ^T are torch tensors in HBM; per cycle one 4-double download (E_one,
  E_coul, E_ex, |d dm|) besides the Exc the ABI returns.  Anthracene B3LYP/def2-SVP (n = 246): 4.3 against 6.0 ms
  per cycle for the host form;
* host (`_run_scf`, neither flag; also what a backend without them gets, such as the oracle backend of the tests):
  per cycle ONE pinned upload [dm | cocc] and ONE pinned download [J | K | Vxc] cross PCIe, everything else is numpy
  (n = 114: 0.5 ms of dsyevd on one LAPACK thread against 1.9 ms for hipSOLVER);
* open-shell (`run_uks`): the host form for two spin densities, eigh(F_s, S) every cycle.

What they share is written once: `_CycleLedger` (energy sum, dE, times, log line, `res`, the thresholds, the profile),
`_aufbau_check` (the converged state of a rotation run against the full solver), `_rotation_tol` (how accurately a
cycle's rotation is solved) and `FockDiagonaliser` (the full solver: S^-1/2, hipSOLVER or one host LAPACK thread).

With world > 1 rank 0 is authoritative: it alone runs DIIS + eigh and broadcasts [dm | cocc | scalars]
(grid_shard.ReplicaSync), so replicas cannot drift apart and every rank leaves the loop in the same cycle
(the stop decision is made from the broadcast scalars).
"""
import os
import time

import numpy as np
from scipy.linalg import eigh

from . import functionals

# the full solver goes to hipSOLVER from this many basis functions; below it one host LAPACK thread is faster, for the solve
# and for everything else left on the host (dsyevd at n = 114: 0.67 ms on one thread, 0.87 on 16), so run_scf pins the pools
_HIPSOLVER_FROM = 400
_FIXED_POINT_FLOOR = 1e-10     # the residual below which no rotation's fixed point is ever asked to go


def _host(a):
    """A numpy array or a tensor as a numpy array."""
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _rotation_tol(last_ddm, floor=_FIXED_POINT_FLOOR):
    """The residual at which the fixed point of a cycle's occupied rotation may stop: a cycle that still moves the
    density by `last_ddm` is solved a thousand times finer than that and no finer, never below `floor` and never
    looser than the cap below (inexact diagonalisation; the orbitals stay exactly orthonormal, i.e. a valid trial
    density, either way).  No previous cycle (None): `floor`."""
    return floor if last_ddm is None else min(max(floor, 1e-3 * float(last_ddm)), 1e-5)


class CDIIS:
    """Pulay DIIS on the commutator SDF - FDS (PySCF scf.diis.CDIIS as used at dft.py:184,225).

    The history is a ring of `space` (F, e) pairs in two flat (space, n^2) arrays; per cycle the Gram matrix of the
    error vectors gets ONE new row (a GEMV) and the extrapolation is one GEMV over the stored Fock matrices (the
    textbook form recomputes 36 dot products and sums 8 scaled matrices: 0.12 against 0.07 ms of a Benzene cycle).
    The commutator is formed through the thin factor when the caller passes cocc with dm = cocc cocc^T: three
    n^2 n_occ products instead of two n^3 ones.  With `device` arrays and products live on the GPU (rocBLAS through
    torch; n = 494 costs 2.3 ms per cycle on 16 host cores) and only the (space+1)^2 system is solved on the host."""

    def __init__(self, space=8, device=None):
        self.space, self.dev = space, device
        self._slots = None
        if device is not None:
            import torch
            self.torch = torch

    def update(self, S, dm, F, keep_on_device=False, cocc=None):
        """Extrapolated Fock matrix.  Device mode accepts numpy or device tensors; `keep_on_device` returns
        the device tensor (device-resident loop) instead of a numpy copy."""
        dev = self.dev is not None
        if dev:
            t = self.torch
            f64 = t.float64
            conv = lambda a: a if t.is_tensor(a) else t.as_tensor(a, dtype=f64, device=self.dev)
        n2 = F.shape[0] * F.shape[1]
        if self._slots is None:
            if dev:
                self._Fb, self._Eb = (t.zeros((self.space, n2), dtype=f64, device=self.dev) for _ in range(2))
                self._S = conv(S)
            else:
                self._Fb, self._Eb = np.zeros((self.space, n2)), np.zeros((self.space, n2))
                self._S = S
            self._Gb, self._slots = np.zeros((self.space, self.space)), []
        slot = self._slots.pop(0) if len(self._slots) == self.space else len(self._slots)   # the oldest pair is overwritten
        Fk = conv(F) if dev else F
        if cocc is not None:
            c = conv(cocc) if dev else cocc
            sdf = (self._S @ c) @ (c.T @ Fk)
        else:
            sdf = self._S @ (conv(dm) if dev else dm) @ Fk
        self._Fb[slot] = Fk.reshape(-1)
        if dev:
            t.sub(sdf.T, sdf, out=self._Eb[slot].view(F.shape))
        else:
            np.subtract(sdf.T, sdf, out=self._Eb[slot].reshape(F.shape))
        self._slots.append(slot)
        idx = np.array(self._slots)
        row = self._Eb @ self._Eb[slot]          # against every slot; unused ones are zero and never read
        row = row.cpu().numpy() if dev else row
        self._Gb[slot, idx] = self._Gb[idx, slot] = row[idx]
        n = len(idx)
        if n < 2:
            return (Fk if keep_on_device else F)
        B = np.zeros((n + 1, n + 1)); B[0, 1:] = B[1:, 0] = 1.0
        B[1:, 1:] = self._Gb[np.ix_(idx, idx)]
        rhs = np.zeros(n + 1); rhs[0] = 1.0
        try:
            cf = np.linalg.solve(B, rhs)[1:]
        except np.linalg.LinAlgError:
            cf = np.linalg.lstsq(B, rhs, rcond=None)[0][1:]
        m = int(idx.max()) + 1
        cs = np.zeros(m); cs[idx] = cf
        if not dev:
            return (cs @ self._Fb[:m]).reshape(F.shape)
        out = (t.as_tensor(cs, device=self.dev) @ self._Fb[:m]).view(F.shape)
        return out if keep_on_device else out.cpu().numpy()


class FockDiagonaliser:
    """F C = S C e, the one dense eigenproblem of an SCF cycle (dft.py:181,227 `eigh(F, S)` on the host).
    F is orthogonalised with X = U s^-1/2 (once per S).  Small matrices stay on the host: LAPACK dsyevd
    on ONE thread (measured on the MI355X box, tools/eigh_threads.py: n = 114 0.67 ms on one thread
    against 1.0 ms for scipy's generalised driver on 16; n = 246 3.2 against 4.9 ms).  From
    `device_from` basis functions on the problem goes to the GPU: hipSOLVER through
    torch.linalg.eigh, the only library call on the device path (n = 494: 11.4 ms against 16.5 ms on
    16 host cores, n = 1150: 27 against 84 ms, tools/eigh_time.py).

    Three ways in.  `__call__`: numpy in, numpy out, on the device from `device_from` functions (the host loop).
    `solve_host`: numpy in, numpy out, LAPACK whatever the size.  `solve_device`: a device tensor in, eigenvectors on
    the device out (the rotation solver's full solves and the two device loops), hipSOLVER from _HIPSOLVER_FROM
    functions and LAPACK below, where a full solve crosses PCIe with 2 n^2 doubles (n = 246: 2.5 against ~6 ms).  It
    needs X in HBM (`device_from=0` puts it there at any size) unless it is asked for `products="host"`."""

    def __init__(self, S, device=None, device_from=_HIPSOLVER_FROM):
        self.S, self.n = S, S.shape[0]
        self.on_device = device is not None and self.n >= device_from
        s, U = np.linalg.eigh(S)
        self.Xh = U / np.sqrt(s)                                  # S^-1/2 (columns)
        if self.on_device:
            import torch
            self.torch = torch
            self.X = torch.as_tensor(self.Xh, dtype=torch.float64, device=device)

    def __call__(self, F):
        if not self.on_device:
            return self.solve_host(F)
        e, C = self._hipsolver(self.torch.as_tensor(F, dtype=self.torch.float64, device=self.X.device))
        return e.cpu().numpy(), C.cpu().numpy()

    def solve_host(self, F):
        e, Cp = eigh(self.Xh.T @ F @ self.Xh, driver="evd")       # run_scf pins the BLAS pool to one thread at this size
        return e, self.Xh @ Cp

    def _hipsolver(self, F):
        e, Cp = self.torch.linalg.eigh(self.X.T @ F @ self.X)
        return e, self.X @ Cp

    def solve_device(self, F, products="device"):
        """(energies, eigenvectors as a tensor on F's device) of a device tensor F.  The energies stay where the
        driver left them: a tensor from hipSOLVER, a numpy array from LAPACK.  `products`: where X^T F X and X C' are
        formed on the LAPACK path -- "device" (F' goes down, C' comes up) or "host" (F goes down, C comes up).  The two
        round differently, so each loop keeps the placement it has always had."""
        if self.n >= _HIPSOLVER_FROM:
            return self._hipsolver(F)
        import torch
        if products == "host":
            e, C = self.solve_host(F.cpu().numpy())
            return e, torch.from_numpy(np.ascontiguousarray(C)).to(F.device)
        e, Cp = eigh((self.X.T @ F @ self.X).cpu().numpy(), driver="evd")
        return e, self.X @ torch.as_tensor(Cp, device=F.device)


class OccupiedRotation:
    """The occupied orbitals of F C = S C e WITHOUT a dense eigensolve per cycle.

    The SCF loop only consumes the occupied subspace (dm = 2 C_occ C_occ^T, dft.py:182,228), and between two
    cycles the Fock matrix moves little.  A full S-orthonormal basis U = [U_o | U_v] is kept from the last full
    diagonalisation; each cycle forms A = U^T F U (two n^3 GEMMs, the only n^3 work) and finds the rotation that
    decouples the two blocks: with K (n_virt x n_occ) solving the Riccati equation

        A_vo + A_vv K - K A_oo - K A_ov K = 0

    the columns of U_o + U_v K span the new occupied space exactly.  K is found by the diagonally preconditioned
    fixed point K <- K - R / (a_v - a_o) -- denominators only ACROSS the gap, so near-degenerate orbitals inside
    either block (Benzene's e pairs, the dense virtual spectrum of a TZVP basis) never enter, which is what
    defeated the refinement and filtering attempts of round 1 -- at O(n_virt^2 n_occ) per step.  The orthogonal
    completion  U_o' = (U_o + U_v K)(1 + K^T K)^-1/2,  U_v' = (U_v - U_o K^T)(1 + K K^T)^-1/2  needs only the
    n_occ x n_occ eigen-decomposition of K^T K; the occupied block is then made canonical (an n_occ x n_occ eigh), so
    its side of the next cycle's denominators is exact.  Falls back to the full solver (which also does the first
    cycle) when the first-order rotation exceeds 0.5, the fixed point has not reached `tol` in `max_inner` steps or
    grows, or the aufbau order is in doubt (highest occupied level within 1e-3 Ha of the lowest virtual diagonal).
    The virtual block is never diagonalised, so that test is a necessary one only: run_scf therefore checks the
    CONVERGED state once against eigh(F, S) (which also supplies the full spectrum it reports) and resumes with the
    full solver and a fresh DIIS history if the occupied space it followed is another (_aufbau_check).

    Where it pays (profiles/r02_eigensolver.txt): solved to `tol` the fixed point needs 15-20 steps in the middle of
    an SCF run (the Fock matrix still moves by 1e-2) and 4-6 at its end; stopped where _rotation_tol puts it for the
    last density change (`accuracy`) it needs 3-5 per cycle.  Per SCF
    cycle of the real molecules: n = 494 (device) 12.5 against 23.4 ms, n = 246 (device) 4.3 against 6.9 ms, n = 114
    (host, plain numpy: ~25 small BLAS/LAPACK calls) 0.86 against 1.23 ms; below ~80 functions dsyevd itself is
    cheaper than those calls -- `eigensolver="auto"` uses it from 80 functions.  Same converged energies (to the
    SCF's own thresholds) and cycle counts within one of the exact loop (tests/test_scf_cpu.py)."""

    def __init__(self, S, nocc, device=None, tol=_FIXED_POINT_FLOOR, max_inner=60, full=None):
        import torch
        self.t, self.no, self.tol, self.max_inner = torch, int(nocc), tol, max_inner
        self.dev = torch.device(device) if device is not None else torch.device("cpu")
        self.host = self.dev.type == "cpu"      # host form: plain numpy (a torch-CPU operation costs 3-5 us, ~70 of them per cycle)
        # the full solver: the backend's FockDiagonaliser (`full`) where there is one, so that S is decomposed once
        self.full = full if full is not None else FockDiagonaliser(S, None if self.host else self.dev, device_from=0)
        self.U = None
        self.stats = {"exact": 0, "rotated": 0, "inner_steps": 0}

    def reset(self):
        """Forget the followed subspace and the counters: the next call is a full solve (a second SCF on the same backend)."""
        self.U = None
        self.stats = {"exact": 0, "rotated": 0, "inner_steps": 0}

    def _exact(self, F):
        if self.host:
            e, self.U = self.full.solve_host(F)
        else:
            e, self.U = self.full.solve_device(F)
            e = self.t.as_tensor(e, device=self.dev)
        self.stats["exact"] += 1
        return e, self.U[:, :self.no]

    def occupied(self, F, accuracy=None):
        """(orbital energies, C_occ (n, nocc)) for the Fock matrix F (numpy array or tensor on self.dev); the
        energies are exact for the occupied block, diagonal estimates for the virtual one after a rotation.
        `accuracy`: the density change of the SCF loop's last cycle, which sets the residual at which the fixed point
        may stop in THIS call (_rotation_tol, never below self.tol); None: solve to self.tol."""
        t, no = self.t, self.no
        tol = _rotation_tol(accuracy, self.tol)
        if self.host:
            return self._occupied_host(np.asarray(F), tol)
        F = F if t.is_tensor(F) else t.as_tensor(F, dtype=t.float64, device=self.dev)
        if self.U is None or no == 0 or no == F.shape[0]:
            return self._exact(F)
        U = self.U
        A = U.T @ (F @ U)
        d = t.diagonal(A)
        do, dv = d[:no], d[no:]
        Aoo, Aov, Avo, Avv = A[:no, :no], A[:no, no:], A[no:, :no], A[no:, no:]
        rden = 1.0 / (dv[:, None] - do[None, :])
        K = -(Avo * rden)
        if not float(K.abs().max()) <= 0.5:
            return self._exact(F)
        # every operation below is a kernel launch (~8 us each at these sizes, the whole cost of the device form):
        # fused multiply-adds (addmm / addcmul), a convergence test -- a host sync -- every third step only, and
        # ONE download / ONE upload for the two n_occ x n_occ eigen-decompositions of the completion
        prev, ok = float("inf"), False
        for it in range(self.max_inner):
            R = t.addmm(Avo, Avv, K).addmm_(K, t.addmm(Aoo, Aov, K), alpha=-1.0)   # Avo + Avv K - K (Aoo + Aov K)
            self.stats["inner_steps"] += 1
            if it % 3 == 0:
                r = float(R.abs().max())
                if r < tol:
                    ok = True
                    break
                if not (r < 4.0 * prev):    # diverging (or NaN)
                    break
                prev = min(prev, r)
            K = t.addcmul(K, R, rden, value=-1.0)
        if not ok:
            return self._exact(F)
        Kt = K.T
        Fo = t.addmm(t.addmm(Aoo, Aov, K), Kt, t.addmm(Avo, Avv, K))          # Y^T F Y in the U basis, Y = Uo + Uv K
        pack = t.cat([(Kt @ K).reshape(-1), Fo.reshape(-1), dv.min().reshape(1)]).cpu().numpy()
        M, Foh, dvmin = pack[:no * no].reshape(no, no), pack[no * no:2 * no * no].reshape(no, no), pack[-1]
        lam, V = np.linalg.eigh(M)
        lam = np.maximum(lam, 0.0)
        isq = 1.0 / np.sqrt(1.0 + lam)
        Mo = (V * isq) @ V.T                                                  # (1 + K^T K)^-1/2
        G = (V * np.where(lam > 1e-12, (isq - 1.0) / np.maximum(lam, 1e-300), -0.5)) @ V.T   # (1 + K K^T)^-1/2 = 1 + K G K^T
        Aoo2 = Mo @ Foh @ Mo                                                  # occupied block in the rotated basis
        eo, Vo = np.linalg.eigh(0.5 * (Aoo2 + Aoo2.T))
        if eo[-1] > dvmin - 1e-3:                                             # aufbau order in doubt
            return self._exact(F)
        up = t.as_tensor(np.concatenate([G.ravel(), (Mo @ Vo).ravel(), eo]), device=self.dev)
        G_d, c_d, eo_d = up[:no * no].view(no, no), up[no * no:2 * no * no].view(no, no), up[2 * no * no:]
        Uo, Uv = U[:, :no], U[:, no:]
        Un = t.empty_like(U)
        t.mm(t.addmm(Uo, Uv, K), c_d, out=Un[:, :no])                         # canonical occupied orbitals (Uo + Uv K) Mo Vo
        T = t.addmm(Uv, Uo, Kt, alpha=-1.0)
        Un[:, no:] = t.addmm(T, (T @ K) @ G_d, Kt)
        self.U = Un
        self.stats["rotated"] += 1
        return t.cat([eo_d, dv]), Un[:, :no]

    def _occupied_host(self, F, tol):
        """The same algorithm in numpy (returns numpy arrays): at n = 114 one cycle is ~25 small BLAS/LAPACK calls."""
        no = self.no
        if self.U is None or no == 0 or no == F.shape[0]:
            return self._exact(F)
        U = self.U
        A = U.T @ (F @ U)
        d = np.diagonal(A)
        do, dv = d[:no], d[no:]
        Aoo, Aov, Avo, Avv = A[:no, :no], A[:no, no:], A[no:, :no], A[no:, no:]
        rden = 1.0 / (dv[:, None] - do[None, :])
        K = -Avo * rden
        if not (np.abs(K).max() <= 0.5):
            return self._exact(F)
        prev, ok = float("inf"), False
        for it in range(self.max_inner):
            R = Avo + Avv @ K - K @ (Aoo + Aov @ K)
            self.stats["inner_steps"] += 1
            r = np.abs(R).max()
            if r < tol:
                ok = True
                break
            if not (r < 4.0 * prev):        # diverging (or NaN)
                break
            prev = min(prev, r)
            K = K - R * rden
        if not ok:
            return self._exact(F)
        lam, V = np.linalg.eigh(K.T @ K)
        lam = np.maximum(lam, 0.0)
        isq = 1.0 / np.sqrt(1.0 + lam)
        Mo = (V * isq) @ V.T                                                  # (1 + K^T K)^-1/2
        g = np.where(lam > 1e-12, (isq - 1.0) / np.maximum(lam, 1e-300), -0.5)
        G = (V * g) @ V.T                                                     # (1 + K K^T)^-1/2 = 1 + K G K^T
        Uo, Uv = U[:, :no], U[:, no:]
        T = Uv - Uo @ K.T
        Uv2 = T + ((T @ K) @ G) @ K.T
        Uo2 = (Uo + Uv @ K) @ Mo
        AvvK = Avv @ K
        Aoo2 = Mo @ (Aoo + Aov @ K + K.T @ Avo + K.T @ AvvK) @ Mo             # occupied block in the rotated basis
        eo, Vo = np.linalg.eigh(0.5 * (Aoo2 + Aoo2.T))
        if eo[-1] > dv.min() - 1e-3:                                          # aufbau order in doubt
            return self._exact(F)
        Un = np.empty_like(U)
        Un[:, :no] = Uo2 @ Vo                                                 # canonical occupied orbitals
        Un[:, no:] = Uv2
        self.U = Un
        self.stats["rotated"] += 1
        return np.concatenate([eo, dv]), Un[:, :no]


class HipBackend:
    """Device side of the loop: libdft.so through DFTSolverWrapper, torch tensors as buffers.

    One process per GPU.  With world > 1 (torch.distributed initialised by the caller) this rank
    keeps grid block shard_bounds(ngrid, world, rank) -- AO values are only ever evaluated for it --
    and Cholesky-vector slice vector_bounds(naux, world, rank) resident; a cycle is the local XC
    sweep + local J/K followed by ONE all-reduce of [Vxc | J | K | Exc] (grid_shard.ShardedFock).  A
    dense ERI is sharded by ROWS (ij): rank r contracts rows eri_row_bounds(nao^2, world, r) into its
    rows of J (and, through the (i,k) view, its partial K); the all-reduce assembles them."""

    def __init__(self, inp, functional, lib_path=None, quirks=True, rank=0, world=1, device=None, group=None,
                 device_resident=None, device_from=200, eigensolver="auto", ao_mode="resident", ao_chunk=0, xc_occ=None,
                 fused_tail=None, dm_factor=False):
        import torch
        from .build import library_path
        from .grid_shard import ReplicaSync, ShardedFock, eri_row_bounds, shard_bounds, vector_bounds
        from .solver import DFTSolverWrapper
        assert torch.cuda.is_available(), "the SCF driver needs a GPU (there is no CPU fallback)"
        self.torch, self.dev = torch, torch.device(device if device is not None else "cuda")
        if self.dev.index is not None:
            torch.cuda.set_device(self.dev)
        self.functional = functional.upper()
        self.solver = DFTSolverWrapper(lib_path or library_path(), functional)   # any name or expression of functionals.resolve()
        self.solver.set_option("quirks", 1 if quirks else 0)
        self.quirks = bool(quirks)
        # A meta-GGA (functionals.Functional.needs_tau) sweeps through DFT_ComputeXCMeta: synchronous, the density matrix itself,
        # resident planes, one rank -- the host loop.  What cannot serve it is refused here, by name, not switched off silently.
        self.meta = bool(self.solver.functional.needs_tau)
        if self.meta:
            for bad, why in ((world > 1, "more than one rank (the grid is not sharded for DFT_ComputeXCMeta)"),
                             (ao_mode == "direct", "--ao direct (tau is formed from resident gradient planes)"),
                             (bool(dm_factor), "dm_factor (the sweep takes the density matrix itself)"),
                             (xc_occ is not None and bool(xc_occ), "xc_occ (there is no occupied-orbital form of tau)"),
                             (bool(fused_tail), "the fused tail (it pre-queues the asynchronous sweep entries, which have no meta form)"),
                             (bool(device_resident), "the device-resident loop (it queues the asynchronous sweep entries, which have no meta form)")):
                if bad:
                    raise ValueError(f"{self.functional} is a meta-GGA: it runs on the host loop with resident AO planes, not with {why}")
            xc_occ, fused_tail, device_resident = False, False, False
        elif xc_occ is None:
            xc_occ = True
        self._lib_path, self._grad2e = lib_path, None       # the device two-electron gradient: opened by the first grad2e()
        t0 = time.time()
        self.rank, self.world = rank, world
        nao = inp.shells.nao
        lo, hi = shard_bounds(inp.grids.size, world, rank)
        ngrid = hi - lo
        self.nao, self.ngrid = nao, ngrid
        f64 = torch.float64
        n1 = max(ngrid, 1)   # an empty block keeps one dummy row so every pointer stays valid; it is never swept
        d_coords = torch.zeros((n1, 3), dtype=f64, device=self.dev)
        self.d_w = torch.zeros(n1, dtype=f64, device=self.dev)
        d_coords[:ngrid] = torch.as_tensor(inp.grids.coords[lo:hi], dtype=f64)
        self.d_w[:ngrid] = torch.as_tensor(inp.grids.weights[lo:hi], dtype=f64)
        # "resident" (the reference's layout, dft.py:155,172): AO values / gradients of the whole grid block stay in
        # HBM for the run (8 ngrid nao (1 or 4) bytes; 53 GB for BASELINE config 5).  "direct": only the grid and the
        # shell table stay; every cycle re-evaluates them chunk by chunk inside DFT_ComputeXCDirect.
        if ao_mode not in ("resident", "direct"):
            raise ValueError(f"ao_mode {ao_mode!r}: expected 'resident' or 'direct'")
        self.ao_mode, self.ao_chunk, self.shells, self.d_coords = ao_mode, int(ao_chunk), inp.shells, d_coords
        # what the grid response of the nuclear gradient reads (xc_grid_response): the atoms and the grid's own bookkeeping
        self._atoms, self._grids = (getattr(inp, "symbols", None), getattr(inp, "atom_xyz", None)), inp.grids
        # the sweep's density step through the occupied orbitals (DFT_ComputeXCOcc: the loop holds cocc with
        # dm = cocc cocc^T in every cycle, dft.py:181-182); False = the reference's call with the full matrix
        self.xc_occ = bool(xc_occ)
        # the reference's call, with the library factorising dm on the device and sweeping through the factor where that
        # pays (option "dm_factor", DFT_FactorDensity): what an unmodified reference driver gets from QCDFT_DM_FACTOR=1
        self.dm_factor = bool(dm_factor) and not self.xc_occ
        if self.dm_factor:
            self.solver.set_option("dm_factor", 1)
        self.d_ao = self.d_gr = None
        if ao_mode == "resident":
            self.d_ao = torch.zeros((n1, nao), dtype=f64, device=self.dev)
            self.d_gr = torch.zeros((3, n1, nao), dtype=f64, device=self.dev) if self.solver.needs_gradient else None
            if ngrid:
                self.solver.eval_ao(inp.shells, d_coords, ngrid, self.d_ao, self.d_gr)  # grid.py:30,38 on the device
        else:
            self._d_exc = torch.zeros(1, dtype=f64, device=self.dev)
        self.d_eri = self.d_chol = self.d_cocc = None
        self.eri_rows = (0, nao * nao)
        if inp.eri is not None:
            # dft.py:166 uploads the whole (nao^2, nao^2) matrix; with world > 1 each rank keeps its ROW block
            rlo, rhi = eri_row_bounds(nao, world, rank)
            self.eri_rows = (rlo, rhi)
            if rhi > rlo:
                self.d_eri = self._dev(inp.eri.reshape(nao * nao, nao * nao)[rlo:rhi])
            # (ij|kl) = (kl|ij): when the matrix in HBM really is symmetric (checked here, once) and only J is wanted, the Coulomb
            # pass streams its upper triangle alone -- half the bytes of dft_solver.cu:550-555's GEMV, which is all a J build costs
            # ... and when it is symmetric in each index pair too, (ij|kl) = (ji|kl) = (ij|lk), the unique eighth alone (k_j_sym8;
            # the loop's dm = cocc cocc^T is symmetric bit for bit)
            if world == 1 and self.solver.c_hf == 0.0 and self.d_eri is not None and bool(torch.equal(self.d_eri, self.d_eri.T)):
                e4 = self.d_eri.view(nao, nao, nao * nao)
                eightfold = bool(torch.equal(e4, e4.transpose(0, 1)))
                self.solver.set_option("eri_symmetric", 2 if eightfold else 1)
                del e4
        else:  # factorised J/K (DFT_ComputeJKFactorized): Cholesky vectors stay resident instead of the ERI
            if getattr(inp, "chol_range", None) is not None:      # inputs.build(world > 1) handed over this rank's slice only
                self.d_chol = torch.as_tensor(inp.chol, dtype=f64, device=self.dev)
            else:
                plo, phi = vector_bounds(inp.chol.shape[0], world, rank)
                self.d_chol = torch.as_tensor(inp.chol[plo:phi], dtype=f64, device=self.dev)
        self.nocc = inp.nocc
        # flat device buffers: [dm | cocc] arrives in one upload, [J | K | Vxc] leaves in one download
        n2 = nao * nao
        self._up = torch.zeros(n2 + nao * inp.nocc, dtype=f64, device=self.dev)
        self.d_dm, self.d_cocc = self._up[:n2].view(nao, nao), self._up[n2:].view(nao, inp.nocc)
        self._down = torch.zeros(3 * n2, dtype=f64, device=self.dev)
        self.d_J, self.d_K, self.d_v = (self._down[k * n2:(k + 1) * n2].view(nao, nao) for k in range(3))
        self._pin_up = torch.empty(self._up.shape, dtype=f64).pin_memory()
        self._pin_down = torch.empty(self._down.shape, dtype=f64).pin_memory()
        self.device_resident = (nao >= device_from) if device_resident is None else bool(device_resident)
        self.diis_device = self.dev if (nao >= 200 or self.device_resident) else None   # DIIS products on the GPU once they cost more than the hops
        self.replica_sync = ReplicaSync(self.dev, group) if world > 1 else None
        if world > 1:
            self._sharded = ShardedFock(nao, self._local_sweep, self._local_jk, self.dev, group)
        # "exact": eigh(F, S) every cycle, the reference's loop (dft.py:227); "rotate": occupied-subspace rotation with
        # the full solver as first cycle and fallback; "auto": rotate where it pays -- from 80 basis functions (per
        # cycle of the real molecules: n = 24 0.23 against 0.21 ms and n = 36 0.37 against 0.34, so not there;
        # n = 114 0.86 against 1.23; n = 246 4.3 against 6.9; n = 494 12.5 against 23.4)
        # the full solver (FockDiagonaliser keeps its threshold whatever the loop form); the device loop needs X in HBM always
        self.eigh = FockDiagonaliser(inp.S, self.dev, device_from=0 if self.device_resident else _HIPSOLVER_FROM)
        self.occ_solver = None
        if eigensolver not in ("auto", "rotate", "exact"):
            raise ValueError(f"eigensolver {eigensolver!r}: expected 'auto', 'rotate' or 'exact'")
        if eigensolver == "rotate" or (eigensolver == "auto" and nao >= 80):
            self.occ_solver = OccupiedRotation(inp.S, inp.nocc, self.dev if self.device_resident else None, full=self.eigh)
        # The end of the cycle (Fock assembly, DIIS, rotation, density, energy traces) as six launches of libdft.so behind the
        # cycle's J / K / Vxc (scf_tail.py, csrc/scf_tail.hip) where the rotation solver is in use and the sizes fit its
        # single-workgroup rotation kernel: Benzene/def2-SVP 0.44 ms of host work per cycle -> ~0.1 ms of device work.
        # None = auto (one rank, `device_resident` not forced off); the host and torch loops remain for everything else.
        from . import scf_tail
        self.tail = None
        # With several ranks rank 0 alone runs the tail (it is authoritative for the replicated state, grid_shard.ReplicaSync) and
        # [dm | cocc | scalars] go out in one broadcast; `self.fused` tells every rank to walk that loop.
        want_tail = (self.occ_solver is not None and device_resident is not False and ao_mode == "resident"
                     and scf_tail.supported(nao, inp.nocc)) if fused_tail is None else bool(fused_tail)
        self.fused = bool(want_tail)
        # one rank: the fused loop queues the next cycle's J / K and sweep behind this cycle's tail, before it waits (False: after)
        self.prequeue = True
        if want_tail:
            if not scf_tail.supported(nao, inp.nocc) or ao_mode != "resident":
                raise ValueError(f"fused_tail: resident AO planes, nao <= {scf_tail.MAX_NAO} and nocc <= {scf_tail.MAX_NOCC} are needed")
            if self.occ_solver is None:
                self.occ_solver = OccupiedRotation(inp.S, inp.nocc, None, full=self.eigh)      # the counters the drivers report; the rotation itself runs in the kernel
            if rank == 0:
                self.tail = scf_tail.ScfTail(self.solver.lib, inp.Hcore, inp.S, inp.nocc, self.dev)
        if self.device_resident or self.diis_device is not None or self.eigh.on_device:
            # rocBLAS / hipSOLVER load their code objects and create their handles on first use (~0.1-0.3 s in all):
            # done here, on operands of the run's own shapes, so that it is booked as initialisation -- where the
            # reference books cublasCreate (a member of XCSolver, dft_solver.cu:532, created with the solver) -- not as SCF time
            a = torch.eye(nao, dtype=f64, device=self.dev)
            (a @ a)[:, :inp.nocc].T @ a
            torch.linalg.solve(a[:9, :9], a[:9, :1])
            if self.device_resident or self.eigh.on_device:
                torch.linalg.eigh(a)
                torch.linalg.eigh(a[:inp.nocc, :inp.nocc])
            del a
        torch.cuda.synchronize()
        self.init_time = time.time() - t0

    def _dev(self, a):
        """A host array as a C-contiguous float64 tensor on this backend's device."""
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=self.torch.float64, device=self.dev)

    # ---- host-loop interface ------------------------------------------------------------------
    def set_state(self, dm, cocc):
        """[dm | cocc] in ONE pinned upload (dft.py:200 uploads dm alone; cocc = sqrt(2) C_occ feeds the
        factorised exchange)."""
        n2 = self.nao * self.nao
        self._pin_up[:n2].copy_(self.torch.as_tensor(np.ascontiguousarray(dm)).reshape(-1))
        self._pin_up[n2:].copy_(self.torch.as_tensor(np.ascontiguousarray(cocc)).reshape(-1))
        self._up.copy_(self._pin_up, non_blocking=True)

    def fock_parts(self, want_k):
        """(J, K or None, Exc, Vxc_raw, seconds in the XC sweep, seconds in J/K) as numpy arrays: the device
        work of one cycle and ONE pinned download of [J | K | Vxc].  Identical on every rank."""
        t0 = time.time()
        exc, t_xc = self._device_parts(want_k)
        t_dev = time.time() - t0
        self._pin_down.copy_(self._down, non_blocking=True)
        self.torch.cuda.synchronize()
        n, n2 = self.nao, self.nao * self.nao
        h = self._pin_down.numpy()
        J, K, V = (h[k * n2:(k + 1) * n2].reshape(n, n).copy() for k in range(3))
        return J, (K if want_k else None), exc, V, t_xc, t_dev - t_xc

    # ---- device work of one cycle (both loops) --------------------------------------------------
    def _device_parts(self, want_k):
        """J, K, Vxc_raw into d_J / d_K / d_v (all-reduced over the ranks when world > 1); returns (Exc, XC seconds)."""
        if self.world > 1:
            self._want_k = want_k
            t0 = time.time()
            parts = self._sharded.compute(self.d_dm, self.d_cocc)
            self.d_v.copy_(parts.vxc); self.d_J.copy_(parts.J)
            if want_k:
                self.d_K.copy_(parts.K)
            return parts.exc, time.time() - t0
        self._jk_device(want_k)
        self.torch.cuda.synchronize()      # J/K are asynchronous: without this the XC bracket below would include them
        t0 = time.time()
        exc = self._xc_device()
        return exc, time.time() - t0

    def _jk_device(self, want_k):
        """This rank's J (and K) into d_J / d_K; zeros when it holds no vectors / no ERI rows."""
        n = self.nao
        if self.d_chol is not None and self.d_chol.shape[0]:
            self.solver.compute_jk_factorized(n, self.d_chol.shape[0], self.nocc, self.d_chol, self.d_dm,
                                              self.d_cocc if want_k else None, self.d_J, self.d_K if want_k else None)
        elif self.d_eri is not None and self.world == 1 and want_k:
            self.solver.compute_jk(n, self.d_eri, self.d_dm, self.d_J, self.d_K)      # dft.py:203 + 218 in one pass
        elif self.d_eri is not None and self.world == 1:
            self.solver.compute_coulomb(n, self.d_eri, self.d_dm, self.d_J)          # dft.py:203
        elif self.d_eri is not None:
            # row block [rlo, rhi) of the ERI: J.ravel()[rlo:rhi] = ERI[rlo:rhi, :] . vec(D) (dft_solver.cu:550-555 on
            # a row slice), K_ik += sum_jl (ij|kl) D_jl over this rank's (ij) rows (dft.py:218); the all-reduce of
            # ShardedFock assembles both (disjoint rows of J, partial sums of K)
            rlo, rhi = self.eri_rows
            self.solver.compute_jk_rows(n, rlo // n, rhi // n, self.d_eri, self.d_dm, self.d_J, self.d_K if want_k else None)
        else:
            self.d_J.zero_(); self.d_K.zero_()

    def _xc_device(self):
        if not self.ngrid:
            self.d_v.zero_()
            return 0.0
        if self.ao_mode == "direct":
            self.solver.compute_xc_direct(self.shells, self.ngrid, self.d_coords, self.d_w, self.d_dm, self.d_v, self._d_exc, self.ao_chunk)
            return float(self._d_exc.item())                                             # device sync, like the ABI call
        if self.meta:
            exc = self.solver.compute_xc_meta(self.ngrid, self.nao, self.d_dm, self.d_ao, self.d_w, self.d_v, self.d_gr)
        elif self.xc_occ:
            exc = self.solver.compute_xc_occ(self.ngrid, self.nao, self.nocc, self.d_cocc, self.d_ao, self.d_w, self.d_v, self.d_gr, self.d_dm)
        else:
            exc = self.solver.compute_xc(self.ngrid, self.nao, self.d_dm, self.d_ao, self.d_w, self.d_v, self.d_gr)
        self.torch.cuda.synchronize()                                                # dft.py:205-208
        return exc

    # world > 1: the two local steps as ShardedFock wants them
    def _local_sweep(self, dm):
        return self._xc_device(), self.d_v

    def _local_jk(self, dm, cocc):
        self._jk_device(self._want_k)
        return self.d_J, (self.d_K if self._want_k else None)


    # ---- open-shell (scf.run_uks): one rank, resident AO planes, the host loop -----------------------------------------
    def _uks_check(self, meta=False, hint=None):
        if meta:
            if not self.meta:
                raise ValueError(f"uks_meta_parts is the open-shell sweep of a meta-GGA (DFT_ComputeXCMetaSpin): {self.functional} is not "
                                 "one (it carries no tpss_x / tpss_c weight); its open-shell sweep is uks_parts")
        else:
            functionals.refuse_meta(self.solver.functional, "open-shell DFT (UKS)", hint)
        if self.world > 1:
            raise ValueError("open-shell DFT (UKS) runs on one rank: the grid of this backend is sharded over several")
        if self.ao_mode != "resident":
            raise ValueError("open-shell DFT (UKS) needs resident AO planes (--ao resident), not --ao direct")
        if self.dm_factor:
            raise ValueError("open-shell DFT (UKS) does not factorise its density matrices on the device: run without dm_factor")
        if self.fused or self.device_resident:
            raise ValueError("open-shell DFT (UKS) walks the host loop: build the backend with fused_tail=False and "
                             "device_resident=False (the fused and the device-resident tail are closed-shell)")

    def uks_parts(self, dm_a, dm_b, cocc_a, cocc_b, want_k):
        """(J, K_alpha or None, K_beta or None, Exc, V_alpha_raw, V_beta_raw) of the spin density matrices dm_s = cocc_s
        cocc_s^T, as numpy arrays: J of the total density and K of each spin through the closed-shell entries (Cholesky
        vectors: one DFT_ComputeJKFactorized call for J with the total dm alone, one per spin for K with that spin's dm and
        orbitals), Exc and the two potentials from DFT_ComputeXCSpin.  A spin without electrons has K = 0."""
        self._uks_check(hint=functionals.OPEN_SHELL_META_HINT)
        return self._uks_parts(dm_a, dm_b, cocc_a, cocc_b, want_k, self.solver.compute_xc_spin)

    def uks_meta_parts(self, dm_a, dm_b, cocc_a, cocc_b, want_k):
        """uks_parts for a meta-GGA (run_uks(meta=True)): the same return tuple, J and K taken exactly as there, Exc and the
        two potentials (tau terms included) from DFT_ComputeXCMetaSpin.  Refuses what uks_parts refuses but the meta-GGA, and
        a functional that is not one."""
        self._uks_check(meta=True)
        return self._uks_parts(dm_a, dm_b, cocc_a, cocc_b, want_k, self.solver.compute_xc_meta_spin)

    def _uks_parts(self, dm_a, dm_b, cocc_a, cocc_b, want_k, sweep):
        t, n = self.torch, self.nao
        d_s = [self._dev(dm_a), self._dev(dm_b)]
        d_c = [self._dev(cocc_a), self._dev(cocc_b)]
        self.d_dm.copy_(d_s[0] + d_s[1])
        if getattr(self, "_uks_out", None) is None:
            self._uks_out = t.zeros((6, n, n), dtype=t.float64, device=self.dev)      # J | K_a | K_b | V_a | V_b | scratch
        o = self._uks_out
        o.zero_()
        if self.d_chol is not None:
            naux = self.d_chol.shape[0]
            self.solver.compute_jk_factorized(n, naux, max(d_c[0].shape[1], 1), self.d_chol, self.d_dm, None, o[0], None)
            for k in range(2):
                if want_k and d_c[k].shape[1]:
                    self.solver.compute_jk_factorized(n, naux, d_c[k].shape[1], self.d_chol, d_s[k], d_c[k], None, o[1 + k])
        else:
            self.solver.compute_coulomb(n, self.d_eri, self.d_dm, o[0])
            for k in range(2):
                if want_k and d_c[k].shape[1]:
                    self.solver.compute_exchange(n, self.d_eri, d_s[k], o[1 + k])
        exc = sweep(self.ngrid, n, d_s[0], d_s[1], self.d_ao, self.d_w, o[3], o[4], self.d_gr)
        t.cuda.synchronize()
        h = o.cpu().numpy()
        return h[0], (h[1] if want_k else None), (h[2] if want_k else None), exc, h[3], h[4]

    # ---- open-shell linear response (excitations.UksResponseOperators, response.polarizability of a run_uks result) -----
    def uks_response_prepare(self, dm_a, dm_b):
        """DFT_FxcPrepareSpinPol at the converged spin density matrices: the table of the open-shell response of Vxc, kept
        in the solver beside (and apart from) the closed-shell tables."""
        self._uks_check()
        self._response_check()
        t = self.torch
        self._d_dm0_s = [self._dev(d) for d in (dm_a, dm_b)]
        self.solver.fxc_prepare_spinpol(self.ngrid, self.nao, self._d_dm0_s[0], self._d_dm0_s[1], self.d_ao, self.d_w, self.d_gr)
        t.cuda.synchronize()

    def uks_excitation_parts(self, A_a, Bs_a, A_b, Bs_b, want_k):
        """(J, M_a, M_b, V1_a, V1_b), each (nvec, nao, nao) as numpy arrays (M_s None without want_k), of the trials
        D_s,k = A_s B_s,k^T + B_s,k A_s^T with A_s (nao, n_s) and Bs_s (nvec, nao, n_s): J[D_a,k + D_b,k], the unsymmetrised
        M_s,k = K[A_s B_s,k^T] (K[D+-] = M +- M^T) and the raw V1_s[D_a,k, D_b,k] of one DFT_FxcApplySpinPol per trial.
        Cholesky vectors: one DFT_ComputeJKFactorizedResponse call per spin, the two J summed.  Dense ERI:
        DFT_ComputeCoulomb on the total and DFT_ComputeJK per spin.  A spin without electrons launches nothing for J and
        M and contributes zeros.  After uks_response_prepare."""
        self._uks_check()
        self._response_check()
        t, n = self.torch, self.nao
        f64 = t.float64
        d_A = [self._dev(a) for a in (A_a, A_b)]
        d_B = [self._dev(b) for b in (Bs_a, Bs_b)]
        for a, b in zip(d_A, d_B):
            if b.dim() != 3 or a.dim() != 2 or a.shape[0] != n or tuple(b.shape[1:]) != tuple(a.shape) or b.shape[0] != d_B[0].shape[0]:
                raise ValueError(f"uks_excitation_parts: A_s (nao, n_s) and Bs_s (nvec, nao, n_s) expected, got {tuple(a.shape)} and {tuple(b.shape)}")
        nvec = d_B[0].shape[0]
        out = t.zeros((6, nvec, n, n), dtype=f64, device=self.dev)                   # J | M_a | M_b | V1_a | V1_b | J of beta
        AB = [t.matmul(a.unsqueeze(0), b.transpose(1, 2)).contiguous() for a, b in zip(d_A, d_B)]
        Dp = [(x + x.transpose(1, 2)).contiguous() for x in AB]
        if self.d_chol is not None:
            for s in range(2):
                if d_A[s].shape[1]:
                    self.solver.compute_jk_factorized_response(n, self.d_chol.shape[0], d_A[s].shape[1], nvec, self.d_chol, d_A[s], d_B[s],
                                                               out[0] if s == 0 else out[5], out[1 + s] if want_k else None)
            out[0].add_(out[5])
        else:
            Dt = (Dp[0] + Dp[1]).contiguous()
            for k in range(nvec):
                self.solver.compute_coulomb(n, self.d_eri, Dt[k], out[0, k])
                for s in range(2):
                    if want_k and d_A[s].shape[1]:
                        self.solver.compute_jk(n, self.d_eri, AB[s][k], None, out[1 + s, k])
        for k in range(nvec):
            self.solver.fxc_apply_spinpol(self.ngrid, n, Dp[0][k], Dp[1][k], self.d_ao, out[3, k], out[4, k], self.d_gr)
        t.cuda.synchronize()
        h = out.cpu().numpy()
        return h[0], (h[1] if want_k else None), (h[2] if want_k else None), h[3], h[4]


    # ---- linear response (response.polarizability): one rank, resident AO planes ------------------------------
    def _response_check(self):
        functionals.refuse_meta(self.solver.functional, "linear response (fxc / CPKS / excitations)")
        if self.world > 1:
            raise ValueError("linear response (fxc / CPKS) runs on one rank: the grid of this backend is sharded over several")
        if self.ao_mode != "resident":
            raise ValueError("linear response (fxc / CPKS) needs resident AO planes (--ao resident), not --ao direct")

    def ground_state_parts(self, dm, cocc, want_k):
        """(J, K or None, Vxc_raw) of a density, as numpy arrays: the parts of its Fock matrix."""
        self._response_check()
        return self._ground_state_parts(dm, cocc, want_k)

    def _ground_state_parts(self, dm, cocc, want_k):
        self.set_state(dm, cocc)
        J, K, _, V, _, _ = self.fock_parts(want_k)
        return J, K, V

    def response_prepare(self, dm0, cocc=None, kind="singlet"):
        """DFT_FxcPrepare at dm0 (through cocc, dm0 = cocc cocc^T, when given and the loop sweeps that way); kind "triplet"
        (or "singlet-spin"): DFT_FxcPrepareSpin, the table of the spin-resolved energy bodies in its own slot."""
        self._response_check()
        from .response import spin_kind
        t = self.torch
        self._d_dm0 = self._dev(dm0)
        d_c = self._dev(cocc) if (cocc is not None and self.xc_occ) else None
        k = spin_kind(kind)
        if k:
            self.solver.fxc_prepare_spin(self.ngrid, self.nao, self._d_dm0, self.d_ao, self.d_w, self.d_gr, d_c, 0 if d_c is None else d_c.shape[1], k)
        else:
            self.solver.fxc_prepare(self.ngrid, self.nao, self._d_dm0, self.d_ao, self.d_w, self.d_gr, d_c, 0 if d_c is None else d_c.shape[1])
        n = self.nao
        self._r_dm1 = t.zeros((n, n), dtype=t.float64, device=self.dev)
        self._r_out = t.zeros((4, n, n), dtype=t.float64, device=self.dev)      # J | K | V1 | K of the second factor

    def response_parts(self, dm1, want_k, factors=None):
        """(J, K or None, V1_raw) of a symmetric perturbation dm1, as numpy arrays.  Dense ERI: DFT_ComputeJK as it
        stands.  Cholesky vectors: J from dm1, and K by linearity from two DFT_ComputeJKFactorized calls -- with
        dm1 = A B^T + B A^T (`factors` = (A, B), what a CPKS step has) and c+- = (A +- B)/sqrt(2),
        K[dm1] = K[c+ c+^T] - K[c- c-^T]."""
        self._response_check()
        t, n = self.torch, self.nao
        self._r_dm1.copy_(t.as_tensor(np.ascontiguousarray(dm1), dtype=t.float64))
        d_J, d_K, d_V, d_K2 = self._r_out
        if self.d_chol is not None:
            naux = self.d_chol.shape[0]
            self.solver.compute_jk_factorized(n, naux, 0, self.d_chol, self._r_dm1, None, d_J, None)
            if want_k:
                if factors is None:
                    raise ValueError("response_parts: K from Cholesky vectors needs dm1 = A B^T + B A^T as factors=(A, B)")
                A, B = (np.asarray(x, dtype=np.float64) for x in factors)
                for sgn, out in ((1.0, d_K), (-1.0, d_K2)):
                    c = self._dev((A + sgn * B) / np.sqrt(2.0))
                    self.solver.compute_jk_factorized(n, naux, c.shape[1], self.d_chol, None, c, None, out)
                    t.cuda.synchronize()     # `c` is released when the loop moves on
                d_K.sub_(d_K2)
        elif want_k:
            self.solver.compute_jk(n, self.d_eri, self._r_dm1, d_J, d_K)
        else:
            self.solver.compute_coulomb(n, self.d_eri, self._r_dm1, d_J)
        self.solver.fxc_apply(self.ngrid, n, self._r_dm1, self.d_ao, d_V, self.d_gr)
        self.torch.cuda.synchronize()
        h = self._r_out.cpu().numpy()
        return h[0], (h[1] if want_k else None), h[2]

    # ---- XC part of the nuclear gradient (gradients.py): one rank -----------------------------------------------
    XC_GRADIENT_HESS_BYTES = 1.0e9      # the six Hessian planes of a grid slice stay within about this

    def xc_gradient(self, dm, slice_rows=None):
        """G (nao, 3) as a numpy array: dExc / d(centre of basis function mu) at fixed points and weights
        (DFT_ComputeXCGradient), summed over slices of the grid.  The Hessian planes of a slice are evaluated into a reused
        buffer (DFT_EvalAOHess); the AO and gradient planes are the resident ones where the backend holds them (a slice of
        the three gradient planes is copied together, the entry wants them back to back) and are evaluated per slice
        otherwise (an LDA-class run keeps no gradient planes, --ao direct keeps none).  slice_rows: rows per slice (default:
        what keeps the Hessian planes within XC_GRADIENT_HESS_BYTES)."""
        return self._xc_gradient_slices(slice_rows, self._xc_gradient_calls(dm)[0])

    def xc_gradient_spin(self, dm_a, dm_b, slice_rows=None):
        """G (nao, 3) as a numpy array for an open-shell state: dExc[dm_a, dm_b] / d(centre of basis function mu) at fixed
        points and weights (DFT_ComputeXCGradientSpin), summed over slices of the grid exactly as xc_gradient does."""
        return self._xc_gradient_slices(slice_rows, self._xc_gradient_calls(dm_a, dm_b)[0])

    def _xc_gradient_calls(self, *dms, meta=False):
        """(entry, edens): the library calls of a grid slice for one matrix (the closed shell; meta: of a meta-GGA, through
        DFT_ComputeXCGradientMeta / DFT_ComputeXCEnergyDensityMeta) or two (an open-shell state; meta: through
        DFT_ComputeXCGradientMetaSpin / DFT_ComputeXCEnergyDensityMetaSpin): entry(m, ao, w, d_out, gr, hs)
        the XC gradient, edens(m, ao, gr, d_e) the energy density, on the uploaded matrices.  The flag travels on the entry
        (entry.meta): whoever runs it refuses a meta-GGA unless the entry is the meta-GGA's own."""
        if len(dms) == 2:
            self._uks_check(meta=meta)
        d, s = [self._dev(x) for x in dms], self.solver
        grad, dens = (s.compute_xc_gradient_meta_spin, s.compute_xc_energy_density_meta_spin) if meta and len(dms) == 2 else \
                     (s.compute_xc_gradient_meta, s.compute_xc_energy_density_meta) if meta else \
                     (s.compute_xc_gradient_spin, s.compute_xc_energy_density_spin) if len(dms) == 2 else \
                     (s.compute_xc_gradient, s.compute_xc_energy_density)
        entry = lambda m, ao, w, out, gr, hs: grad(m, self.nao, *d, ao, w, out, gr, hs)      # noqa: E731
        entry.meta = meta
        return entry, lambda m, ao, gr, e: dens(m, self.nao, *d, ao, e, gr)

    def _xc_gradient_slices(self, slice_rows, entry, block=None, after=None):
        """The slicing xc_gradient, xc_gradient_spin and xc_gradient_meta share: entry(m, ao, w, d_out, gr, hs) is the library
        call of a slice.  block = (lo, hi): the rows of the grid to sweep (default: all of it); after(lo, hi, ao, gr), when
        given, runs behind the entry of every slice on the same planes (the grid response takes the energy density there).
        A meta-GGA is refused unless the entry says it is the meta-GGA form (entry.meta, _xc_gradient_calls; a meta solver
        always takes the Hessian planes)."""
        if not getattr(entry, "meta", False):
            functionals.refuse_meta(self.solver.functional, "the XC part of the nuclear gradient", functionals.META_GRADIENT_HINT)
        if self.world > 1:
            raise ValueError("the XC gradient runs on one rank: the grid of this backend is sharded over several")
        if self.dm_factor:
            raise ValueError("the XC gradient takes the density matrix itself: run without dm_factor")
        t, n, s = self.torch, self.nao, self.solver
        b_lo, b_hi = (0, self.ngrid) if block is None else (int(block[0]), int(block[1]))
        ng = b_hi - b_lo
        whole = ng == self.ngrid
        f64 = t.float64
        rows = int(slice_rows) if slice_rows else max(16, int(self.XC_GRADIENT_HESS_BYTES // (48 * n)) // 16 * 16)
        rows = max(1, min(rows, ng))
        gga = s.needs_gradient
        d_out = t.zeros((n, 3), dtype=f64, device=self.dev)
        d_G = t.zeros((n, 3), dtype=f64, device=self.dev)
        d_hess = t.empty(6 * rows * n, dtype=f64, device=self.dev) if gga else None
        own_gr = self.d_gr is None
        own_ao = self.d_ao is None or own_gr        # DFT_EvalAO writes the values along with the gradients
        d_gr_s = t.empty(3 * rows * n, dtype=f64, device=self.dev) if (own_gr or rows < ng or not whole) else None
        d_ao_s = t.empty(rows * n, dtype=f64, device=self.dev) if own_ao else None
        for lo in range(b_lo, b_hi, rows):
            hi = min(lo + rows, b_hi)
            m = hi - lo
            coords = self.d_coords[lo:hi]
            if own_gr:
                ao, gr = d_ao_s[:m * n].view(m, n), d_gr_s[:3 * m * n].view(3, m, n)
                s.eval_ao(self.shells, coords, m, ao, gr)
            elif rows < ng or not whole:
                ao, gr = self.d_ao[lo:hi], d_gr_s[:3 * m * n].view(3, m, n)
                gr.copy_(self.d_gr[:, lo:hi])
            else:
                ao, gr = self.d_ao, self.d_gr
            hs = None
            if gga:
                hs = d_hess[:6 * m * n].view(6, m, n)
                s.eval_ao_hess(self.shells, coords, m, hs)
            t.cuda.synchronize()
            entry(m, ao, self.d_w[lo:hi], d_out, gr, hs)
            t.cuda.synchronize()
            d_G += d_out
            if after is not None:
                after(lo, hi, ao, gr)
                t.cuda.synchronize()
        t.cuda.synchronize()
        return d_G.cpu().numpy()

    # ---- grid response of the nuclear gradient (gradients.py): one rank ---------------------------------------------
    def xc_grid_response(self, dm, slice_rows=None):
        """(natm, 3) as a numpy array: what the motion of the grid with the atoms adds to the XC term of dE/dR_A,

            xc_grid[A] = -sum_mu G^(A)[mu] + sum_g w0_g e_g D_A cell_g,

        G^(A) = xc_gradient's G on the rows of the grid atom A owns (the existing slicing per atom block: a block is cut
        further when its Hessian planes exceed XC_GRADIENT_HESS_BYTES), e_g from DFT_ComputeXCEnergyDensity on the planes
        of each slice, the second sum from DFT_BeckeWeightGradient."""
        return self._xc_grid_response(slice_rows, *self._xc_gradient_calls(dm))

    def xc_grid_response_spin(self, dm_a, dm_b, slice_rows=None):
        """xc_grid_response for an open-shell state: DFT_ComputeXCGradientSpin and DFT_ComputeXCEnergyDensitySpin per block."""
        return self._xc_grid_response(slice_rows, *self._xc_gradient_calls(dm_a, dm_b))

    def _xc_grid_response(self, slice_rows, entry, edens):
        from . import basis, grid_gen
        if not entry.meta:
            functionals.refuse_meta(self.solver.functional, "the grid response of the nuclear gradient", functionals.META_GRADIENT_HINT)
        if self.world > 1:
            raise ValueError("the grid response runs on one rank: the grid of this backend is sharded over several")
        if self.dm_factor:
            raise ValueError("the grid response takes the density matrix itself: run without dm_factor")
        symbols, xyz = self._atoms
        own, w0 = getattr(self._grids, "atom_index", None), getattr(self._grids, "atomic_weights", None)
        if own is None or w0 is None or symbols is None or xyz is None:
            raise ValueError("the grid response needs the grid's atom_index and atomic_weights (grid_gen.Grids) and the atoms of the input: "
                             "this grid does not say which atom a point moves with")
        xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
        own, w0 = np.asarray(own), np.asarray(w0, dtype=np.float64)
        natm = xyz.shape[0]
        if len(symbols) != natm or own.shape != (self.ngrid,) or w0.shape != (self.ngrid,) or \
                (self.ngrid and (own.min() < 0 or own.max() >= natm)):
            raise ValueError(f"the grid response: the grid's atom_index / atomic_weights do not match the {natm} atoms and {self.ngrid} points of this backend")
        t, n = self.torch, self.nao
        # the blocks of consecutive rows one atom owns (grid_gen.Grids: one per atom)
        cut = np.flatnonzero(np.diff(own)) + 1
        los, his = np.concatenate([[0], cut]), np.concatenate([cut, [self.ngrid]])
        d_e = t.zeros(max(self.ngrid, 1), dtype=t.float64, device=self.dev)
        out = np.zeros((natm, 3))

        def after(lo, hi, ao, gr):
            edens(hi - lo, ao, gr if self.solver.needs_gradient else None, d_e[lo:hi])

        for lo, hi in zip(los, his):
            if hi > lo:
                G = self._xc_gradient_slices(slice_rows, entry, block=(int(lo), int(hi)), after=after)
                out[int(own[lo])] -= G.sum(axis=0)
        d_f = d_e[:self.ngrid] * t.as_tensor(w0, dtype=t.float64, device=self.dev)
        d_own = t.as_tensor(own.astype(np.int32), dtype=t.int32, device=self.dev)
        d_out = t.zeros((natm, 3), dtype=t.float64, device=self.dev)
        radii = grid_gen.bragg_radii_bohr([basis.atomic_number(sy) for sy in symbols])
        t.cuda.synchronize()
        self.solver.becke_weight_gradient(self.ngrid, xyz, radii, self.d_coords, d_own, d_f, d_out)
        t.cuda.synchronize()
        return out + d_out.cpu().numpy()

    # ---- nuclear gradient of a meta-GGA (gradients.nuclear_gradient(meta=True)): one rank, closed shell ----------------
    def _meta_gradient_check(self, who):
        if not self.meta:
            raise ValueError(f"{who} is the gradient of a meta-GGA (DFT_ComputeXCGradientMeta): {self.functional} is not one (it "
                             f"carries no tpss_x / tpss_c weight); its gradient is {who.replace('_meta', '')}")

    def xc_gradient_meta(self, dm, slice_rows=None):
        """xc_gradient for a meta-GGA: G (nao, 3) with the tau term (DFT_ComputeXCGradientMeta), summed over slices of the grid
        exactly as xc_gradient does.  Refuses what xc_gradient refuses but the meta-GGA, and a functional that is not one."""
        self._meta_gradient_check("xc_gradient_meta")
        return self._xc_gradient_slices(slice_rows, self._xc_gradient_calls(dm, meta=True)[0])

    def xc_grid_response_meta(self, dm, slice_rows=None):
        """xc_grid_response for a meta-GGA: DFT_ComputeXCGradientMeta and DFT_ComputeXCEnergyDensityMeta per block."""
        self._meta_gradient_check("xc_grid_response_meta")
        return self._xc_grid_response(slice_rows, *self._xc_gradient_calls(dm, meta=True))

    def xc_gradient_meta_spin(self, dm_a, dm_b, slice_rows=None):
        """xc_gradient_spin for a meta-GGA: G (nao, 3) with the tau term of either spin (DFT_ComputeXCGradientMetaSpin), summed
        over slices of the grid exactly as xc_gradient does.  Refuses what xc_gradient_spin refuses but the meta-GGA, and a
        functional that is not one."""
        self._meta_gradient_check("xc_gradient_meta_spin")
        return self._xc_gradient_slices(slice_rows, self._xc_gradient_calls(dm_a, dm_b, meta=True)[0])

    def xc_grid_response_meta_spin(self, dm_a, dm_b, slice_rows=None):
        """xc_grid_response_spin for a meta-GGA: DFT_ComputeXCGradientMetaSpin and DFT_ComputeXCEnergyDensityMetaSpin per block."""
        self._meta_gradient_check("xc_grid_response_meta_spin")
        return self._xc_grid_response(slice_rows, *self._xc_gradient_calls(dm_a, dm_b, meta=True))

    def ground_state_parts_meta(self, dm, cocc, want_k):
        """ground_state_parts for a meta-GGA (the Fock matrix of W in the gradient): set_state and fock_parts, which sweep through
        DFT_ComputeXCMeta.  ground_state_parts itself serves the response and keeps refusing a meta-GGA."""
        self._meta_gradient_check("ground_state_parts_meta")
        return self._ground_state_parts(dm, cocc, want_k)

    # ---- two-electron part of the nuclear gradient on the device (integrals.DeviceGrad2e): one rank ----------------
    def _grad2e_engine(self):
        """integrals.DeviceGrad2e on this backend's shells: opened by the first call, alive until close()."""
        if self.world > 1:
            raise ValueError("the device two-electron gradient runs on one rank: this backend is one of several")
        if self._grad2e is None:
            from .integrals import DeviceGrad2e
            self._grad2e = DeviceGrad2e(self.shells, self._lib_path)
        return self._grad2e

    def grad2e(self, dm, c_hf):
        """(natm, 3) as a numpy array: what integrals.grad2e(shells, dm, c_hf) computes on the host, from DFT_Grad2e.  The
        handle is opened by the first call and lives until close()."""
        g = self._grad2e_engine()
        with self.torch.cuda.device(self.dev):
            return g.grad(dm, c_hf)

    def grad2e_spin(self, dm_a, dm_b, c_hf):
        """(natm, 3) as a numpy array: what integrals.grad2e_spin(shells, dm_a + dm_b, dm_a - dm_b, c_hf) computes on the
        host, from DFT_Grad2eSpin on grad2e's handle: one pass over the derivative integrals for both spins."""
        g = self._grad2e_engine()
        dm_a, dm_b = np.asarray(dm_a, dtype=np.float64), np.asarray(dm_b, dtype=np.float64)
        with self.torch.cuda.device(self.dev):
            return g.grad_spin(dm_a + dm_b, dm_a - dm_b, c_hf)

    def close(self):
        """Releases the handles this backend opened on demand (the buffers go with the object)."""
        g, self._grad2e = getattr(self, "_grad2e", None), None
        if g is not None:
            g.close()

    __del__ = close

    def excitation_parts(self, A, Bs, want_k, kind="singlet"):
        """(J, M or None, V1_raw), each (nvec, nao, nao) as numpy arrays, of the trials D_k = A B_k^T + B_k A^T with A
        (nao, nocc) and Bs (nvec, nao, nocc): J[D_k], the unsymmetrised M_k = K[A B_k^T] -- K[D]_mn = sum_ls (ml|ns) D_ls,
        so K[A B_k^T +- B_k A^T] = M_k +- M_k^T, the antisymmetric combination included -- and V1[D_k].  Cholesky
        vectors: ONE DFT_ComputeJKFactorizedResponse call for all trials.  Dense ERI: DFT_ComputeJK per trial (its K is
        the literal einsum, for any dm).  One DFT_FxcApply per trial either way.  After response_prepare.
        kind "triplet": V1 by DFT_FxcApplyKind from the spin-flip table (after response_prepare(kind="triplet")) and no
        J at all -- None is returned for it, no Coulomb kernel runs on either path."""
        self._response_check()
        from .response import spin_kind
        kd = spin_kind(kind)
        want_j = kd != 1
        t, n = self.torch, self.nao
        f64 = t.float64
        d_A, d_B = self._dev(A), self._dev(Bs)
        if d_B.dim() != 3 or d_A.dim() != 2 or d_A.shape[0] != n or tuple(d_B.shape[1:]) != tuple(d_A.shape):
            raise ValueError(f"excitation_parts: A (nao, nocc) and Bs (nvec, nao, nocc) expected, got {tuple(d_A.shape)} and {tuple(d_B.shape)}")
        nvec, nocc = d_B.shape[0], d_A.shape[1]
        out = t.zeros((3, nvec, n, n), dtype=f64, device=self.dev)                   # J | M | V1
        AB = t.matmul(d_A.unsqueeze(0), d_B.transpose(1, 2))                           # A B_k^T
        Dp = (AB + AB.transpose(1, 2)).contiguous()
        if self.d_chol is not None:
            if want_j or want_k:
                self.solver.compute_jk_factorized_response(n, self.d_chol.shape[0], nocc, nvec, self.d_chol, d_A, d_B,
                                                           out[0] if want_j else None, out[1] if want_k else None)
        else:
            for k in range(nvec):
                if want_j:
                    self.solver.compute_coulomb(n, self.d_eri, Dp[k], out[0, k])
                if want_k:
                    self.solver.compute_jk(n, self.d_eri, AB[k], None, out[1, k])
        for k in range(nvec):
            if kd:
                self.solver.fxc_apply_kind(self.ngrid, n, Dp[k], self.d_ao, out[2, k], self.d_gr, kd)
            else:
                self.solver.fxc_apply(self.ngrid, n, Dp[k], self.d_ao, out[2, k], self.d_gr)
        t.cuda.synchronize()
        h = out.cpu().numpy()
        return (h[0] if want_j else None), (h[1] if want_k else None), h[2]


def run_scf(inp, backend, functional, max_cycle=200, conv_e=1e-8, conv_dm=1e-6, log=print):
    from .hostinfo import blas_threads
    # host LAPACK/BLAS never on every visible core (256 on a 16-core share: ~90 ms stalls): one thread where the full
    # solver is LAPACK's (_HIPSOLVER_FROM), above it the pool gets the CPU share
    with blas_threads(1 if inp.S.shape[0] < _HIPSOLVER_FROM else None):
        if getattr(backend, "fused", False):
            return _run_scf_fused(inp, backend, functional, max_cycle, conv_e, conv_dm, log)
        if getattr(backend, "device_resident", False):
            return _run_scf_device(inp, backend, functional, max_cycle, conv_e, conv_dm, log)
        return _run_scf(inp, backend, functional, max_cycle, conv_e, conv_dm, log)


class _CycleLedger:
    """The bookkeeping of one SCF run, the same in all four loops: the exchange weight, the log's header, the per-cycle
    times, `res` with `per_cycle`, the energy of the last cycle, the QCDFT_SCF_PROFILE rows and the closing statistics.
    A loop creates one where its cycles start, calls start() and cycle() once per cycle and returns finish()."""

    def __init__(self, inp, functional, conv_e, conv_dm, log, **res):
        self.c_hf = functionals.resolve(functional).c_hf     # dft.py:197 (0.2 for B3LYP, else 0) for any functional
        self.want_k = self.c_hf != 0.0
        self.E_nuc, self.conv_e, self.conv_dm, self.log = inp.E_nuc, conv_e, conv_dm, log
        if log:
            log("\nSCF started!"); log("-" * 80)
            log(f"{'epoch':>4} {'tot energy':>15} {'Δenergy':>12} {'Δdensity':>12} {'HF_Ex':>12}"); log("-" * 80)
        self.E_old, self.xc_times, self.jk_times, self.it_times, self.t_start = 0.0, [], [], [], time.time()
        self.res = {"converged": False, **res}
        self.per_cycle = self.res["per_cycle"] = []          # (E_tot, |dm' - dm|) of every cycle
        self.prof = [] if os.environ.get("QCDFT_SCF_PROFILE") else None     # per-part times of a cycle's tail (a loop may add syncs for them)

    def start(self):
        self.t_it = time.time()
        return self.t_it

    def cycle(self, E_one, E_coul, E_xc, E_ex, ddm, **fields):
        """Books the cycle that start() opened -- energy from the NEW density (dft.py:236), its time (taken before the log
        line is written), the log line, `res` (with the loop's own `fields`) -- and says whether both thresholds of
        dft.py:243 are met.  The same scalars on every rank, so the same answer."""
        E_tot = E_one + E_coul + E_xc + E_ex + self.E_nuc
        dE, self.E_old = E_tot - self.E_old, E_tot
        self.it_times.append(time.time() - self.t_it)
        if self.log:
            self.log(f"{len(self.it_times):4d} {E_tot:18.8f} {dE:15.6e} {ddm:15.6e} {E_ex:12.6f}")
        self.res.update(E_tot=E_tot, E_one=E_one, E_coul=E_coul, E_xc=E_xc, E_ex_hf=E_ex, cycles=len(self.it_times), **fields)
        self.per_cycle.append((E_tot, ddm))
        return abs(dE) < self.conv_e and ddm < self.conv_dm

    def finish(self, parts_key=None, parts=(), title=""):
        """`res`, closed.  `parts_key`, `parts`: where the medians of the profile rows go and what their columns are."""
        res = self.res
        if self.prof:
            med = np.median(np.array(self.prof[1:] if len(self.prof) > 1 else self.prof), axis=0)
            res[parts_key] = dict(zip(parts, (float(x) for x in med)))
            if self.log:
                self.log(f"{title} (median ms per cycle): " + ", ".join(f"{k} {v:.3f}" for k, v in res[parts_key].items()))
        res["total_time"] = time.time() - self.t_start
        res["xc_ms_avg"] = 1e3 * sum(self.xc_times) / max(1, len(self.xc_times))     # dft.py:259 (includes the first call's allocations)
        steady = lambda ts: 1e3 * float(np.median(ts[1:] if len(ts) > 1 else ts))
        res["xc_ms"], res["jk_ms"], res["iter_ms"] = steady(self.xc_times), steady(self.jk_times), steady(self.it_times)  # medians past cycle 1
        res["cycle_ms"] = [round(1e3 * t, 4) for t in self.it_times]          # every cycle, the first (lazy allocations) included
        res["nelec_grid"] = None
        return res


def _aufbau_check(full_solve, root, flag, broadcast, log):
    """Is the occupied space that a rotation run converged in the AUFBAU one?  The rotation solver follows the occupied
    space continuously and never diagonalises the virtual block, so this is checked once, on the converged state, against
    eigh(F, S) of the converged Fock matrix: `full_solve()` gives (the full spectrum, |2 C_o C_o^T - dm|_F as a float)
    of that solve.  Rank 0 decides (`root`: this rank does), every rank hears it through `flag`, a one-element buffer of
    the kind that `broadcast` (ReplicaSync.broadcast_numpy, ReplicaSync.broadcast or None) moves.  Returns (ok, the
    spectrum if ok and this rank solved, else None).  After a mismatch -- an occupied/virtual level crossing that the
    solver followed through -- the caller resumes as the reference's loop, full solver and a fresh DIIS history."""
    spectrum = None
    if root:
        spectrum, gap = full_solve()
        flag[0] = float(gap < 1e-4)
    if broadcast:
        broadcast([flag])
    if float(flag[0]):
        return True, spectrum
    if log:
        log("     converged occupied space is not the aufbau one: continuing with eigh(F, S) every cycle")
    return False, None


def _run_scf(inp, backend, functional, max_cycle, conv_e, conv_dm, log):
    """Host form of the loop body (dft.py:199-266).  `backend` supplies either fock_parts(want_k) (HipBackend)
    or the reference-shaped pair jk(want_k) / xc() (the oracle backend of the tests)."""
    Hcore, S, nocc = inp.Hcore, inp.S, inp.nocc
    sync = getattr(backend, "replica_sync", None)
    root = getattr(backend, "rank", 0) == 0 or sync is None   # rank 0 is authoritative: DIIS + eigh run once, replicas receive the result
    solve_full = getattr(backend, "eigh", None) or (lambda F: eigh(F, S))
    occ = getattr(backend, "occ_solver", None)
    rotate, last_ddm = occ is not None, None   # `rotate` is cleared if the converged state fails _aufbau_check

    def solve(F):   # (orbital energies, C_occ): the loop never uses the virtual orbitals (dft.py:182,228)
        if rotate:
            e_, co_ = occ.occupied(F, last_ddm)
            return np.asarray(e_), np.asarray(co_)
        e_, C_ = solve_full(F)
        return e_, C_[:, :nocc]

    def checked():   # the converged Fock matrix through the full solver, for _aufbau_check
        e_x, C_x = solve_full(F)
        e_x, C_x = np.asarray(e_x), np.asarray(C_x)
        return e_x, float(np.linalg.norm(2.0 * C_x[:, :nocc] @ C_x[:, :nocc].T - dm_new))

    e, C = solve(Hcore)                                                                # dft.py:181
    cocc = np.ascontiguousarray(np.sqrt(2.0) * C)
    dm = cocc @ cocc.T                                                                 # = 2 C_occ C_occ^T, dft.py:182
    if sync:
        sync.broadcast_numpy([dm, cocc])                                               # replicas start from rank 0's guess
    diis = CDIIS(device=getattr(backend, "diis_device", None))
    led = _CycleLedger(inp, functional, conv_e, conv_dm, log)
    c_hf, want_k = led.c_hf, led.want_k
    for _ in range(max_cycle):
        t_it = led.start()
        if hasattr(backend, "fock_parts"):
            backend.set_state(dm, cocc)                                                # dft.py:200
            J, K, E_xc, Vraw, t_xc, t_jk = backend.fock_parts(want_k)
        else:
            backend.set_dm(dm)
            J, K = backend.jk(want_k)
            t_jk = time.time() - t_it
            E_xc, Vraw, t_xc = backend.xc()
        led.jk_times.append(t_jk); led.xc_times.append(t_xc)
        dm_new, cocc_new, scal = np.empty_like(dm), np.empty_like(cocc), np.zeros(4)
        if root:
            tp = [time.time()]
            Vxc = 0.5 * (Vraw + Vraw.T)                                                # dft.py:212
            F = Hcore + J + Vxc - (c_hf * 0.5 * K if K is not None else 0.0)           # dft.py:221,223
            tp.append(time.time())
            F = diis.update(S, dm, F, cocc=cocc)
            tp.append(time.time())
            e, C = solve(F)
            tp.append(time.time())
            cocc_new = np.ascontiguousarray(np.sqrt(2.0) * C)
            dm_new = cocc_new @ cocc_new.T
            scal = np.array([np.sum(dm_new * Hcore), 0.5 * np.sum(dm_new * J),
                             -0.25 * c_hf * np.sum(dm_new * K) if K is not None else 0.0,
                             np.linalg.norm(dm_new - dm)])
            tp.append(time.time())
            if led.prof is not None:
                led.prof.append([1e3 * (tp[0] - t_it - t_jk - t_xc)] + [1e3 * (b - a) for a, b in zip(tp, tp[1:])])
        if sync:
            sync.broadcast_numpy([dm_new, cocc_new, scal])
        E_one, E_coul, E_ex, last_ddm = (float(x) for x in scal)
        if led.cycle(E_one, E_coul, E_xc, E_ex, last_ddm, dm=dm_new, mo_energy=e):
            ok, e_x = _aufbau_check(checked, root, np.ones(1), sync and sync.broadcast_numpy, log) if rotate else (True, None)
            led.res["mo_energy"] = e if e_x is None else e_x                           # the exact orbital energies, virtual ones included
            if ok:
                led.res["converged"] = True
                break
            rotate = False
            diis = CDIIS(device=getattr(backend, "diis_device", None))   # its history belongs to the other state
        dm, cocc = dm_new, cocc_new
    return led.finish("host_parts_ms", ("transfers", "fock", "diis", "eigen", "density_energies"), "host parts")


def _run_scf_device(inp, backend, functional, max_cycle, conv_e, conv_dm, log):
    """Device-resident form of the same loop: nothing but scalars crosses PCIe per cycle."""
    t, dev, nocc, sync = backend.torch, backend.dev, inp.nocc, backend.replica_sync
    f64, root = t.float64, backend.rank == 0 or sync is None
    H = t.as_tensor(inp.Hcore, dtype=f64, device=dev)
    S = t.as_tensor(inp.S, dtype=f64, device=dev)
    eigh_full = backend.eigh.solve_device                                              # X^T F X and X C' on the device at every size
    sqrt2 = float(np.sqrt(2.0))
    rotate, last_ddm = backend.occ_solver is not None, None

    def eigh_occ(F):                                                                   # dft.py:181,227 on the device
        if rotate:
            e, co = backend.occ_solver.occupied(F, last_ddm)
            return e, co * sqrt2
        e, C = eigh_full(F)
        return e, C[:, :nocc] * sqrt2

    def checked():
        e_x, C_x = eigh_full(F)
        return e_x, float(t.linalg.norm(2.0 * C_x[:, :nocc] @ C_x[:, :nocc].T - dm_new))

    e, cocc = eigh_occ(H)
    dm = cocc @ cocc.T
    if sync:
        sync.broadcast([dm, cocc])
    diis = CDIIS(device=dev)
    led = _CycleLedger(inp, functional, conv_e, conv_dm, log)
    c_hf, want_k, prof = led.c_hf, led.want_k, led.prof
    scal = t.zeros(4, dtype=f64, device=dev)
    for _ in range(max_cycle):
        t_it = led.start()
        backend.d_dm.copy_(dm); backend.d_cocc.copy_(cocc)                             # device to device
        E_xc, t_xc = backend._device_parts(want_k)
        t.cuda.synchronize()
        led.xc_times.append(t_xc); led.jk_times.append(time.time() - t_it - t_xc)
        J, K, V = backend.d_J, backend.d_K, backend.d_v
        if root:
            tp = [time.time()]
            mark = (lambda: (t.cuda.synchronize(), tp.append(time.time()))) if prof is not None else (lambda: None)
            F = H + J + 0.5 * (V + V.T)                                                # dft.py:212,223
            if want_k:
                F = F - (0.5 * c_hf) * K                                               # dft.py:221
            mark()
            F = diis.update(S, dm, F, keep_on_device=True, cocc=cocc)
            mark()
            e, cocc_new = eigh_occ(F)
            mark()
            dm_new = cocc_new @ cocc_new.T
            dv = dm_new.reshape(-1)
            tr = backend._down.view(3, -1) @ dv                # [J:D, K:D, Vraw:D] in one launch (J, K, V are its rows)
            scal = t.stack([t.dot(dv, H.reshape(-1)), 0.5 * tr[0], (-0.25 * c_hf if want_k else 0.0) * tr[1],
                            t.linalg.norm(dm_new - dm)])
            mark()
            if prof is not None and len(tp) == 5:
                prof.append([1e3 * (b - a) for a, b in zip(tp, tp[1:])])
        else:
            dm_new, cocc_new = t.empty_like(dm), t.empty_like(cocc)
        if sync:
            sync.broadcast([dm_new, cocc_new, scal])
        E_one, E_coul, E_ex, last_ddm = scal.tolist()                                  # the cycle's only download
        if led.cycle(E_one, E_coul, E_xc, E_ex, last_ddm):
            ok, e_x = _aufbau_check(checked, root, t.ones(1, dtype=f64, device=dev), sync and sync.broadcast, log) if rotate else (True, None)
            e = e if e_x is None else e_x
            if ok:
                led.res["converged"] = True
                dm = dm_new
                break
            rotate = False
            diis = CDIIS(device=dev)
        dm, cocc = dm_new, cocc_new
    led.res["dm"] = dm.cpu().numpy()
    led.res["mo_energy"] = _host(e)
    return led.finish("device_parts_ms", ("fock", "diis", "eigen", "density_energies"), "device-resident parts")


def _run_scf_fused(inp, backend, functional, max_cycle, conv_e, conv_dm, log):
    """The loop with its host part on the device (scf_tail.ScfTail): per cycle the J / K and XC kernels, then the tail's
    launches for dft.py:212-236, then ONE wait on host-mapped memory for the energy / convergence scalars.  The few full
    diagonalisations of a run (first cycle, refused rotations, the final aufbau check) go through the backend's
    FockDiagonaliser, as in the other two loops.  With several ranks the cycle's device work is the sharded
    one (grid_shard.ShardedFock: local sweep + local J/K + one all-reduce), rank 0 alone runs the tail, and
    [dm | cocc | scalars] reach the other ranks in one broadcast."""
    t = backend.torch
    tail, rot_stats = backend.tail, backend.occ_solver.stats
    root, sync, world = backend.rank == 0, backend.replica_sync, backend.world
    nocc = inp.nocc
    sqrt2 = float(np.sqrt(2.0))

    def full_solve(F_dev):                                                             # dft.py:181,227: (energies, eigenvectors on the device)
        e_, U = backend.eigh.solve_device(F_dev, products="host")                      # where LAPACK solves, this loop forms X^T F X and X C' on the host
        return _host(e_), U

    def diagonalise_into_basis(F_dev):
        e_, U = full_solve(F_dev)
        tail.basis.copy_(U)
        rot_stats["exact"] += 1
        return e_

    def checked():
        e_x, C_x = full_solve(tail.fock)
        return e_x, float(t.linalg.norm(2.0 * C_x[:, :nocc] @ C_x[:, :nocc].T - backend.d_dm))

    e = None
    if root:
        tail.reset()
        e = diagonalise_into_basis(tail.d_h)
        backend.d_cocc.copy_(sqrt2 * tail.basis[:, :nocc]); backend.d_dm.copy_(backend.d_cocc @ backend.d_cocc.T)   # dft.py:182
    scal = t.zeros(8, dtype=t.float64, device=backend.dev)                           # what travels with [dm | cocc] when there are replicas
    if sync:
        sync.broadcast([backend._up])                                                  # [dm | cocc] is one flat buffer (HipBackend)
    led = _CycleLedger(inp, functional, conv_e, conv_dm, log)
    res, c_hf, want_k, xc_times, jk_times = led.res, led.c_hf, led.want_k, led.xc_times, led.jk_times
    rotate, last_ddm = True, None
    d_K = backend.d_K if want_k else None
    marks, tail_log = [], []      # (start, J/K done, XC done) events; (status, fixed-point steps, Jacobi sweeps, continued, queued ahead)
    sol = backend.solver
    pool = [t.cuda.Event(enable_timing=True) for _ in range(3 * 40)] if world == 1 else []   # made here: not in the cycles' time
    # One rank: the next cycle's J/K and sweep are queued BEHIND this cycle's tail before the host has seen its result -- they only
    # need dm / cocc, which the tail leaves in place -- so the GPU never waits for the host between cycles (30 us of a 0.65 ms
    # Benzene cycle).  Two sets of [J | K | Vxc] in turn: a cycle whose rotation is refused after all still owns intact matrices
    # for DFT_ScfTailFinish, and the parts queued ahead of it (from the density that was not replaced) are simply queued again.
    # The same holds when the step needed more fixed-point steps than it queued (memory-resident rotation, status 3): the step
    # leaves dm / cocc alone and DFT_ScfTailMore writes them after the parts queued ahead have read the old ones.  Each set has
    # its own Exc scalar: a continuation reads its cycle's Exc after the sweep queued ahead has run.
    ahead = world == 1 and backend.prequeue
    n2 = backend.nao * backend.nao
    sets = [(backend.d_J, backend.d_K, backend.d_v)]
    d_excs = [t.zeros(1, dtype=t.float64, device=backend.dev) for _ in range(2)]
    if world == 1:
        spare = t.zeros_like(backend._down)
        sets.append(tuple(spare[k * n2:(k + 1) * n2].view(backend.nao, backend.nao) for k in range(3)))

    def enqueue_parts(k):
        backend.d_J, backend.d_K, backend.d_v = sets[k % 2]
        d_exc = d_excs[k % 2]
        ev = pool[3 * len(marks):3 * len(marks) + 3] if 3 * len(marks) + 3 <= len(pool) else [t.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        backend._jk_device(want_k)
        ev[1].record()
        if backend.xc_occ:
            sol.compute_xc_occ_async(backend.ngrid, backend.nao, nocc, backend.d_cocc, backend.d_ao, backend.d_w, backend.d_v, d_exc,
                                     backend.d_gr, backend.d_dm)
        else:
            sol.compute_xc_async(backend.ngrid, backend.nao, backend.d_dm, backend.d_ao, backend.d_w, backend.d_v, d_exc, backend.d_gr)
        ev[2].record()
        marks.append(ev)

    queued, last_status = -1, None
    for cycle in range(max_cycle):
        t_it = led.start()
        if world == 1:
            if queued < cycle:
                enqueue_parts(cycle); queued = cycle
            d_J, d_Kc, d_V = sets[cycle % 2]
            d_K = d_Kc if want_k else None
            E_xc = None
        else:
            d_J, d_V = backend.d_J, backend.d_v
            E_xc, t_xc = backend._device_parts(want_k)                                 # sharded: ends in the all-reduce of [Vxc | J | K | Exc]
            xc_times.append(t_xc); jk_times.append(time.time() - t_it - t_xc)
        if root:
            tol = _rotation_tol(last_ddm)
            tail.step(rotate, c_hf, tol, d_J, d_K, d_V, backend.d_dm, backend.d_cocc, d_exc=d_excs[cycle % 2] if world == 1 else None)
            if ahead and last_status == 0 and rotate:                                  # the last rotation went through: expect this one to
                enqueue_parts(cycle + 1); queued = cycle + 1
            E_one, E_coul, E_ex, ddm, status, steps, sweeps, exc_dev = tail.wait()
            tail_log.append((status, steps, sweeps, tail.continued, queued > cycle))
            last_status = status
            if (status != 0 or tail.continued) and queued > cycle:                     # queued ahead from the density the step started from:
                queued = cycle; marks.pop()                                            # not this cycle's successor
            if status == 2:                                                            # singular Pulay system: least squares on the host
                tail.step(rotate, c_hf, tol, d_J, d_K, d_V, backend.d_dm, backend.d_cocc,
                          coef=tail.pulay_coefficients_on_host(), repeat=True)
                E_one, E_coul, E_ex, ddm, status, steps, _, _ = tail.wait()
            if status == 1:                                                            # no rotation (asked for, or possible): full solve
                e = diagonalise_into_basis(tail.fock)
                tail.finish(c_hf, d_J, d_K, backend.d_dm, backend.d_cocc)
                E_one, E_coul, E_ex, ddm, status, _, _, _ = tail.wait()
            else:
                rot_stats["rotated"] += 1; rot_stats["inner_steps"] += steps
            if status != 0:
                raise RuntimeError(f"SCF tail: status {status}")
            if world == 1:
                E_xc = exc_dev
        if sync:
            if root:
                scal[:4] = t.tensor([E_one, E_coul, E_ex, ddm], dtype=t.float64)
            sync.broadcast([backend._up, scal])
            E_one, E_coul, E_ex, ddm = scal[:4].tolist()
        last_ddm = ddm
        if led.cycle(E_one, E_coul, E_xc, E_ex, ddm):
            flag = t.ones(1, dtype=t.float64, device=backend.dev)
            ok, e_x = _aufbau_check(checked, root, flag, sync and sync.broadcast, log) if rotate else (True, None)
            e = e if e_x is None else e_x
            if ok:
                res["converged"] = True
                break
            rotate = False
            if root:
                tail.reset()
    backend.d_J, backend.d_K, backend.d_v = sets[0]
    res["dm"] = backend.d_dm.cpu().numpy()                                             # (waits for anything still queued ahead)
    res["mo_energy"] = None if e is None else np.asarray(e)
    res["loop"] = "fused"
    res["tail_log"] = tail_log
    for ev in marks:                                                                   # device-side durations: nothing waited in between
        jk_times.append(1e-3 * ev[0].elapsed_time(ev[1])); xc_times.append(1e-3 * ev[1].elapsed_time(ev[2]))
    return led.finish()


def _blockdiag(a, b):
    n = a.shape[0]
    out = np.zeros((2 * n, 2 * n))
    out[:n, :n], out[n:, n:] = a, b
    return out


def spin_square(S, cocc_a, cocc_b):
    """<S^2> of a single determinant: Sz (Sz + 1) + N_beta - |C_a,occ^T S C_b,occ|_F^2."""
    na, nb = cocc_a.shape[1], cocc_b.shape[1]
    sz = 0.5 * (na - nb)
    return sz * (sz + 1.0) + nb - float(np.sum((cocc_a.T @ S @ cocc_b) ** 2))


def run_uks(inp, backend, functional, max_cycle=200, conv_e=1e-8, conv_dm=1e-6, log=print, meta=False):
    """Unrestricted Kohn-Sham loop on the host, for inp.nalpha / inp.nbeta electrons of the two spins (inputs.build(...,
    charge, spin)).  `backend.uks_parts(dm_a, dm_b, cocc_a, cocc_b, want_k)` supplies (J[D_a + D_b], K[D_a], K[D_b], Exc,
    V_a, V_b) with the potentials in the library's convention (HipBackend on the device; the tests have a numpy one).

        F_s = Hcore + J[D_a + D_b] + (V_s + V_s^T)/2 - c_hf K[D_s],        D_s = C_s,occ C_s,occ^T
        E   = tr(D Hcore) + 1/2 tr(D J) - 1/2 c_hf sum_s tr(D_s K[D_s]) + Exc + E_nuc,    D = D_a + D_b

    The loop keeps run_scf's contract: core guess eigh(Hcore, S) for both spins (at spin = 0 the two stay equal: no
    broken-symmetry guess), one DIIS with common coefficients over both spins' error vectors (CDIIS as it stands, on the
    block-diagonal matrices diag(F_a, F_b), diag(D_a, D_b), diag(S, S): the commutator of block-diagonal matrices holds
    both errors, their Gram matrix is the sum), eigh(F_s, S) per spin, energies from the NEW densities with J / K / Exc of
    the old ones, convergence |dE| < conv_e and |dD_a| + |dD_b| (Frobenius) < conv_dm.  With nalpha = nbeta the loop is
    run_scf's host loop term by term.  Returns run_scf's fields with dm the total density, and dm_a, dm_b, mo_energy_a,
    mo_energy_b, mo_coeff_a, mo_coeff_b, s_squared (spin_square), nalpha, nbeta, uks = True.

    meta=True (the driver's --open-shell-meta): the functional is a meta-GGA and the parts come from
    `backend.uks_meta_parts`, same arguments and same tuple (HipBackend: DFT_ComputeXCMetaSpin); the loop itself is the
    same.  Without it a meta-GGA is refused, as before the open-shell meta-GGA sweep existed."""
    if meta:
        if not functionals.resolve(functional).needs_tau:
            raise ValueError(f"run_uks(meta=True) is for a meta-GGA: {functional} carries no tpss_x / tpss_c weight; run it with meta=False")
        if not callable(getattr(backend, "uks_meta_parts", None)):
            raise ValueError(f"run_uks(meta=True): the backend ({type(backend).__name__}) has no uks_meta_parts, the open-shell meta-GGA "
                             "sweep (HipBackend has one; the tests have a numpy one)")
        parts = backend.uks_meta_parts
    else:
        functionals.refuse_meta(functional, "open-shell DFT (run_uks)", functionals.OPEN_SHELL_META_HINT)
        parts = backend.uks_parts
    from .hostinfo import blas_threads
    Hcore, S = inp.Hcore, inp.S
    na = int(getattr(inp, "nalpha", None) if getattr(inp, "nalpha", None) is not None else inp.nocc)
    nb = int(getattr(inp, "nbeta", None) if getattr(inp, "nbeta", None) is not None else inp.nocc)
    if na < nb or nb < 0 or na <= 0 or na > S.shape[0]:
        raise ValueError(f"run_uks: nalpha = {na}, nbeta = {nb} do not fit {S.shape[0]} basis functions (nalpha >= nbeta >= 0)")
    S2 = _blockdiag(S, S)
    with blas_threads(1 if S.shape[0] < _HIPSOLVER_FROM else None):
        C0 = eigh(Hcore, S)[1]
        cocc = [np.ascontiguousarray(C0[:, :na]), np.ascontiguousarray(C0[:, :nb])]
        dm = [c @ c.T for c in cocc]
        diis = CDIIS()
        led = _CycleLedger(inp, functional, conv_e, conv_dm, log, uks=True, nalpha=na, nbeta=nb)
        c_hf, want_k = led.c_hf, led.want_k
        for _ in range(max_cycle):
            t_it = led.start()
            J, Ka, Kb, E_xc, Va, Vb = parts(dm[0], dm[1], cocc[0], cocc[1], want_k)
            led.xc_times.append(time.time() - t_it); led.jk_times.append(0.0)        # one bracket: the parts are not timed apart here
            F = [Hcore + J + 0.5 * (V + V.T) - (c_hf * K if K is not None else 0.0) for V, K in ((Va, Ka), (Vb, Kb))]
            Fx = diis.update(S2, _blockdiag(dm[0], dm[1]), _blockdiag(F[0], F[1]))
            n = S.shape[0]
            ea, Ca = eigh(Fx[:n, :n], S)
            eb, Cb = eigh(Fx[n:, n:], S)
            cocc_new = [np.ascontiguousarray(Ca[:, :na]), np.ascontiguousarray(Cb[:, :nb])]
            dm_new = [c @ c.T for c in cocc_new]
            D = dm_new[0] + dm_new[1]
            E_one, E_coul = float(np.sum(D * Hcore)), 0.5 * float(np.sum(D * J))
            E_ex = -0.5 * c_hf * float(np.sum(dm_new[0] * Ka) + np.sum(dm_new[1] * Kb)) if want_k else 0.0
            ddm = float(np.linalg.norm(dm_new[0] - dm[0]) + np.linalg.norm(dm_new[1] - dm[1]))
            done = led.cycle(E_one, E_coul, E_xc, E_ex, ddm, dm=D, dm_a=dm_new[0], dm_b=dm_new[1], mo_energy_a=ea, mo_energy_b=eb,
                             mo_coeff_a=Ca, mo_coeff_b=Cb, mo_energy=ea, s_squared=spin_square(S, cocc_new[0], cocc_new[1]))
            dm, cocc = dm_new, cocc_new
            if done:
                led.res["converged"] = True
                break
        return led.finish()
