"""CPU backend for scf.run_uks(meta=True) (TEST INFRASTRUCTURE: lives under tests/): the oracle's AO planes, the oracle's J and
K from the dense ERI, Exc and the two potentials from metagga.xc_meta_spin_host.  Serves any functional, with or without
meta components (uks_meta_parts only: it has no uks_parts)."""
import numpy as np

import oracle
from quantum_compute_dft_amd import functionals, metagga


class UksMetaHostBackend:
    def __init__(self, inp, functional):
        if inp.eri is None:
            raise ValueError("UksMetaHostBackend needs the dense ERI")
        self.inp, self.functional = inp, functional
        self.f = functionals.resolve(functional)
        self.ao, self.gr = oracle.eval_ao(inp.shells, inp.grids.coords, deriv=1)

    def uks_meta_parts(self, dm_a, dm_b, cocc_a, cocc_b, want_k):
        eri = self.inp.eri
        dm_a, dm_b = np.ascontiguousarray(dm_a), np.ascontiguousarray(dm_b)
        J = oracle.coulomb(eri, np.ascontiguousarray(dm_a + dm_b))
        Ka = oracle.exchange(eri, dm_a) if want_k else None
        Kb = oracle.exchange(eri, dm_b) if want_k else None
        w8, w2 = self.f.weight_vector(), self.f.meta_weight_vector()
        exc, va, vb = metagga.xc_meta_spin_host((w8, w2), dm_a, dm_b, self.ao, self.inp.grids.weights, self.gr)
        return J, Ka, Kb, exc, va, vb

    def energy(self, cocc_a, cocc_b):
        """E_tot of the determinant of the occupied orbitals cocc_s (nao, n_s), orthonormal in S, as run_uks sums it."""
        inp, c_hf = self.inp, self.f.c_hf
        dm_a, dm_b = cocc_a @ cocc_a.T, cocc_b @ cocc_b.T
        J, Ka, Kb, exc, _, _ = self.uks_meta_parts(dm_a, dm_b, cocc_a, cocc_b, c_hf != 0.0)
        D = dm_a + dm_b
        e = float(np.sum(D * inp.Hcore)) + 0.5 * float(np.sum(D * J)) + exc + inp.E_nuc
        if c_hf != 0.0:
            e -= 0.5 * c_hf * float(np.sum(dm_a * Ka) + np.sum(dm_b * Kb))
        return e

    def fock(self, dm_a, dm_b):
        """(F_alpha, F_beta) of the densities, as run_uks assembles them."""
        c_hf = self.f.c_hf
        J, Ka, Kb, _, va, vb = self.uks_meta_parts(dm_a, dm_b, None, None, c_hf != 0.0)
        return [self.inp.Hcore + J + 0.5 * (v + v.T) - (c_hf * k if k is not None else 0.0) for v, k in ((va, Ka), (vb, Kb))]
