"""CPU backend for scf.run_uks (TEST INFRASTRUCTURE: lives under tests/): J and K from the dense ERI in numpy, Exc and the
two potentials from response.xc_spin_host on the oracle's AO planes.  A functional without a density-functional
component (triplet_reference.HF: exact exchange alone) skips the sweep."""
import numpy as np

import oracle
from quantum_compute_dft_amd import functionals, response


class UksHostBackend:
    def __init__(self, inp, functional):
        if inp.eri is None:
            raise ValueError("UksHostBackend needs the dense ERI")
        self.inp, self.functional = inp, functional
        f = functionals.resolve(functional)
        self.sweep = bool(f.weights)
        self.ao = self.gr = None
        if self.sweep:
            self.ao, gr = oracle.eval_ao(inp.shells, inp.grids.coords, deriv=1)
            self.gr = gr if f.needs_gradient else None

    def uks_parts(self, dm_a, dm_b, cocc_a, cocc_b, want_k):
        eri = self.inp.eri
        J = np.einsum("ijkl,kl->ij", eri, dm_a + dm_b)
        Ka = np.einsum("ikjl,kl->ij", eri, dm_a) if want_k else None
        Kb = np.einsum("ikjl,kl->ij", eri, dm_b) if want_k else None
        if not self.sweep:
            z = np.zeros_like(J)
            return J, Ka, Kb, 0.0, z, z
        exc, va, vb = response.xc_spin_host(self.functional, dm_a, dm_b, self.ao, self.inp.grids.weights, self.gr)
        return J, Ka, Kb, exc, va, vb

    def fock(self, dm_a, dm_b, c_hf):
        """(F_alpha, F_beta) of the densities, as run_uks assembles them."""
        J, Ka, Kb, _, va, vb = self.uks_parts(dm_a, dm_b, None, None, c_hf != 0.0)
        return [self.inp.Hcore + J + 0.5 * (v + v.T) - (c_hf * k if k is not None else 0.0) for v, k in ((va, Ka), (vb, Kb))]
