"""Input builder: counterpart of the reference's grid.py (`build`, `get_ao_grad`, grid.py:23-67)
without PySCF: molecule + basis -> shell table, level-3 Becke/Lebedev grid, S, T, V, dense ERI,
E_nuc, electron count.  AO values / gradients are NOT built here: the driver evaluates them on the
device with DFT_EvalAO (grid.py:30,38 did it on the CPU and dft.py:155,172 uploaded them)."""
import os
from dataclasses import dataclass

import numpy as np

from . import basis, grid_gen, integrals

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


@dataclass
class SCFInputs:
    symbols: list
    atom_xyz: np.ndarray   # bohr
    shells: basis.ShellTable
    grids: grid_gen.Grids
    S: np.ndarray
    T: np.ndarray
    V: np.ndarray
    Hcore: np.ndarray
    eri: np.ndarray        # (nao, nao, nao, nao), or None when only Cholesky vectors were built
    E_nuc: float
    nocc: int
    nelec: int
    chol: np.ndarray = None  # (naux, nao, nao) Cholesky vectors of the ERI (eri_mode='cholesky')
    chol_range: tuple = None  # (lo, hi, naux): `chol` is only THIS rank's slice of the naux vectors (build(..., world > 1))
    point_charges: np.ndarray = None  # (n, 4): x, y, z (bohr), q of the external point charges (build(..., point_charges=...))
    V_ext: np.ndarray = None  # (nao, nao) potential of those charges on the electrons, already part of Hcore
    E_nuc_ext: float = 0.0    # nuclei -- external charges repulsion, already part of E_nuc
    efield: np.ndarray = None  # (3,) uniform external electric field F in a.u. (build(..., efield=...)), already part of Hcore and E_nuc
    nalpha: int = None   # electrons of the two spins (build(..., charge, spin)); None: nocc each, the closed shell
    nbeta: int = None
    charge: int = 0
    spin: int = 0        # nalpha - nbeta


def external_charges(symbols, atom_xyz, shells, point_charges, device="cpu"):
    """(charges (n, 4), V_ext, E_nuc_ext) of external point charges x, y, z (bohr), q:
         V_ext[mu, nu] = -sum_c q_c <mu| 1/|r - R_c| |nu>      E_nuc_ext = sum_{A, c} Z_A q_c / |R_A - R_c|
    The interaction of the charges among themselves is NOT included (a constant of the environment, not of the
    molecule).  ValueError when a charge sits within 1e-8 bohr of a nucleus."""
    pc = np.array(point_charges, dtype=np.float64)
    if pc.ndim != 2 or pc.shape[1] != 4:
        raise ValueError(f"point_charges: expected an (n, 4) array of x, y, z (bohr), q; got shape {pc.shape}")
    xyz = np.asarray(atom_xyz, dtype=np.float64)
    z = np.array([basis.atomic_number(s) for s in symbols], dtype=np.float64)
    dist = np.linalg.norm(xyz[:, None, :] - pc[None, :, :3], axis=2)              # (natm, n)
    if dist.size and dist.min() < 1e-8:
        a, c = np.unravel_index(np.argmin(dist), dist.shape)
        raise ValueError(f"point charge {c} sits on nucleus {a} ({symbols[a]}): |R_A - R_c| = {dist[a, c]:.1e} bohr")
    V_ext = -integrals.point_coulomb(shells, pc[:, :3], weights=pc[:, 3], device=device)
    return pc, V_ext, float(np.sum(z[:, None] * pc[None, :, 3] / dist))


def uniform_field(symbols, atom_xyz, shells, efield):
    """(F (3,), V_F, E_nuc_F) of a uniform electric field F (a.u.):  V_F = sum_k F_k D_k (the electrons' energy +F.r, D the
    dipole integrals about the origin of the coordinates),  E_nuc_F = -sum_A Z_A F.R_A.  The total energy then carries
    -F.mu, so that mu = -dE/dF (properties.dipole_moment) for a variational functional."""
    F = np.array(efield, dtype=np.float64)
    if F.shape != (3,) or not np.all(np.isfinite(F)):
        raise ValueError(f"efield: expected three finite numbers Fx, Fy, Fz (a.u.), got {efield!r}")
    z = np.array([basis.atomic_number(s) for s in symbols], dtype=np.float64)
    V_F = np.einsum("k,kij->ij", F, integrals.dipole(shells))
    return F, V_F, -float(z @ (np.asarray(atom_xyz, dtype=np.float64) @ F))


def build(atom_path, basis_name="sto-3g", grid_level=3, device="cpu", verbose=True, eri_mode="dense",
          chol_tol=1e-9, rank=0, world=1, group=None, point_charges=None, efield=None, charge=0, spin=0, atom_xyz=None):
    """grid.py:42-67.  `atom_path`: an .xyz file (or a molecule name resolved in data/).
    eri_mode "dense": the (nao^4) tensor of grid.py:65; "cholesky": pivoted Cholesky vectors only.
    world > 1 (torch.distributed initialised): the Cholesky factorisation -- the one expensive step, host integral columns
    + device algebra -- runs on rank 0 ALONE, on the whole node's CPU allowance while the other ranks wait, and every
    rank receives only its slice of the vectors (grid_shard.scatter_vectors); `chol_range` records the slice.
    point_charges: (n, 4) x, y, z (bohr), q -- electrostatic embedding (external_charges): Hcore = T + V + V_ext and E_nuc
    gains the nuclei--charges repulsion, so every SCF loop runs in the field of the charges unchanged; their interaction
    among themselves is not included.  Every rank computes V_ext itself (deterministic: nothing is broadcast).
    efield: (Fx, Fy, Fz) in a.u. -- a uniform external electric field (uniform_field): Hcore gains sum_k F_k D_k and E_nuc
    -sum_A Z_A F.R_A, so every SCF loop, the fused tail included, runs in the field with no other change.
    charge, spin: the molecule's charge and nalpha - nbeta (scf.run_uks); the defaults are the neutral closed shell.
    nelec = sum Z - charge, nalpha = (nelec + spin) / 2, nbeta = (nelec - spin) / 2, nocc = nbeta; ValueError when spin is
    negative, exceeds the electron count or has not its parity (an odd count needs --spin), or no electron is left.
    atom_xyz: (natm, 3) coordinates in bohr that replace the file's (the elements and their order stay the file's): what a
    geometry optimisation and a finite-difference gradient rebuild the inputs with."""
    if not os.path.exists(atom_path):
        cand = os.path.join(DATA_DIR, atom_path if atom_path.endswith(".xyz") else atom_path + ".xyz")
        if os.path.exists(cand):
            atom_path = cand
    symbols, xyz = basis.parse_xyz(atom_path)
    if atom_xyz is not None:
        new = np.array(atom_xyz, dtype=np.float64)
        if new.shape != xyz.shape or not np.all(np.isfinite(new)):
            raise ValueError(f"atom_xyz: expected finite coordinates of shape {xyz.shape} (bohr), got shape {new.shape}")
        xyz = new
    shells = basis.build_shells(symbols, xyz, basis_name)
    charge, spin = int(charge), int(spin)
    nelec = sum(basis.atomic_number(s) for s in symbols) - charge
    if nelec <= 0:
        raise ValueError(f"charge {charge} leaves no electrons ({nelec})")
    if spin < 0 or spin > nelec:
        raise ValueError(f"spin (nalpha - nbeta) = {spin} does not fit {nelec} electrons: expected 0 <= spin <= {nelec}")
    if (nelec - spin) % 2:
        raise ValueError(f"{nelec} electrons (charge {charge}) and spin (nalpha - nbeta) = {spin} have different parity: "
                         f"an {'odd' if nelec % 2 else 'even'} electron count needs an {'odd' if nelec % 2 else 'even'} --spin")
    nalpha, nbeta = (nelec + spin) // 2, (nelec - spin) // 2
    if nalpha > shells.nao:
        raise ValueError(f"spin {spin}: {nalpha} alpha electrons do not fit {shells.nao} basis functions")
    nocc = nbeta                     # the closed shell: nelec // 2 as ever
    if verbose:  # grid.py:54-56,60
        print(f"Number of basis functions: {shells.nao}")
        print(f"Number of electrons: {nelec}")
        print(f"Number of occupied orbitals: {nocc}")
    grids = grid_gen.Grids(symbols, xyz, level=grid_level, device=device)
    if verbose:
        print(f"Number of grid points for integration: {grids.size}")
    S, T, V = integrals.int1e(shells, symbols, xyz)
    eri = chol = chol_range = None
    if eri_mode == "dense":
        eri = integrals.int2e(shells)
    elif eri_mode == "cholesky":
        from .cholesky import cholesky_eri
        import time
        t0 = time.time()
        if world > 1:
            import torch.distributed as dist
            from .grid_shard import scatter_vectors, vector_bounds
            from .hostinfo import host_cpu_share
            full = None
            if rank == 0:
                integrals.set_threads(host_cpu_share(whole_node=True))    # the other ranks are waiting in the scatter below
                try:
                    full = cholesky_eri(shells, tol=chol_tol, device=device)
                finally:
                    integrals.set_threads(host_cpu_share())
            chol, naux = scatter_vectors(full, shells.nao, device, world, rank, group)
            del full
            chol_range = (*vector_bounds(naux, world, rank), naux)
            if not str(device).startswith("cuda"):
                chol = chol.numpy()
        else:
            chol = cholesky_eri(shells, tol=chol_tol, device=device)   # on a GPU: the factorisation's algebra and the vectors stay there
        if verbose:
            where = "integral columns (DFT_EriColumns), algebra and vectors on the device" if str(device).startswith("cuda") else "on the host"
            print(f"Cholesky vectors of the ERI: {chol.shape[0]} (threshold {chol_tol:g}, {time.time() - t0:.1f} s; {where})")
    else:
        raise ValueError(f"eri_mode {eri_mode!r}: expected 'dense' or 'cholesky'")
    if point_charges is None:
        inp = SCFInputs(symbols, xyz, shells, grids, S, T, V, T + V, eri,
                        integrals.energy_nuc(symbols, xyz), nocc, nelec, chol, chol_range)
    else:
        pc, V_ext, E_ext = external_charges(symbols, xyz, shells, point_charges, device)
        inp = SCFInputs(symbols, xyz, shells, grids, S, T, V, T + V + V_ext, eri,
                        integrals.energy_nuc(symbols, xyz) + E_ext, nocc, nelec, chol, chol_range, pc, V_ext, E_ext)
    inp.nalpha, inp.nbeta, inp.charge, inp.spin = nalpha, nbeta, charge, spin
    if efield is not None:
        F, V_F, E_F = uniform_field(symbols, xyz, shells, efield)
        inp.Hcore = inp.Hcore + V_F
        inp.E_nuc = inp.E_nuc + E_F
        inp.efield = F
    return inp
