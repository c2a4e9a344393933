"""Properties of a converged density.  Electrostatic potential and electric field at arbitrary points and the forces on
the external point charges of an embedded run, on the device where one is in use (csrc/point_coulomb.hip through
integrals.point_coulomb / integrals.point_field); the dipole moment from the host dipole integrals."""
import numpy as np

from . import basis, integrals


DEBYE_PER_AU = 2.541746473   # 1 e bohr in debye (CODATA 2018)


def dipole_moment(inp, dm, origin=(0.0, 0.0, 0.0), debye=False):
    """mu_k = sum_A Z_A (R_A - origin)_k - tr(dm D_k), D = integrals.dipole(shells, origin): (3,) in e bohr, or in debye.
    Independent of the origin for a neutral molecule.  For a variational functional (option quirks = 0) and a
    converged density mu = -dE/dF of a run in the uniform field F (inputs.build(..., efield=F))."""
    o = np.asarray(origin, dtype=np.float64).reshape(3)
    z = np.array([basis.atomic_number(s) for s in inp.symbols], dtype=np.float64)
    D = integrals.dipole(inp.shells, o)
    mu = z @ (np.asarray(inp.atom_xyz, dtype=np.float64) - o) - np.einsum("kij,ji->k", D, np.asarray(dm, dtype=np.float64))
    return mu * DEBYE_PER_AU if debye else mu


def electrostatic_potential(inp, dm, points, device="cpu", electronic_only=False):
    """V(r) = sum_A Z_A / |r - R_A| - int rho(r') / |r - r'| dr' in atomic units at `points` (n, 3) bohr, for the density
    matrix `dm` of the molecule of `inp` (inputs.build).  The potential of the MOLECULE: external point charges of an
    embedded run are not included (add sum_c q_c / |r - R_c| for the total).  `electronic_only`: the second term alone
    (negative).  ValueError for a point within 1e-8 bohr of a nucleus (not checked with electronic_only)."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points: expected an (n, 3) array in bohr, got shape {pts.shape}")
    u = integrals.point_coulomb(inp.shells, pts, dm=np.asarray(dm, dtype=np.float64), device=device)
    if electronic_only:
        return -u
    z = np.array([basis.atomic_number(s) for s in inp.symbols], dtype=np.float64)
    dist = np.linalg.norm(pts[:, None, :] - np.asarray(inp.atom_xyz, dtype=np.float64)[None, :, :], axis=2)      # (n, natm)
    if dist.size and dist.min() < 1e-8:
        c, a = np.unravel_index(np.argmin(dist), dist.shape)
        raise ValueError(f"point {c} sits on nucleus {a} ({inp.symbols[a]}): the nuclear potential is singular there")
    return (z[None, :] / dist).sum(axis=1) - u


def electric_field(inp, dm, points, device="cpu", electronic_only=False):
    """E(r) = sum_A Z_A (r - R_A) / |r - R_A|^3 + G(r) in atomic units (Ha / (e bohr)) at `points` (n, 3) bohr: (n, 3),
    minus the gradient of electrostatic_potential.  G[c, k] = sum_{mu nu} dm[mu, nu] d<mu| 1/|r - R| |nu> / dR_k at
    R = points[c] is the electronic part (integrals.point_field; exact, the basis does not move with the point).  The
    field of the MOLECULE: external point charges of an embedded run are not included.  `electronic_only`: G alone.
    ValueError for a point within 1e-8 bohr of a nucleus (not checked with electronic_only)."""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points: expected an (n, 3) array in bohr, got shape {pts.shape}")
    G = integrals.point_field(inp.shells, pts, np.asarray(dm, dtype=np.float64), device=device)
    if electronic_only:
        return G
    z = np.array([basis.atomic_number(s) for s in inp.symbols], dtype=np.float64)
    d = pts[:, None, :] - np.asarray(inp.atom_xyz, dtype=np.float64)[None, :, :]                                  # (n, natm, 3)
    dist = np.linalg.norm(d, axis=2)
    if dist.size and dist.min() < 1e-8:
        c, a = np.unravel_index(np.argmin(dist), dist.shape)
        raise ValueError(f"point {c} sits on nucleus {a} ({inp.symbols[a]}): the nuclear potential is singular there")
    return (z[None, :, None] * d / dist[:, :, None] ** 3).sum(axis=1) + G


def point_charge_forces(inp, dm, device="cpu"):
    """F_c = q_c E(R_c) in Ha / bohr, (ncharges, 3): the force the molecule (nuclei and the density `dm`) exerts on every
    external point charge of `inp` (inputs.build(..., point_charges=...)), E = electric_field.  For a converged density
    -F_c is the derivative of the total energy with respect to R_c (Hellmann-Feynman: no basis function moves with a
    charge).  The forces of the charges on each other are NOT included, just as their mutual energy is not part of
    inp.E_nuc.  ValueError if `inp` has no point charges."""
    pc = getattr(inp, "point_charges", None)
    if pc is None or len(pc) == 0:
        raise ValueError("point_charge_forces: the inputs were built without point charges")
    return pc[:, 3:4] * electric_field(inp, dm, pc[:, :3], device=device)
