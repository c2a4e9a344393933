"""Properties of a converged density.  Electrostatic potential at arbitrary points, on the device where one is in use
(csrc/point_coulomb.hip through integrals.point_coulomb)."""
import numpy as np

from . import basis, integrals


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
