"""Independent reference for the Becke weight gradient: the cell function restated in torch with the points tied to their
owners, coords = R[own] + t, and differentiated by autograd.  It shares no derivative code with
grid_gen.becke_weight_gradient_host or the kernel.  The distances are written out (no cdist) and guarded: sqrt is not
differentiated at 0 (a point on a nucleus, the diagonal of the atom-atom table), where its derivative would be inf * 0."""
import numpy as np
import torch

from quantum_compute_dft_amd import grid_gen


def _norm(v):
    """|v| along the last axis; exactly 0 with a zero gradient where v = 0."""
    r2 = (v * v).sum(dim=-1)
    pos = r2 > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, r2, torch.ones_like(r2))), torch.zeros_like(r2))


def cell_function(R, t, own, charges):
    """cell_g (ngrid,) as a differentiable function of the atom positions R (natm, 3); t (ngrid, 3) the fixed offsets of
    the points from their owners."""
    natm = R.shape[0]
    rad = torch.sqrt(torch.as_tensor(grid_gen.bragg_radii_bohr(charges), dtype=torch.float64)) + 1e-200
    rr = rad[:, None] / rad[None, :]
    a = (0.25 * (rr.T - rr)).clamp(-0.5, 0.5)
    eye = torch.eye(natm, dtype=torch.bool)
    Rij = torch.where(eye, torch.ones((natm, natm), dtype=torch.float64), _norm(R[:, None, :] - R[None, :, :]))
    r = R[own] + t
    d = _norm(r[:, None, :] - R[None, :, :])
    mu = (d[:, :, None] - d[:, None, :]) / Rij[None]
    g = mu + a[None] * (1 - mu * mu)
    for _ in range(3):
        g = (3 - g * g) * g * 0.5
    s = torch.where(eye[None], torch.ones_like(g), 0.5 * (1 - g))
    p = s.prod(dim=2)
    return p.gather(1, own[:, None])[:, 0] / p.sum(dim=1)


def becke_weight_gradient_autograd(coords, owner, atom_xyz, charges, f, block=4096):
    """(natm, 3) = d/dR sum_g f_g cell_g(R) with the points moving with their owners, and cell (ngrid,)."""
    R0 = torch.as_tensor(np.asarray(atom_xyz, dtype=np.float64)).reshape(-1, 3)
    own = torch.as_tensor(np.asarray(owner).astype(np.int64))
    c = torch.as_tensor(np.asarray(coords, dtype=np.float64)).reshape(-1, 3)
    t = c - R0[own]
    fw = torch.as_tensor(np.asarray(f, dtype=np.float64))
    out = torch.zeros_like(R0)
    cells = []
    for lo in range(0, c.shape[0], block):
        R = R0.clone().requires_grad_(True)
        cell = cell_function(R, t[lo:lo + block], own[lo:lo + block], charges)
        (fw[lo:lo + block] * cell).sum().backward()
        out += R.grad
        cells.append(cell.detach())
    return out.numpy(), torch.cat(cells).numpy()
