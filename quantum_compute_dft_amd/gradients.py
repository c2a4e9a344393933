"""Analytic nuclear gradient dE/dR_A of a converged closed-shell (RKS) or unrestricted (UKS) energy, at fixed quadrature
points and weights.

    g_A = -tr(W dS/dR_A) + tr(D dT/dR_A) + tr(D dV/dR_A)           integrals.grad1e (basis centres) and the field of the
                                                                    electrons at the nucleus (integrals.point_coulomb_field)
        + d/dR_A [1/2 sum D D (ab|cd) - c_hf/4 sum D D (ab|cd)]    integrals.grad2e
        + g_A^xc                                                    DFT_ComputeXCGradient on the device, xc_gradient_host here
        + dE_nuc/dR_A  (+ the external charges' terms of an embedded run)

with W = 2 C_occ diag(eps_occ) C_occ^T = D F D / 2.  `nuclear_gradient` assembles it; the XC part has host counterparts of
DFT_EvalAOHess / DFT_ComputeXCGradient (csrc/xc_grad.hip; solver.eval_ao_hess / compute_xc_gradient,
scf.HipBackend.xc_gradient) below.  `nuclear_gradient_uks` is the same assembly for a run_uks state: W = sum_s D_s F_s D_s, the
two-electron term with the spin density beside the total one (integrals.grad2e_spin / DFT_Grad2eSpin), the XC term once
per spin (xc_gradient_spin_host / DFT_ComputeXCGradientSpin).  `nuclear_gradient(meta=True)` is the closed-shell assembly for a
meta-GGA: the same terms, the XC part with the tau term (xc_gradient_meta_host / DFT_ComputeXCGradientMeta, csrc/xc_grad_meta.hip);
`nuclear_gradient_uks(meta=True)` the open-shell one (xc_gradient_meta_spin_host / DFT_ComputeXCGradientMetaSpin,
csrc/xc_grad_meta_spin.hip).

    G[mu, x] = d/dt Exc  when, in column mu only,  ao[:, mu] -> ao[:, mu] - t ao_grad[x][:, mu]  and
               ao_grad[k][:, mu] -> ao_grad[k][:, mu] - t ao_hess[xk][:, mu]          (dm and the weights fixed)

is the derivative of Exc by the centre of basis function mu; the XC term of dE/dR_A is the sum of G[mu, :] over the
functions on atom A.  The motion of the grid points with their atoms and the derivatives of the Becke weights are not
part of it, so the term alone is not translationally invariant.

Here the coefficients c0..c3 of a point come from the functional bodies the kernels run, compiled for the host
(response.point_host), in the convention of the solver type; the rest is numpy on AO planes the caller supplies.
"""
import numpy as np

from . import basis, functionals, integrals, response

# plane index of the second derivative (x, k) in the order xx, xy, xz, yy, yz, zz
HESS_INDEX = ((0, 1, 2), (1, 3, 4), (2, 4, 5))

# Real solid harmonics of basis.py / csrc/ao_kernels.hpp as polynomials {(i, j, k): coefficient of x^i y^j z^k}
_C1 = 0.488602511902919921
_D = (1.092548430592079070, 0.315391565252520002, 0.546274215296039535)
_F = (0.590043589926643510, 2.890611442640554055, 0.457045799464465739, 0.373176332590115391, 1.445305721320277020)
_HARMONICS = {
    0: [{(0, 0, 0): 0.282094791773878143}],
    1: [{(1, 0, 0): _C1}, {(0, 1, 0): _C1}, {(0, 0, 1): _C1}],
    2: [{(1, 1, 0): _D[0]}, {(0, 1, 1): _D[0]}, {(0, 0, 2): 2 * _D[1], (2, 0, 0): -_D[1], (0, 2, 0): -_D[1]},
        {(1, 0, 1): _D[0]}, {(2, 0, 0): _D[2], (0, 2, 0): -_D[2]}],
    3: [{(2, 1, 0): 3 * _F[0], (0, 3, 0): -_F[0]},
        {(1, 1, 1): _F[1]},
        {(0, 1, 2): 4 * _F[2], (2, 1, 0): -_F[2], (0, 3, 0): -_F[2]},
        {(0, 0, 3): 2 * _F[3], (2, 0, 1): -3 * _F[3], (0, 2, 1): -3 * _F[3]},
        {(1, 0, 2): 4 * _F[2], (3, 0, 0): -_F[2], (1, 2, 0): -_F[2]},
        {(2, 0, 1): _F[4], (0, 2, 1): -_F[4]},
        {(3, 0, 0): _F[0], (1, 2, 0): -3 * _F[0]}],
}
AO_EXP_CUT = 46.0


def _poly_diff(poly, axis):
    out = {}
    for pw, c in poly.items():
        if pw[axis]:
            q = list(pw)
            q[axis] -= 1
            out[tuple(q)] = out.get(tuple(q), 0.0) + c * pw[axis]
    return out


def _poly_eval(poly, d):
    v = np.zeros(d.shape[0])
    for (i, j, k), c in poly.items():
        v += c * d[:, 0] ** i * d[:, 1] ** j * d[:, 2] ** k
    return v


def ao_hessian_host(shells, coords):
    """(6, ngrid, nao): the second derivatives xx, xy, xz, yy, yz, zz of every AO of a basis.ShellTable at coords
    (ngrid, 3), in the conventions of DFT_EvalAO (real solid harmonics, column order, primitives cut below exp(-46)).
    phi = R(r^2) S(x, y, z):  d_ij phi = R0 S_ij + R1 (x_i S_j + x_j S_i + delta_ij S) + R2 x_i x_j S."""
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    out = np.zeros((6, coords.shape[0], int(shells.nao)))
    for s in range(len(shells.l)):
        l, n, off, col = int(shells.l[s]), int(shells.nprim[s]), int(shells.off[s]), int(shells.ao[s])
        if l not in _HARMONICS:
            raise ValueError(f"shell {s}: l={l} unsupported (s-f)")
        d = coords - np.asarray(shells.xyz[s], dtype=np.float64)[None, :]
        r2 = np.einsum("gk,gk->g", d, d)
        a = np.asarray(shells.exp[off:off + n], dtype=np.float64)
        t = a[None, :] * r2[:, None]
        e = np.where(t < AO_EXP_CUT, np.asarray(shells.coef[off:off + n])[None, :] * np.exp(-np.minimum(t, AO_EXP_CUT)), 0.0)
        R0, R1, R2 = e.sum(axis=1), (-2.0 * a * e).sum(axis=1), (4.0 * a * a * e).sum(axis=1)
        for m, poly in enumerate(_HARMONICS[l]):
            S = _poly_eval(poly, d)
            d1 = [_poly_diff(poly, i) for i in range(3)]
            S1 = [_poly_eval(p, d) for p in d1]
            for i in range(3):
                for j in range(i, 3):
                    Sij = _poly_eval(_poly_diff(d1[i], j), d)
                    v = R0 * Sij + R1 * (d[:, i] * S1[j] + d[:, j] * S1[i]) + R2 * d[:, i] * d[:, j] * S
                    if i == j:
                        v = v + R1 * S
                    out[HESS_INDEX[i][j], :, col + m] = v
    return out


def _densities(functional, dms, ao, ao_grad):
    """(library type, reads sigma, ao, ao_grad, the matrices, [(rho, grad rho) of each]) for the host entries below: the
    planes as C-ordered float64, grad rho None for an LDA-class functional."""
    t, _, gga = response._kind(functional)
    if gga and ao_grad is None:
        raise ValueError("ao_grad is needed for a gradient-corrected functional")
    ao = np.ascontiguousarray(ao, dtype=np.float64)
    gr = None if ao_grad is None else np.ascontiguousarray(ao_grad, dtype=np.float64)
    dms = [np.asarray(d, dtype=np.float64) for d in dms]
    return t, gga, ao, gr, dms, [response._density(d, ao, gr if gga else None) for d in dms]


def _point_closed(functional, rho, g, weights, quirks):
    """response.point_host at a closed-shell density: sigma from grad rho (zeros for an LDA-class functional, g None)."""
    if g is None:
        g, sigma = np.zeros((rho.shape[0], 3)), np.zeros(rho.shape[0])
    else:
        sigma = np.einsum("gk,gk->g", g, g)
    return response.point_host(functional, rho, sigma, g, weights, quirks)


def _xc_contract(fac, gga, ao, gr, hs, pairs):
    """G (nao, 3) = -fac sum_s sum_g [ ao_grad[x] (Q_s D_s) + (sum_k c_sk ao_hess[xk]) (AO D_s) ][g, mu] over the pairs
    (dm_s, c_s) of a density matrix (its symmetric part counts) and its point coefficients c_s0..c_s3,
    Q_s = 2 c_s0 AO + sum_k c_sk ao_grad[k]: one pair for the closed shell, one per spin for an open-shell state."""
    G = np.zeros((ao.shape[1], 3))
    for dm, c in pairs:
        ds = 0.5 * (dm + dm.T)
        X = ao @ ds
        if not gga:
            Z = 2.0 * c[0][:, None] * X
            for x in range(3):
                G[:, x] -= fac * np.einsum("gm,gm->m", gr[x], Z)
            continue
        Q = 2.0 * c[0][:, None] * ao
        for k in range(3):
            Q += c[1 + k][:, None] * gr[k]
        Z = Q @ ds
        for x in range(3):
            H = sum(c[1 + k][:, None] * hs[HESS_INDEX[x][k]] for k in range(3))
            G[:, x] -= fac * (np.einsum("gm,gm->m", gr[x], Z) + np.einsum("gm,gm->m", H, X))
    return G


def _xc_gradient_args(functional, dms, ao, weights, ao_grad, ao_hess):
    """What xc_gradient_host and xc_gradient_spin_host do first: the refusals, then (_xc_contract's first five arguments,
    the weights, the matrices, [(rho, grad rho) of each])."""
    if ao_grad is None:
        raise ValueError("ao_grad is needed: the derivative of the density by a centre is made of it")
    t, gga, ao, gr, dms, dens = _densities(functional, dms, ao, ao_grad)
    if gga and ao_hess is None:
        raise ValueError("ao_hess is needed for a gradient-corrected functional")
    hs = np.ascontiguousarray(ao_hess, dtype=np.float64) if gga else None
    return (2.0 if t == 2 else 1.0, gga, ao, gr, hs), np.ascontiguousarray(weights, dtype=np.float64), dms, dens


def xc_gradient_host(functional, dm, ao, weights, ao_grad, ao_hess=None, quirks=True):
    """G (nao, 3) of DFT_ComputeXCGradient from AO planes in numpy: ao (ngrid, nao), ao_grad (3, ngrid, nao), ao_hess
    (6, ngrid, nao) (not needed for an LDA-class functional).  The point coefficients are the sweep's own, in the
    convention of the solver type: c0 = w vrho, c_k = 4 w vsigma grad_k rho for the one-sided types (GGA, mixes), half
    of each for B3LYP (its M + M^T); in both

        G[mu, x] = -fac sum_g [ ao_grad[x] (Q D) + (sum_k c_k ao_hess[xk]) (AO D) ][g, mu],   Q = 2 c0 AO + sum_k c_k ao_grad[k]

    with fac = 1 (one-sided) or 2 (B3LYP).  With quirks and vwn5_c / pbe_c in the functional the shipped potentials
    are not the derivatives of the energy; G is then built from the shipped ones."""
    planes, w, dms, [(rho, g)] = _xc_gradient_args(functional, [dm], ao, weights, ao_grad, ao_hess)
    return _xc_contract(*planes, [(dms[0], _point_closed(functional, rho, g, w, quirks)[1:])])


def xc_gradient_spin_host(functional, dm_a, dm_b, ao, weights, ao_grad, ao_hess=None):
    """G (nao, 3) of DFT_ComputeXCGradientSpin from AO planes in numpy: the derivative of xc_spin_host's Exc under the
    column replacement above, both spin density matrices and the weights fixed.  The per-spin coefficients c_s0..c_s3 are
    the spin-resolved sweep's own (response.point_spin_host, closed-shell conventions), and

        G[mu, x] = -fac sum_s sum_g [ ao_grad[x] (Q_s D_s) + (sum_k c_sk ao_hess[xk]) (AO D_s) ][g, mu],   Q_s = 2 c_s0 AO + sum_k c_sk ao_grad[k]

    with fac = 1 (one-sided types) or 2 (B3LYP): xc_gradient_host's formula once per spin.  The spin-resolved bodies are the
    derivatives of the energy: no `quirks`."""
    planes, w, dms, [(ra, ga), (rb, gb)] = _xc_gradient_args(functional, [dm_a, dm_b], ao, weights, ao_grad, ao_hess)
    p = response.point_spin_host(functional, ra, rb, ga, gb, w)
    return _xc_contract(*planes, zip(dms, (p[1:5], p[5:9])))


def xc_energy_density_host(functional, dm, ao, ao_grad=None, quirks=True):
    """e_g (ngrid,) of DFT_ComputeXCEnergyDensity from AO planes in numpy: the energy per volume of the sweep's point body at the
    density of dm, without the weight (response.point_host with unit weights)."""
    _, _, ao, _, _, dens = _densities(functional, [dm], ao, ao_grad)
    return _point_closed(functional, *dens[0], np.ones(ao.shape[0]), quirks)[0]


def xc_energy_density_spin_host(functional, dm_a, dm_b, ao, ao_grad=None):
    """e_g (ngrid,) of DFT_ComputeXCEnergyDensitySpin from AO planes in numpy (response.point_spin_host, row 0)."""
    (ra, ga), (rb, gb) = _densities(functional, [dm_a, dm_b], ao, ao_grad)[5]
    return response.point_spin_host(functional, ra, rb, ga, gb)[0]


def _meta_planes(who, *planes):
    """The planes of a meta host entry as C-ordered float64; none may be missing (tau is made of the gradient planes, its
    derivative by a centre of the Hessian planes)."""
    if any(x is None for x in planes):
        raise ValueError(f"{who}: ao_grad{' and ao_hess are' if len(planes) == 3 else ' is'} needed for a meta-GGA")
    return [np.ascontiguousarray(x, dtype=np.float64) for x in planes]


def xc_gradient_meta_host(functional, dm, ao, weights, ao_grad, ao_hess, tau_term=True):
    """G (nao, 3) of DFT_ComputeXCGradientMeta from AO planes in numpy: the derivative of metagga.xc_meta_host's Exc under the
    column replacement above.  tau = 1/2 sum_k (d_k AO) Ds (d_k AO) moves through its gradient planes alone, so with the meta
    point's coefficients (metagga.point_meta_host: c0..c3 one-sided, ct = w e_tau / 2) and Y_k = ao_grad[k] Ds

        G[mu, x] = G_gga[mu, x; c0..c3] - 2 sum_g ct sum_k ao_hess[xk][g, mu] Y_k[g, mu],

    G_gga xc_gradient_host's formula at fac = 1.  The six Hessian planes, no third derivatives.  A functional without a
    meta weight has ct = 0 and gets xc_gradient_host's G of the same mix at quirks 0.  tau_term=False leaves the second sum
    out (for the tests: what a force without the tau term misses)."""
    from . import metagga
    ao, gr, hs = _meta_planes("xc_gradient_meta_host", ao, ao_grad, ao_hess)
    dm = np.asarray(dm, dtype=np.float64)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    rho, g, tau = metagga.density_host(dm, ao, gr)
    p = metagga.point_meta_host(functional, rho, g, tau, w)
    G = _xc_contract(1.0, True, ao, gr, hs, [(dm, p["coef"])])
    ct = p["ct"]
    if tau_term and np.any(ct != 0.0):
        ds = 0.5 * (dm + dm.T)
        Y = [gr[k] @ ds for k in range(3)]
        for x in range(3):
            G[:, x] -= 2.0 * np.einsum("g,gm->m", ct, sum(hs[HESS_INDEX[x][k]] * Y[k] for k in range(3)))
    return G


def xc_energy_density_meta_host(functional, dm, ao, ao_grad):
    """e_g (ngrid,) of DFT_ComputeXCEnergyDensityMeta from AO planes in numpy: the energy per volume of the meta point at the
    density and tau of dm, without the weight (metagga.point_meta_host with unit weights)."""
    from . import metagga
    ao, gr = _meta_planes("xc_energy_density_meta_host", ao, ao_grad)
    rho, g, tau = metagga.density_host(np.asarray(dm, dtype=np.float64), ao, gr)
    return metagga.point_meta_host(functional, rho, g, tau, np.ones(ao.shape[0]))["e"]


def xc_gradient_meta_spin_host(functional, dm_a, dm_b, ao, weights, ao_grad, ao_hess, tau_term=True):
    """G (nao, 3) of DFT_ComputeXCGradientMetaSpin from AO planes in numpy: the derivative of metagga.xc_meta_spin_host's Exc
    under the column replacement above, both spin density matrices and the weights fixed.  xc_gradient_meta_host's terms once
    per spin with the spin point's coefficients (metagga.point_meta_spin_host: c_s0..c_s3 one-sided, ct_s = w e_tau_s / 2),
    Ds_s the symmetric part of dm_s and Y_sk = ao_grad[k] Ds_s:

        G[mu, x] = sum_s { G_gga[mu, x; c_s0..c_s3, Ds_s] - 2 sum_g ct_s sum_k ao_hess[xk][g, mu] Y_sk[g, mu] }.

    A spin without electrons contributes nothing; a functional without a meta weight has ct_s = 0 and gets
    xc_gradient_spin_host's G of the same mix.  tau_term=False leaves the second sum out (for the tests)."""
    from . import metagga
    ao, gr, hs = _meta_planes("xc_gradient_meta_spin_host", ao, ao_grad, ao_hess)
    dms = [np.asarray(d, dtype=np.float64) for d in (dm_a, dm_b)]
    w = np.ascontiguousarray(weights, dtype=np.float64)
    ra, ga, ta, rb, gb, tb = metagga.density_spin_host(dms[0], dms[1], ao, gr)
    p = metagga.point_meta_spin_host(functional, ra, rb, ga, gb, ta, tb, w)
    G = _xc_contract(1.0, True, ao, gr, hs, [(dms[0], p["coef_a"]), (dms[1], p["coef_b"])])
    for dm, ct in zip(dms, (p["ct_a"], p["ct_b"])):
        if tau_term and np.any(ct != 0.0):
            ds = 0.5 * (dm + dm.T)
            Y = [gr[k] @ ds for k in range(3)]
            for x in range(3):
                G[:, x] -= 2.0 * np.einsum("g,gm->m", ct, sum(hs[HESS_INDEX[x][k]] * Y[k] for k in range(3)))
    return G


def xc_energy_density_meta_spin_host(functional, dm_a, dm_b, ao, ao_grad):
    """e_g (ngrid,) of DFT_ComputeXCEnergyDensityMetaSpin from AO planes in numpy: the energy per volume of the spin meta point
    at the densities and taus of dm_a / dm_b, without the weight (metagga.point_meta_spin_host with unit weights)."""
    from . import metagga
    ao, gr = _meta_planes("xc_energy_density_meta_spin_host", ao, ao_grad)
    ra, ga, ta, rb, gb, tb = metagga.density_spin_host(np.asarray(dm_a, dtype=np.float64), np.asarray(dm_b, dtype=np.float64), ao, gr)
    return metagga.point_meta_spin_host(functional, ra, rb, ga, gb, ta, tb, np.ones(ao.shape[0]))["e"]


def _grid_of(grids, symbols, atom_xyz, who):
    """(owner, atomic weights, charges) of a grid that says which atom each point moves with, checked against the atoms."""
    own, w0 = getattr(grids, "atom_index", None), getattr(grids, "atomic_weights", None)
    if own is None or w0 is None:
        raise ValueError(f"{who}: the grid carries no atom_index / atomic_weights (grid_gen.Grids keeps both): it does not say which "
                         "atom a point moves with")
    own, w0 = np.asarray(own), np.asarray(w0, dtype=np.float64)
    natm, ng = np.asarray(atom_xyz).reshape(-1, 3).shape[0], np.asarray(grids.coords).reshape(-1, 3).shape[0]
    if len(symbols) != natm or own.shape != (ng,) or w0.shape != (ng,) or (ng and (own.min() < 0 or own.max() >= natm)):
        raise ValueError(f"{who}: the grid's atom_index / atomic_weights do not match the {natm} atoms and {ng} points")
    return own.astype(np.int64), w0, [basis.atomic_number(s) for s in symbols]


def _xc_grid_response_host(grids, symbols, atom_xyz, gradient, edens, who):
    """-sum_mu G^(A)[mu] + sum_g w0_g e_g D_A cell_g: gradient(rows) and edens(rows) evaluate G and e on a block of rows."""
    from . import grid_gen
    own, w0, charges = _grid_of(grids, symbols, atom_xyz, who)
    xyz = np.asarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
    out = np.zeros_like(xyz)
    e = np.zeros(own.shape[0])
    cut = np.flatnonzero(np.diff(own)) + 1
    for lo, hi in zip(np.concatenate([[0], cut]), np.concatenate([cut, [own.shape[0]]])):
        if hi > lo:
            rows = slice(int(lo), int(hi))
            out[own[lo]] -= gradient(rows).sum(axis=0)
            e[rows] = edens(rows)
    return out + grid_gen.becke_weight_gradient_host(grids.coords, own, xyz, charges, w0 * e)


def xc_grid_response_host(functional, dm, shells, grids, symbols, atom_xyz, quirks=True, planes=None):
    """(natm, 3): the grid response of the XC term of dE/dR_A, the host counterpart of scf.HipBackend.xc_grid_response.  With
    Exc = sum_g w0_g cell_g e_g, the points r_g = R_own(g) + t_g moving rigidly with their owners:

        xc_grid[A] = -sum_mu G^(A)[mu] + sum_g w0_g e_g D_A cell_g,

    G^(A) = xc_gradient_host on the rows atom A owns (the motion of A's points: grad_r e = -sum_B de/dR_B at fixed r), e_g
    the energy per volume (response.point_host with unit weights) and the last sum grid_gen.becke_weight_gradient_host.
    planes: (ao, ao_grad, ao_hess) at grids.coords when the caller has them (evaluated here otherwise)."""
    f = functionals.resolve(functional)
    functionals.refuse_meta(f, "xc_grid_response_host")
    ao, gr, hs = planes if planes is not None else ao_planes_host(shells, grids.coords)
    w = np.asarray(grids.weights, dtype=np.float64)
    gga = f.needs_gradient
    return _xc_grid_response_host(
        grids, symbols, atom_xyz,
        lambda r: xc_gradient_host(f, dm, ao[r], w[r], gr[:, r], hs[:, r] if gga else None, quirks),
        lambda r: xc_energy_density_host(f, dm, ao[r], gr[:, r] if gga else None, quirks), "xc_grid_response_host")


def xc_grid_response_spin_host(functional, dm_a, dm_b, shells, grids, symbols, atom_xyz, planes=None):
    """xc_grid_response_host for an open-shell state: xc_gradient_spin_host per atom block and response.point_spin_host's e."""
    f = functionals.resolve(functional)
    functionals.refuse_meta(f, "xc_grid_response_spin_host")
    ao, gr, hs = planes if planes is not None else ao_planes_host(shells, grids.coords)
    w = np.asarray(grids.weights, dtype=np.float64)
    gga = f.needs_gradient
    return _xc_grid_response_host(
        grids, symbols, atom_xyz,
        lambda r: xc_gradient_spin_host(f, dm_a, dm_b, ao[r], w[r], gr[:, r], hs[:, r] if gga else None),
        lambda r: xc_energy_density_spin_host(f, dm_a, dm_b, ao[r], gr[:, r] if gga else None), "xc_grid_response_spin_host")


def xc_grid_response_meta_host(functional, dm, shells, grids, symbols, atom_xyz, planes=None):
    """xc_grid_response_host for a meta-GGA: xc_gradient_meta_host per atom block and xc_energy_density_meta_host's e.  The
    formula is the same: it holds for any e built from AO values and derivatives at the point."""
    f = functionals.resolve(functional)
    ao, gr, hs = planes if planes is not None else ao_planes_host(shells, grids.coords)
    w = np.asarray(grids.weights, dtype=np.float64)
    return _xc_grid_response_host(
        grids, symbols, atom_xyz,
        lambda r: xc_gradient_meta_host(f, dm, ao[r], w[r], gr[:, r], hs[:, r]),
        lambda r: xc_energy_density_meta_host(f, dm, ao[r], gr[:, r]), "xc_grid_response_meta_host")


def xc_grid_response_meta_spin_host(functional, dm_a, dm_b, shells, grids, symbols, atom_xyz, planes=None):
    """xc_grid_response_meta_host for an open-shell state: xc_gradient_meta_spin_host per atom block and
    xc_energy_density_meta_spin_host's e."""
    f = functionals.resolve(functional)
    ao, gr, hs = planes if planes is not None else ao_planes_host(shells, grids.coords)
    w = np.asarray(grids.weights, dtype=np.float64)
    return _xc_grid_response_host(
        grids, symbols, atom_xyz,
        lambda r: xc_gradient_meta_spin_host(f, dm_a, dm_b, ao[r], w[r], gr[:, r], hs[:, r]),
        lambda r: xc_energy_density_meta_spin_host(f, dm_a, dm_b, ao[r], gr[:, r]), "xc_grid_response_meta_spin_host")


def sum_over_atoms(shells, G):
    """(natm, 3): G (nao, 3) summed over the functions each atom owns (the shell-to-atom map of the shell table)."""
    G = np.asarray(G, dtype=np.float64)
    natm = int(np.max(shells.atom)) + 1
    out = np.zeros((natm, 3))
    for s in range(len(shells.l)):
        c0 = int(shells.ao[s])
        out[int(shells.atom[s])] += G[c0:c0 + 2 * int(shells.l[s]) + 1].sum(axis=0)
    return out


def ao_planes_host(shells, coords):
    """(ao (ngrid, nao), ao_grad (3, ngrid, nao), ao_hess (6, ngrid, nao)) of a basis.ShellTable at coords, in numpy, in
    DFT_EvalAO's conventions: what the host assembly of the gradient sweeps when the backend keeps no planes."""
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    ng, nao = coords.shape[0], int(shells.nao)
    ao, gr = np.zeros((ng, nao)), np.zeros((3, ng, nao))
    for s in range(len(shells.l)):
        l, n, off, col = int(shells.l[s]), int(shells.nprim[s]), int(shells.off[s]), int(shells.ao[s])
        d = coords - np.asarray(shells.xyz[s], dtype=np.float64)[None, :]
        r2 = np.einsum("gk,gk->g", d, d)
        a = np.asarray(shells.exp[off:off + n], dtype=np.float64)
        t = a[None, :] * r2[:, None]
        e = np.where(t < AO_EXP_CUT, np.asarray(shells.coef[off:off + n])[None, :] * np.exp(-np.minimum(t, AO_EXP_CUT)), 0.0)
        R0, R1 = e.sum(axis=1), (-2.0 * a * e).sum(axis=1)
        for m, poly in enumerate(_HARMONICS[l]):
            S = _poly_eval(poly, d)
            ao[:, col + m] = R0 * S
            for i in range(3):
                gr[i, :, col + m] = R0 * _poly_eval(_poly_diff(poly, i), d) + R1 * d[:, i] * S
    return ao, gr, ao_hessian_host(shells, coords)


def _pair_repulsion_gradient(xyz, z, cen, q):
    """(natm, 3): d/dR_A of sum_{A, c} z_A q_c / |R_A - R_c| (pairs closer than 1e-12 bohr -- an atom with itself -- skipped)."""
    d = xyz[:, None, :] - cen[None, :, :]
    r = np.linalg.norm(d, axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(r > 1e-12, z[:, None] * q[None, :] / r ** 3, 0.0)
    return -(f[:, :, None] * d).sum(axis=1)


def _fock(inp, backend, f, dm):
    """The Fock matrix of dm from the backend's parts: ground_state_parts (scf.HipBackend, response.HostResponse) or the
    set_dm / jk / xc interface of the host SCF backends."""
    want_k = f.c_hf != 0.0
    if f.needs_tau and hasattr(backend, "ground_state_parts_meta"):
        parts = backend.ground_state_parts_meta
    else:
        parts = getattr(backend, "ground_state_parts", None)
    if parts is not None:
        from scipy.linalg import eigh
        e0, C0 = eigh(inp.S @ dm @ inp.S, inp.S)
        cocc = np.ascontiguousarray(C0[:, ::-1][:, :inp.nocc] * np.sqrt(np.maximum(e0[::-1][:inp.nocc], 0.0)))
        J, K, V = parts(dm, cocc, want_k)
    else:
        backend.set_dm(dm)
        J, K = backend.jk(want_k)
        V = backend.xc()[1]
    return inp.Hcore + J + 0.5 * (V + V.T) - (0.5 * f.c_hf * K if want_k else 0.0)


_QUIRKY = ("vwn5_c", "pbe_c")


def _checked(who, inp, backend, functional, two_electron, device_method, wrong_result, grid_response, meta=False, hint=None):
    """The refusals nuclear_gradient and nuclear_gradient_uks share; (the functional, its weight vector).  device_method: what
    the backend needs for two_electron="device"; wrong_result: why the SCF result is the other assembly's (None: it is not).
    meta: the caller asked for the meta-GGA assembly -- a meta-GGA is then what is wanted (the weight vector carries the two
    meta weights behind the eight) and anything else is refused; hint: what the meta-GGA refusal adds."""
    if two_electron not in ("host", "device"):
        raise ValueError(f"{who}: two_electron must be 'host' or 'device', not {two_electron!r}")
    if two_electron == "device" and not hasattr(backend, device_method):
        raise ValueError(f"{who}: two_electron='device' needs a backend with a device two-electron gradient "
                         "(scf.HipBackend); this backend has none")
    if wrong_result:
        raise ValueError(wrong_result)
    if getattr(inp, "efield", None) is not None:
        raise ValueError(f"{who}: a run in a uniform electric field (efield) is not supported")
    if getattr(backend, "world", 1) > 1:
        raise ValueError(f"{who} runs on one rank: the grid of this backend is sharded over several")
    if grid_response:
        _grid_of(inp.grids, inp.symbols, inp.atom_xyz, who)          # refuses a grid that does not say which atom a point moves with
    f = functionals.resolve(functional if functional is not None else backend.functional)
    if meta:
        if not f.needs_tau:
            raise ValueError(f"{who}(meta=True) is the gradient of a meta-GGA (DFT_ComputeXCGradientMeta / MetaSpin): {f.name} is not one (it "
                             "carries no tpss_x / tpss_c weight); its gradient is meta=False's")
        return f, f.weight_vector() + f.meta_weight_vector()
    functionals.refuse_meta(f, who, hint)
    return f, f.weight_vector()


def _has_quirky(wv):
    return any(wv[functionals.COMPONENTS.index(c)] != 0.0 for c in _QUIRKY)


def _assemble(inp, backend, f, wv, dm, W, two_electron, mats, host_extra, grid_response, meta=False):
    """(g, terms) from the total density dm, W and the finished two-electron term.  mats: the matrices of the XC term --
    (dm,) for the closed shell (backend.xc_gradient / xc_grid_response, xc_gradient_host / xc_grid_response_host otherwise),
    (dm_a, dm_b) for an open-shell state (the *_spin ones); host_extra: what the host functions take behind them (quirks).
    meta: a meta-GGA (the *_meta ones for the closed shell, the *_meta_spin ones for an open-shell state; wv then carries the
    meta weights too, so that TPSS, whose eight are all zero, keeps its XC term)."""
    spin = len(mats) == 2
    sfx = ("_meta" if meta else "") + ("_spin" if spin else "")
    host_gradient, host_grid = (xc_gradient_meta_spin_host, xc_grid_response_meta_spin_host) if spin and meta else \
                               (xc_gradient_spin_host, xc_grid_response_spin_host) if spin else \
                               (xc_gradient_meta_host, xc_grid_response_meta_host) if meta else (xc_gradient_host, xc_grid_response_host)
    sh, xyz = inp.shells, np.asarray(inp.atom_xyz, dtype=np.float64)
    z = np.array([basis.atomic_number(s) for s in inp.symbols], dtype=np.float64)
    g1 = integrals.grad1e(sh, xyz, z, dm, W)
    field = integrals.point_coulomb_field(sh, xyz, dm)         # sum D d<1/|r - R_A|>/dR_A: the operator part of V
    terms = {"one_electron": g1[0] + g1[1] + g1[2] - z[:, None] * field,
             "two_electron": two_electron,
             "nuclear": _pair_repulsion_gradient(xyz, z, xyz, z)}
    if any(w != 0.0 for w in wv):
        planes = None
        if hasattr(backend, "xc_gradient" + sfx):
            G = getattr(backend, "xc_gradient" + sfx)(*mats)
        else:
            planes = ao, gr, hs = ao_planes_host(sh, inp.grids.coords)
            G = host_gradient(f, *mats, ao, inp.grids.weights, gr, hs if f.needs_gradient else None, *host_extra)
        terms["xc"] = sum_over_atoms(sh, G)
        if grid_response:
            if hasattr(backend, "xc_grid_response" + sfx):
                terms["xc_grid"] = getattr(backend, "xc_grid_response" + sfx)(*mats)
            else:
                terms["xc_grid"] = host_grid(f, *mats, sh, inp.grids, inp.symbols, xyz, *host_extra, planes=planes)
    else:
        terms["xc"] = np.zeros_like(xyz)
        if grid_response:
            terms["xc_grid"] = np.zeros_like(xyz)
    pc = getattr(inp, "point_charges", None)
    if pc is not None and len(pc):
        terms["external"] = integrals.grad1e(sh, pc[:, :3], pc[:, 3], dm, W)[2] + _pair_repulsion_gradient(xyz, z, pc[:, :3], pc[:, 3])
    else:
        terms["external"] = np.zeros_like(xyz)
    return sum(terms.values()), terms


def nuclear_gradient(inp, scf_result, backend, functional=None, quirks=None, two_electron="host", grid_response=False, meta=False):
    """(g (natm, 3) in Ha / bohr, terms): dE/dR_A of the converged closed-shell state `scf_result` (scf.run_scf) and its
    breakdown {"one_electron", "two_electron", "xc", "nuclear", "external"}, each (natm, 3).  By default the derivative at FIXED
    quadrature points and weights: the Becke-weight derivatives and the motion of the points with their atoms are not
    included, so the XC term -- and with it the total -- is not translationally invariant; sum_A g_A measures what is
    left out.  `backend`: what the SCF ran on.  scf.HipBackend sweeps the XC part on the device (xc_gradient); any other
    backend (set_dm / jk / xc, or ground_state_parts) gets it from xc_gradient_host on planes evaluated here.  The
    two-electron part never builds the dense ERI, so runs on Cholesky vectors are served alike.  An embedded run
    (inp.point_charges) includes the basis term over the external charges and the nuclei--charge repulsion ("external");
    the forces on the charges themselves are properties.point_charge_forces'.  functional / quirks default to the
    backend's.  `two_electron`: "host" (integrals.grad2e, the default) or "device" (backend.grad2e: the derivative quartets
    made and contracted on the device, csrc/grad2e.hip); every other term is the same either way.  `grid_response` = True adds
    the term "xc_grid": the motion of the quadrature points with their atoms and the derivatives of the Becke weights
    (backend.xc_grid_response on scf.HipBackend, xc_grid_response_host otherwise); g is then the derivative of the energy as the
    grid follows the atoms, and sums to zero over the atoms.  Without it everything is as it was.
    `meta` = True (the driver's --meta-gradient): the functional is a meta-GGA and the XC terms carry the tau term --
    backend.xc_gradient_meta / xc_grid_response_meta (scf.HipBackend: DFT_ComputeXCGradientMeta) where the backend has them,
    xc_gradient_meta_host / xc_grid_response_meta_host on planes evaluated here otherwise; the Fock matrix of W comes from
    backend.ground_state_parts_meta where there is one.  The other terms do not depend on the functional.  A functional
    that is no meta-GGA is refused; without the keyword a meta-GGA is refused, as before this assembly existed."""
    wrong = ("nuclear_gradient: an unrestricted (UKS) result has no analytic gradient here: the assembly is closed-shell "
             "(nuclear_gradient_uks assembles the open-shell one)") if scf_result.get("uks") else None
    f, wv = _checked("nuclear_gradient", inp, backend, functional, two_electron, "grad2e", wrong, grid_response, meta,
                     functionals.META_GRADIENT_HINT)
    if quirks is None:
        quirks = bool(getattr(backend, "quirks", getattr(backend, "q", True)))
    if quirks and _has_quirky(wv):
        raise ValueError("nuclear_gradient: with quirks = 1 the shipped vwn5_c / pbe_c potentials are not the derivatives of their "
                         "energies, so the converged state is not stationary and the analytic gradient is not the energy's; "
                         "run with --quirks 0")
    dm = np.asarray(scf_result["dm"], dtype=np.float64)
    dm = np.ascontiguousarray(0.5 * (dm + dm.T))
    F = _fock(inp, backend, f, dm)
    W = 0.5 * dm @ F @ dm
    W = 0.5 * (W + W.T)
    g2e = backend.grad2e(dm, f.c_hf) if two_electron == "device" else integrals.grad2e(inp.shells, dm, f.c_hf)
    return _assemble(inp, backend, f, wv, dm, W, g2e, (dm,), () if meta else (quirks,), grid_response, meta)


def nuclear_gradient_uks(inp, uks_result, backend, functional=None, two_electron="host", grid_response=False, meta=False):
    """(g (natm, 3) in Ha / bohr, terms): dE/dR_A of the converged unrestricted state `uks_result` (scf.run_uks), with
    nuclear_gradient's five terms and its conventions (fixed quadrature points and weights).  With D = D_a + D_b:

        one_electron   grad1e with D and W = sym(sum_s D_s F_s D_s), F_s from backend.uks_parts as run_uks assembles it,
                       and the Hellmann-Feynman field of D at the nuclei
        two_electron   d/dR_A [1/2 sum D D (ab|cd) - c_hf/4 sum (D D + M M) (ab|cd)], M = D_a - D_b: integrals.grad2e_spin, or
                       backend.grad2e_spin (DFT_Grad2eSpin: one pass over the derivative integrals) with two_electron="device"
        xc             backend.xc_gradient_spin (DFT_ComputeXCGradientSpin) where the backend has it, xc_gradient_spin_host on
                       planes evaluated here otherwise

    A spin without electrons has D_s = 0 and contributes nothing.  Point charges are served through "external".
    `grid_response` = True adds "xc_grid" as in nuclear_gradient (backend.xc_grid_response_spin / xc_grid_response_spin_host).
    `meta` = True (the driver's --open-shell-meta-gradient): the functional is a meta-GGA, the state scf.run_uks(meta=True)'s.
    F_s then comes from backend.uks_meta_parts (refused where the backend has none) and the XC terms carry the tau term of
    either spin -- backend.xc_gradient_meta_spin / xc_grid_response_meta_spin (scf.HipBackend: DFT_ComputeXCGradientMetaSpin)
    where the backend has them, xc_gradient_meta_spin_host / xc_grid_response_meta_spin_host otherwise.  A functional that is
    no meta-GGA is refused; without the keyword a meta-GGA is refused, as before this assembly existed."""
    wrong = None if ("dm_a" in uks_result and "dm_b" in uks_result) else \
        "nuclear_gradient_uks needs a scf.run_uks result (dm_a, dm_b); nuclear_gradient serves the closed shell"
    f, wv = _checked("nuclear_gradient_uks", inp, backend, functional, two_electron, "grad2e_spin", wrong, grid_response, meta,
                     functionals.OPEN_SHELL_META_GRADIENT_HINT)
    if meta and not hasattr(backend, "uks_meta_parts"):
        raise ValueError("nuclear_gradient_uks(meta=True) takes the Fock matrices of a meta-GGA from backend.uks_meta_parts "
                         "(scf.HipBackend: DFT_ComputeXCMetaSpin); this backend has none")
    if getattr(backend, "dm_factor", False):
        raise ValueError("nuclear_gradient_uks takes the density matrices themselves: run without dm_factor")
    if bool(getattr(backend, "quirks", getattr(backend, "q", False))) and _has_quirky(wv):
        raise ValueError("nuclear_gradient_uks: the spin-resolved potentials are the derivatives of the energy, but with quirks = 1 the "
                         "ground state solved the shipped vwn5_c / pbe_c potentials, which are not; run with --quirks 0")
    from scipy.linalg import eigh
    S = inp.S
    dms = [np.asarray(uks_result[k], dtype=np.float64) for k in ("dm_a", "dm_b")]
    dms = [np.ascontiguousarray(0.5 * (d + d.T)) for d in dms]
    coccs = []
    for d, key in zip(dms, ("nalpha", "nbeta")):       # D_s S is the projector on the occupied orbitals of spin s; an empty spin has no columns
        e0, C0 = eigh(S @ d @ S, S)
        n = int(uks_result[key]) if key in uks_result else int(round(float(np.sum(d * S))))
        coccs.append(np.ascontiguousarray(C0[:, ::-1][:, :n] * np.sqrt(np.maximum(e0[::-1][:n], 0.0))))
    want_k = f.c_hf != 0.0
    J, Ka, Kb, _, Va, Vb = (backend.uks_meta_parts if meta else backend.uks_parts)(dms[0], dms[1], coccs[0], coccs[1], want_k)
    W = np.zeros_like(S)
    for d, V, K in ((dms[0], Va, Ka), (dms[1], Vb, Kb)):
        F = inp.Hcore + J + 0.5 * (V + V.T) - (f.c_hf * K if (want_k and K is not None) else 0.0)
        W += d @ F @ d
    W = 0.5 * (W + W.T)
    dm, ms = np.ascontiguousarray(dms[0] + dms[1]), np.ascontiguousarray(dms[0] - dms[1])
    g2e = backend.grad2e_spin(dms[0], dms[1], f.c_hf) if two_electron == "device" else integrals.grad2e_spin(inp.shells, dm, ms, f.c_hf)
    return _assemble(inp, backend, f, wv, dm, W, g2e, tuple(dms), (), grid_response, meta)
