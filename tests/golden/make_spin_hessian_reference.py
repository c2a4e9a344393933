"""Writes tests/golden/spin_hessian_ref.npz: all second derivatives of the energy per volume e(ra, rb, saa, sab, sbb) of the
eight components at the 126 polarised points of make_spin_potential_reference.py, in 60-digit arithmetic (mpmath) -- the
independent reference of tests/test_spin_response_cpu.py for the table of DFT_FxcPrepareSpinPol.  Run by hand
(python tests/golden/make_spin_hessian_reference.py); the tests only read the file.

The energies are the restatements of make_triplet_kernel_reference.py (imported through make_spin_potential_reference.py,
not changed), the points are that file's points() -- no point sits on a cut-off of the code --, the derivatives are
mpmath.diff of the energies, mixed partials included.  At zeta = +-1 the minority channel has rho = 0 and no gradient:
only the block of the majority's (rho_s, sigma_ss) is stored, everything else is NaN in the file (the code does not
differentiate by an absent channel and leaves exact zeros there).

A second derivative below 1e-40 |e| / |x_i x_j| is stored as exactly 0: it vanishes to the precision of the reference (LYP is
linear in the three sigmas, and what mpmath.diff returns there is its own rounding, 1e-84 and the like).

Stored: ra, rb (n), ga, gb (n, 3), zeta (n), components, and per component `<name>` (n, 5, 5): H_ij = d^2 e / dx_i dx_j,
x = (ra, rb, saa, sab, sbb), symmetric.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_spin_potential_reference import COMPONENTS, ENERGY, points  # noqa: E402  (sets mp.mp.dps = 60)


def orders(n, i, j):
    o = [0] * n
    o[i] += 1
    o[j] += 1
    return tuple(o)


def hessian(e, ra, rb, ga, gb, z):
    m = lambda x: mp.mpf(float(x))
    a, b = m(ra), m(rb)
    dot = lambda u, v: sum(m(p) * m(q) for p, q in zip(u, v))
    saa, sab, sbb = dot(ga, ga), dot(ga, gb), dot(gb, gb)
    H = np.full((5, 5), np.nan)
    zero = mp.mpf(0)
    if z == 1.0:      # alpha alone: the block of (ra, saa)
        f, at, idx = (lambda x, s: e(x, zero, s, zero, zero)), (a, saa), (0, 2)
    elif z == -1.0:   # beta alone: the block of (rb, sbb)
        f, at, idx = (lambda x, s: e(zero, x, zero, zero, s)), (b, sbb), (1, 4)
    else:
        f, at, idx = e, (a, b, saa, sab, sbb), (0, 1, 2, 3, 4)
    n = len(at)
    e0 = abs(f(*at))
    for p in range(n):
        for q in range(p, n):
            h = mp.diff(f, at, orders(n, p, q))
            if abs(h) * abs(at[p] * at[q]) < mp.mpf("1e-40") * e0:
                h = zero
            H[idx[p], idx[q]] = H[idx[q], idx[p]] = float(h)
    return H


def main():
    ra, rb, ga, gb, zs = points()
    out = {"ra": ra, "rb": rb, "ga": ga, "gb": gb, "zeta": zs, "components": np.array(COMPONENTS)}
    for name in COMPONENTS:
        out[name] = np.array([hessian(ENERGY[name], *p) for p in zip(ra, rb, ga, gb, zs)])
        print(name, "done", flush=True)
    np.savez(os.path.join(HERE, "spin_hessian_ref.npz"), **out)


if __name__ == "__main__":
    main()
