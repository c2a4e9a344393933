"""Writes tests/golden/spin_potential_ref.npz: the energy per volume e(ra, rb, saa, sab, sbb) of the eight components and
its five first derivatives at polarised points, in 60-digit arithmetic (mpmath) -- the independent reference of
tests/test_spin_potential_cpu.py.  Run by hand (python tests/golden/make_spin_potential_reference.py); the tests only
read the file.

The energies are the restatements of make_triplet_kernel_reference.py (from the papers' formulas, arranged differently from
csrc/xc_spin_functionals.hpp; that file is imported, not changed); the derivatives are mpmath.diff of them.

Points: rho = ra + rb log-spaced over 1e-7 ... 10 (nine values), zeta in {0, +-0.3, +-0.9, +-1}, and per (rho, zeta) two
directions of grad rb against grad ra, cos = +-0.6, so that sigma_ab takes both signs.  The gradients are per channel,
|grad rho_s| = 2 kF(rho_s) rho_s s with the reduced gradient s cycling through {0.3, 1, 3}, raised (x 4 until it fits)
where sigma_ss would fall under 1e-18: no point sits on a cut-off of the code (kSigmaCut = 1e-20 per channel for B88, for
the total in PBE).  At zeta = +-1 the minority channel has rho = 0 and no gradient, and only e and the two majority
derivatives are stored (the others are NaN in the file): the code evaluates such a point as fully polarised and does not
differentiate by the absent channel, where d phi / d zeta of PBE correlation diverges.

Stored: ra, rb (n), ga, gb (n, 3) -- the doubles the code is handed; the reference is evaluated at exactly those, with
sigma_ss' = grad rho_s . grad rho_s' formed in 60 digits -- zeta (n), components, and per component `<name>` (n, 6): e,
e_ra, e_rb, e_saa, e_sab, e_sbb.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_triplet_kernel_reference import COMPONENTS, ENERGY  # noqa: E402  (sets mp.mp.dps = 60)

RHOS = np.logspace(-7, 1, 9)
ZETAS = [0.0, 0.3, -0.3, 0.9, -0.9, 1.0, -1.0]
S_CYCLE = [0.3, 1.0, 3.0]
COSINES = [0.6, -0.6]


def channel_gradient(r, s):
    """|grad rho_s| of reduced gradient s (per channel), s raised until sigma_ss >= 1e-18."""
    if r == 0.0:
        return 0.0
    while True:
        g = 2.0 * np.cbrt(3.0 * np.pi ** 2 * r) * r * s
        if g * g >= 1e-18:
            return g
        s *= 4.0


def points():
    ra, rb, ga, gb, zs = [], [], [], [], []
    k = 0
    for rho in RHOS:
        for z in ZETAS:
            for c in COSINES:
                a, b = 0.5 * rho * (1.0 + z), 0.5 * rho * (1.0 - z)
                na, nb = channel_gradient(a, S_CYCLE[k % 3]), channel_gradient(b, S_CYCLE[(k + 1) % 3])
                k += 1
                ra.append(a); rb.append(b); zs.append(z)
                ga.append([na, 0.0, 0.0])
                gb.append([c * nb, np.sqrt(1.0 - c * c) * nb, 0.0])
    return np.array(ra), np.array(rb), np.array(ga), np.array(gb), np.array(zs)


def row(e, ra, rb, ga, gb, z):
    m = lambda x: mp.mpf(float(x))
    a, b = m(ra), m(rb)
    dot = lambda u, v: sum(m(p) * m(q) for p, q in zip(u, v))
    saa, sab, sbb = dot(ga, ga), dot(ga, gb), dot(gb, gb)
    nan = float("nan")
    if z == 1.0:      # alpha alone: e, e_ra, e_saa
        f = lambda x, s: e(x, mp.mpf(0), s, mp.mpf(0), mp.mpf(0))
        return [float(f(a, saa)), float(mp.diff(f, (a, saa), (1, 0))), nan, float(mp.diff(f, (a, saa), (0, 1))), nan, nan]
    if z == -1.0:     # beta alone: e, e_rb, e_sbb
        f = lambda x, s: e(mp.mpf(0), x, mp.mpf(0), mp.mpf(0), s)
        return [float(f(b, sbb)), nan, float(mp.diff(f, (b, sbb), (1, 0))), nan, nan, float(mp.diff(f, (b, sbb), (0, 1)))]
    at = (a, b, saa, sab, sbb)
    return [float(e(*at))] + [float(mp.diff(e, at, tuple(int(i == k) for i in range(5)))) for k in range(5)]


def main():
    ra, rb, ga, gb, zs = points()
    out = {"ra": ra, "rb": rb, "ga": ga, "gb": gb, "zeta": zs, "components": np.array(COMPONENTS)}
    for name in COMPONENTS:
        out[name] = np.array([row(ENERGY[name], *p) for p in zip(ra, rb, ga, gb, zs)])
        print(name, "done")
    np.savez(os.path.join(HERE, "spin_potential_ref.npz"), **out)


if __name__ == "__main__":
    main()
