"""Independent high-precision reference for the AO planes on the grid: values, Cartesian gradients and Hessians of the
contracted real-solid-harmonic Gaussians that oracle/ao_oracle.c, gradients.ao_hessian_host, k_eval_ao and k_eval_ao_hess
evaluate.  Test infrastructure only: pure Python on mpmath, never imported by the product and never by a test marked gpu
(those read tests/golden/ao_ref_*.npz, written from here by tests/golden/make_ao_reference.py).

What it shares with the engines is the specification alone -- component order p: x, y, z; d: xy, yz, z2, xz, x2-y2;
f: m = -3..3; unit self-overlap of every contracted function.  Everything else comes from oracle/eri_reference.py:
  * the angular part is sph_coeffs(l): FITTED Cartesian -> real-solid-harmonic coefficients, no typed constants;
  * the radial coefficients are _prims(shell) and the rows of shell_transform(shell): unit self-overlap from the RAW
    exponents and contraction coefficients, by the reference's own overlap integrals.

Formulation (not the engines' R0 * S, R0 * Sx + R1 * S * x):

    phi_m(r) = sum_p d_p sum_{ijk} T[m, ijk] x^i y^j z^k exp(-a_p r^2),       (x, y, z) = point - centre in mpf,

a sum of Cartesian monomials times one Gaussian, differentiated by the monomial rule

    d/dx [x^i e] = i x^(i-1) e - 2 a x^(i+1) e

once for the gradient planes and twice for the Hessian planes.  Points and centres are taken as the exact doubles given.

ao_planes also returns the MAGNITUDE of the same sums,

    A[plane, g, col] = sum_p (1 + a_p r^2) sum_{terms} |term|,

the scale of the fp64 rounding error of any engine that forms these terms (tests/ao_reference_cases.py derives the model).
The tests compute A themselves in fp64; here it serves the generator's own checks.
"""
import numpy as np
from mpmath import mp, mpf

from . import eri_reference as R

PLANES = ("v", "x", "y", "z", "xx", "xy", "xz", "yy", "yz", "zz")          # Hessian order of DFT_EvalAOHess
_AXES = ((), (0,), (1,), (2,), (0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
NPLANE = {0: 1, 1: 4, 2: 10}


def monomial_rule(power, axes):
    """d/d(axes...) of x^i y^j z^k exp(-a r^2) = sum over the returned (power', n, q) of n (-2a)^q x^i' y^j' z^k' exp(-a r^2)."""
    terms = [(tuple(power), 1, 0)]
    for ax in axes:
        new = []
        for pw, n, q in terms:
            if pw[ax]:
                lo = list(pw)
                lo[ax] -= 1
                new.append((tuple(lo), n * pw[ax], q))
            hi = list(pw)
            hi[ax] += 1
            new.append((tuple(hi), n, q + 1))
        terms = new
    return terms


def shell_scale(sh):
    """(T (2l+1, ncart), d (nprim,)) of a shell as doubles: what the tests' fp64 magnitude uses."""
    with mp.workdps(R.DPS):
        return R.to_double(R.shell_transform(sh)), np.array([float(d) for _, d in R._prims(sh)])


@R._work
def shell_planes(sh, points, deriv=2, skip_from=None):
    """(ref, A), object arrays (nplane, ngrid, 2l+1) of mpf for one shell.  skip_from: leave out every primitive with
    a r^2 >= skip_from (a cut taken there), None keeps all."""
    npl = NPLANE[deriv]
    T = R.shell_transform(sh)
    prims = R._prims(sh)
    carts = R.cart_powers(sh.l)
    rules = [[monomial_rule(pw, _AXES[k]) for pw in carts] for k in range(npl)]
    c = [mpf(x) for x in sh.centre]
    nf = sh.nfun
    ref = np.zeros((npl, len(points), nf), dtype=object)
    A = np.zeros((npl, len(points), nf), dtype=object)
    absT = [[abs(v) for v in row] for row in T]
    for g, pt in enumerate(points):
        d = [mpf(float(pt[k])) - c[k] for k in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        pw_tab = [[dk ** n for n in range(sh.l + 3)] for dk in d]
        for a, dp in prims:
            t = a * r2
            if skip_from is not None and t >= skip_from:
                continue
            e = dp * mp.exp(-t)
            w = 1 + t
            m2a = -2 * a
            for k in range(npl):
                mono, mabs = [], []
                for rule in rules[k]:
                    v = s = mpf(0)
                    for (i, j, kk), n, q in rule:
                        term = n * m2a ** q * pw_tab[0][i] * pw_tab[1][j] * pw_tab[2][kk] * e
                        v += term
                        s += abs(term)
                    mono.append(v)
                    mabs.append(s)
                for m in range(nf):
                    ref[k, g, m] += mp.fdot(T[m], mono)
                    A[k, g, m] += w * mp.fdot(absT[m], mabs)
    return ref, A


def ao_planes(shells, points, deriv=2, skip_from=None):
    """(ref, A): mpf object arrays (nplane, ngrid, nao) over the functions of `shells` in order: plane 0 the value, 1..3 the
    gradient, 4..9 the Hessian xx xy xz yy yz zz.  `shells`: eri_reference.Shell (raw exponents and coefficients)."""
    parts = [shell_planes(s, points, deriv, skip_from) for s in shells]
    return np.concatenate([p[0] for p in parts], axis=2), np.concatenate([p[1] for p in parts], axis=2)


def self_check(digits=30):
    """At three points per l the derivative planes against mp.diff of the value plane; returns the worst relative
    difference (asserted below 10^-digits).  Run at generation time."""
    worst = mpf(0)
    pts = [(0.37, -0.52, 0.81), (-1.3, 0.24, 0.45), (0.011, 1.7, -0.6)]
    for l in range(4):
        sh = R.Shell(l, (0.1, -0.2, 0.05), (1.9, 0.43), (0.6, -0.35))
        with mp.workdps(R.DPS):
            ref, _ = shell_planes(sh, pts, 2)
        with mp.workdps(2 * R.DPS):
            for g, pt in enumerate(pts):
                for m in range(sh.nfun):
                    def f(x, y, z, m=m):
                        return _value(sh, (x, y, z))[m]
                    for k in range(1, 10):
                        order = tuple(_AXES[k].count(ax) for ax in range(3))
                        num = mp.diff(f, tuple(mpf(v) for v in pt), order)
                        scale = max(abs(num), abs(ref[0, g, m]))
                        rel = abs(num - ref[k, g, m]) / scale
                        worst = max(worst, rel)
                        assert rel < mpf(10) ** -digits, (l, g, m, PLANES[k], rel)
    return float(worst)


def _value(sh, xyz):
    """Values of the 2l+1 functions at an mpf position (current precision), for self_check's mp.diff."""
    T = R._shell_transform_at(sh.key(), mp.prec)
    d = [xyz[k] - mpf(sh.centre[k]) for k in range(3)]
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    rad = sum(dp * mp.exp(-mpf(a) * r2) for a, dp in zip(sh.exps, R._prim_coefs_at(sh.key(), mp.prec)))
    mono = [d[0] ** i * d[1] ** j * d[2] ** k for i, j, k in R.cart_powers(sh.l)]
    return [mp.fdot(row, mono) * rad for row in T]
