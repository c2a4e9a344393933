"""Writes tests/golden/meta_ref.npz: the energy per volume e(ra, rb, saa, sab, sbb, ta, tb) of the two meta-GGA components
(tpss_x, tpss_c) and its seven first derivatives, in 60-digit arithmetic (mpmath) -- the independent reference of
tests/test_meta_cpu.py.  Run by hand (python tests/golden/make_meta_reference.py); the tests only read the file.

The energies are written here from the formulas of Tao, Perdew, Staroverov and Scuseria (2003) as the issue states them,
arranged differently from csrc/xc_meta_functionals.hpp (grad zeta from its definition, z and alpha per formula, eps_revPKZB
in the paper's form); PBE correlation is the 60-digit restatement of make_triplet_kernel_reference.py (imported, not
changed).  The derivatives are mpmath.diff of them.  The numerical rules are the header's.  z = tau_W / tau is clamped to 1
with alpha = 0: as constants where tau <= 0 or tau_W >= 2 tau; for tau < tau_W < 2 tau the values are 1 and 0 while the
derivatives stay those of tau_W / tau and (tau - tau_W) / tau_unif -- here z = 1 + (z_raw - z_raw at the point of evaluation)
and alpha likewise (z_alpha; every energy takes that point as `at`).  An absent spin channel (rho_s = 0) adds nothing to the
exchange, to the sum over spins of eps_revPKZB and to the (1 +- zeta)^(-4/3) terms of C(zeta, xi).

Points (every combination; no point sits on a cut-off of the code):
  rho = ra + rb in {1e-7, 1e-5, 1e-3, 0.1, 1, 100};  zeta in {0, +-0.9, +-1};
  per channel |grad rho_s| = 2 kF(rho_s) rho_s s with the reduced gradient s cycling through {0.3, 1, 3} (raised x 4 until
  sigma_ss >= 1e-18), grad rho_b at cos = +-0.6 against grad rho_a, so that sigma_ab takes both signs;
  per channel z_s = tau_W,s / tau_s in {1e-8, 1e-3, 0.3, 0.999} by tau_s = tau_W,s / z_s, and the two clamps:
  tau_s = 0.9 tau_W,s (values z = 1, alpha = 0, derivatives kept -- the alpha = 0 case, on the far side of where a
  one-orbital density sits) and tau_s = 0.4 tau_W,s (constants, reached the way an indefinite density matrix reaches it);
  and, for the second branch of the max() in eps~, at zeta in {0, +-0.9} channel reduced gradients (0.01, 10) and (10, 0.01)
  with z_s = 0.3: the channel with the small gradient then has eps_PBE(n_s, 0) below eps_PBE of the point.
At zeta = +-1 the minority channel has rho = 0, no gradient and no tau, and only e and the three majority derivatives are
stored (the others are NaN in the file): the code does not differentiate by an absent channel.

Stored: x (n, 7) -- the doubles the code is handed: ra, rb, saa, sab, sbb, ta, tb; the reference is evaluated at exactly
those -- zeta (n), ztarget (n; 0 and -1 mark the two clamps), branch (n, 2): 1 where eps~ of channel a / b is eps_PBE of the
point (the second branch of the max), components, and per component `<name>` (n, 8): e and the seven derivatives.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_triplet_kernel_reference import pbe_c  # noqa: E402  (sets mp.mp.dps = 60)
from make_spin_potential_reference import channel_gradient  # noqa: E402

COMPONENTS = ("tpss_x", "tpss_c")
RHOS = [1e-7, 1e-5, 1e-3, 0.1, 1.0, 100.0]
ZETAS = [0.0, 0.9, -0.9, 1.0, -1.0]
ZS = [1e-8, 1e-3, 0.3, 0.999, 0.0, -1.0]     # 0.0: tau_s = 0.9 tau_W,s (held); -1.0: tau_s = 0.4 tau_W,s (constants)
S_CYCLE = [0.3, 1.0, 3.0]
COSINES = [0.6, -0.6]
pi, third = mp.pi, mp.mpf(1) / 3
ZERO = mp.mpf(0)


def z_alpha(n, sigma, tau, at):
    """(z, alpha) of (n, sigma, tau) under the header's rule; at = the same three at the point of evaluation, where the
    branch is chosen and the held values are anchored."""
    def raw(n, sigma, tau):
        tau_w = sigma / (8 * n)
        return tau_w / tau, (tau - tau_w) / (mp.mpf(3) / 10 * (3 * pi ** 2) ** (2 * third) * n ** (5 * third))
    n0, sigma0, tau0 = at
    tw0 = sigma0 / (8 * n0)
    if tau0 <= 0 or tw0 >= 2 * tau0:
        return mp.mpf(1), ZERO
    z, alpha = raw(n, sigma, tau)
    if tw0 > tau0:
        z0, alpha0 = raw(n0, sigma0, tau0)
        return 1 + (z - z0), alpha - alpha0
    return z, alpha


def fx(n, sigma, tau, at):
    """F_x of an unpolarised density."""
    kappa, b, c, e, mu = (mp.mpf(v) for v in ("0.804", "0.40", "1.59096", "1.537", "0.21951"))
    p = sigma / (4 * (3 * pi ** 2) ** (2 * third) * n ** (8 * third))
    z, alpha = z_alpha(n, sigma, tau, at)
    qb = mp.mpf(9) / 20 * (alpha - 1) / mp.sqrt(1 + b * alpha * (alpha - 1)) + 2 * p / 3
    x = ((mp.mpf(10) / 81 + c * z ** 2 / (1 + z ** 2) ** 2) * p + mp.mpf(146) / 2025 * qb ** 2
         - mp.mpf(73) / 405 * qb * mp.sqrt((3 * z / 5) ** 2 / 2 + p ** 2 / 2)
         + (mp.mpf(10) / 81) ** 2 / kappa * p ** 2 + 2 * mp.sqrt(e) * mp.mpf(10) / 81 * (3 * z / 5) ** 2 + e * mu * p ** 3) / (1 + mp.sqrt(e) * p) ** 2
    return 1 + kappa - kappa / (1 + x / kappa)


def tpss_x(ra, rb, saa, sab, sbb, ta, tb, at=None):
    a = at if at is not None else (ra, rb, saa, sab, sbb, ta, tb)

    def channel(r, s, t, r0, s0, t0):      # E_x[2 n_s] / 2
        if r == 0:
            return ZERO
        n = 2 * r
        return -mp.mpf(3) / 4 * (3 / pi) ** third * n ** (4 * third) * fx(n, 4 * s, 2 * t, (2 * r0, 4 * s0, 2 * t0)) / 2
    return channel(ra, saa, ta, a[0], a[2], a[5]) + channel(rb, sbb, tb, a[1], a[4], a[6])


def eps_tilde(ra, rb, saa, sab, sbb):
    """(eps~_a, eps~_b, branch_a, branch_b); None for an absent channel."""
    n = ra + rb
    full = pbe_c(ra, rb, saa, sab, sbb) / n
    out, br = [], []
    for r, s, first in ((ra, saa, True), (rb, sbb, False)):
        if r == 0:
            out.append(None); br.append(0)
            continue
        alone = (pbe_c(r, ZERO, s, ZERO, ZERO) if first else pbe_c(ZERO, r, ZERO, ZERO, s)) / r
        out.append(max(alone, full)); br.append(int(full > alone))
    return out[0], out[1], br[0], br[1]


def tpss_c(ra, rb, saa, sab, sbb, ta, tb, at=None):
    a = at if at is not None else (ra, rb, saa, sab, sbb, ta, tb)
    d = mp.mpf("2.8")
    n = ra + rb
    sigma, tau = saa + 2 * sab + sbb, ta + tb
    z, _ = z_alpha(n, sigma, tau, (a[0] + a[1], a[2] + 2 * a[3] + a[4], a[5] + a[6]))
    zeta = (ra - rb) / n
    # grad zeta = (grad na - grad nb) / n - zeta grad n / n
    gz2 = ((saa - 2 * sab + sbb) - 2 * zeta * (saa - sbb) + zeta ** 2 * sigma) / n ** 2
    gz2 = max(gz2, ZERO)
    xi2 = gz2 / (4 * (3 * pi ** 2 * n) ** (2 * third))
    c0 = mp.mpf("0.53") + mp.mpf("0.87") * zeta ** 2 + mp.mpf("0.50") * zeta ** 4 + mp.mpf("2.26") * zeta ** 6
    s43 = (ZERO if ra == 0 else (1 + zeta) ** (-4 * third)) + (ZERO if rb == 0 else (1 - zeta) ** (-4 * third))
    C = c0 / (1 + xi2 * s43 / 2) ** 4
    eps = pbe_c(ra, rb, saa, sab, sbb) / n
    ea, eb, _, _ = eps_tilde(ra, rb, saa, sab, sbb)
    ssum = (ZERO if ea is None else ra / n * ea) + (ZERO if eb is None else rb / n * eb)
    rev = eps * (1 + C * z ** 2) - (1 + C) * z ** 2 * ssum
    return n * rev * (1 + d * rev * z ** 3)


ENERGY = {"tpss_x": tpss_x, "tpss_c": tpss_c}


def points():
    xs, zetas, zts = [], [], []

    def add(rho, zeta, sa, sb, cos, zt):
        a, b = 0.5 * rho * (1.0 + zeta), 0.5 * rho * (1.0 - zeta)
        na, nb = channel_gradient(a, sa), channel_gradient(b, sb)
        ga, gb = np.array([na, 0.0, 0.0]), np.array([cos * nb, np.sqrt(1.0 - cos * cos) * nb, 0.0])
        saa, sab, sbb = float(ga @ ga), float(ga @ gb), float(gb @ gb)
        f = (1.0 / zt) if zt > 0 else 0.9 if zt == 0 else 0.4
        ta = saa / (8.0 * a) * f if a else 0.0
        tb = sbb / (8.0 * b) * f if b else 0.0
        xs.append([a, b, saa, sab, sbb, ta, tb]); zetas.append(zeta); zts.append(zt)

    k = 0
    for rho in RHOS:
        for zeta in ZETAS:
            for zt in ZS:
                for cos in COSINES:
                    add(rho, zeta, S_CYCLE[k % 3], S_CYCLE[(k + 1) % 3], cos, zt)
                    k += 1
        for zeta in ZETAS[:3]:
            add(rho, zeta, 0.01, 10.0, 0.6, 0.3)
            add(rho, zeta, 10.0, 0.01, -0.6, 0.3)
    return np.array(xs), np.array(zetas), np.array(zts)


def row(e, x, zeta):
    at = tuple(mp.mpf(float(v)) for v in x)
    nan = float("nan")
    keep = [0, 2, 5] if zeta == 1.0 else [1, 4, 6] if zeta == -1.0 else list(range(7))
    out = [float(e(*at, at=at))]
    for k in range(7):
        if k not in keep:
            out.append(nan)
            continue
        f = lambda v, k=k: e(*(at[:k] + (v,) + at[k + 1:]), at=at)
        out.append(float(mp.diff(f, at[k])))
    return out


def main():
    xs, zetas, zts = points()
    br = np.array([eps_tilde(*(mp.mpf(float(v)) for v in x[:5]))[2:] for x in xs])
    out = {"x": xs, "zeta": zetas, "ztarget": zts, "branch": br, "components": np.array(COMPONENTS)}
    for name in COMPONENTS:
        out[name] = np.array([row(ENERGY[name], x, z) for x, z in zip(xs, zetas)])
        print(name, "done")
    np.savez(os.path.join(HERE, "meta_ref.npz"), **out)


if __name__ == "__main__":
    main()
