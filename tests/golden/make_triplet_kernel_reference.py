"""Writes tests/golden/triplet_kernel_ref.npz: the spin-flip (kind 1) and singlet (kind 2) response tables T0..T4 and the
energy at three polarisations, per component, in 60-digit arithmetic (mpmath) -- the independent reference of
tests/test_triplet_cpu.py.  Run by hand (python tests/golden/make_triplet_kernel_reference.py); the tests only read
the file.

The eight spin-resolved energy densities e(ra, rb, saa, sab, sbb) below are restated from the papers' formulas, not
from csrc/xc_spin_functionals.hpp, and arranged differently where the literature offers another arrangement (Slater and
PBE exchange per spin channel rather than through the closed-shell form at doubled density; LYP as Miehlich et al. print
it, with |grad rho|^2, not by the coefficients of the three sigmas; PBE's t through k_s).  Constants that the literature
gives as expressions are expressions here ((1 - ln 2) / pi^2, 1 / (6 pi^2), 4 / (9 (2^(1/3) - 1))); PBE exchange takes
mu = 0.2195149727645171 as the project (and the project it was modelled on) carries it.
No cut-off and no clamp: the point grid avoids them (see POINTS).

Definitions (h = rho / 2, q = sigma / 4; upper sign kind 1, lower sign kind 2), all by mpmath.diff:

    T0 = d/dt e_ra        along (ra, rb) = (h + t/2, h -+ t/2)
    T1 = d/dt e_ra        along (saa, sab, sbb) = (q + t/4, q [+ t/4 for kind 2], q -+ t/4)
    u  = 2 e_saa -+ e_sab
    T2 = d/dt u  along the first line, T3 = d/dt u along the second, T4 = u
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 60
COMPONENTS = ("slater_x", "vwn5_c", "vwn_rpa_c", "pw92_c", "pbe_x", "pbe_c", "b88_x", "lyp_c")
RHOS = [1e-8, 1e-4, 1e-2, 0.3, 5.0, 100.0]
# Reduced gradients s = |grad rho| / (2 kF rho).  The issue's {0, 0.1, 1, 3}, with the points that sit on a cut-off of
# the code replaced: s = 0 (sigma = 0 is below kSigmaCut = 1e-20, where B88 is zero and the PBE bodies hold the reduced
# gradient constant under the perturbation) by 0.01; and at rho = 1e-8 every s below 3 (sigma_bb at zeta = 0.3 would
# fall under the cut-off) by {3, 5, 8, 12}.
S_VALUES = [0.01, 0.1, 1.0, 3.0]
S_VALUES_LOWEST_RHO = [3.0, 5.0, 8.0, 12.0]
ZETAS = [0.0, 0.3, 1.0]

pi = mp.pi
third = mp.mpf(1) / 3


def points():
    out = []
    for r in RHOS:
        for s in (S_VALUES_LOWEST_RHO if r == RHOS[0] else S_VALUES):
            kf = (3 * pi ** 2 * mp.mpf(r)) ** third
            out.append((mp.mpf(r), (2 * kf * mp.mpf(r) * mp.mpf(s)) ** 2, s))
    return out


def pw(x, p):
    return mp.mpf(0) if x == 0 else x ** p


# ---- exchange -------------------------------------------------------------------------------------------------------
def slater_x(ra, rb, saa, sab, sbb):
    return -mp.mpf(3) / 2 * (3 / (4 * pi)) ** third * (pw(ra, 4 * third) + pw(rb, 4 * third))


def pbe_x(ra, rb, saa, sab, sbb):
    kappa, mu = mp.mpf("0.804"), mp.mpf("0.2195149727645171")     # the value the project carries (beta pi^2 / 3 at beta = 0.06672455...), not 0.066725 pi^2 / 3

    def channel(r, s):
        if r == 0:
            return mp.mpf(0)
        s2 = s / (4 * (6 * pi ** 2) ** (2 * third) * r ** (8 * third))
        return -mp.mpf(3) / 4 * (6 / pi) ** third * r ** (4 * third) * (1 + kappa - kappa / (1 + mu * s2 / kappa))
    return channel(ra, saa) + channel(rb, sbb)


def b88_x(ra, rb, saa, sab, sbb):
    beta = mp.mpf("0.0042")

    def channel(r, s):
        if r == 0:
            return mp.mpf(0)
        x = mp.sqrt(s) / r ** (4 * third)
        return -beta * r ** (4 * third) * x ** 2 / (1 + 6 * beta * x * mp.asinh(x))
    return channel(ra, saa) + channel(rb, sbb)


# ---- local correlation ----------------------------------------------------------------------------------------------
def f_zeta(z):
    return (pw(1 + z, 4 * third) + pw(1 - z, 4 * third) - 2) / (2 ** (4 * third) - 2)


FPP0 = 4 / (9 * (mp.mpf(2) ** third - 1))


def interpolate(eP, eF, ac, z):
    return eP + ac * f_zeta(z) / FPP0 * (1 - z ** 4) + (eF - eP) * f_zeta(z) * z ** 4


def vwn_fit(x, A, b, c, x0):
    X = lambda y: y * y + b * y + c
    Q = mp.sqrt(4 * c - b * b)
    at = mp.atan(Q / (2 * x + b))
    return A * (mp.log(x * x / X(x)) + 2 * b / Q * at
                - b * x0 / X(x0) * (mp.log((x - x0) ** 2 / X(x)) + 2 * (b + 2 * x0) / Q * at))


VWN5 = [("0.0310907", "3.72744", "12.9352", "-0.10498"), ("0.01554535", "7.06042", "18.0578", "-0.32500"),
        (None, "1.13107", "13.0045", "-0.0047584")]
VWN_RPA = [("0.0310907", "13.0720", "42.7198", "-0.409286"), ("0.01554535", "20.1231", "101.578", "-0.743294"),
           (None, "1.06835", "11.4813", "-0.228344")]


def vwn(sets):
    def e(ra, rb, saa, sab, sbb):
        rho = ra + rb
        x = mp.sqrt((3 / (4 * pi * rho)) ** third)
        fits = [vwn_fit(x, -1 / (6 * pi ** 2) if A is None else mp.mpf(A), mp.mpf(b), mp.mpf(c), mp.mpf(x0)) for A, b, c, x0 in sets]
        return rho * interpolate(fits[0], fits[1], fits[2], (ra - rb) / rho)
    return e


def pw92_eps(rho, z):
    rs = (3 / (4 * pi * rho)) ** third

    def G(A, a1, b1, b2, b3, b4):
        a1, b1, b2, b3, b4 = (mp.mpf(v) for v in (a1, b1, b2, b3, b4))
        return -2 * A * (1 + a1 * rs) * mp.log(1 + 1 / (2 * A * (b1 * mp.sqrt(rs) + b2 * rs + b3 * rs ** mp.mpf("1.5") + b4 * rs ** 2)))
    A0 = (1 - mp.log(2)) / pi ** 2
    eP = G(A0, "0.21370", "7.5957", "3.5876", "1.6382", "0.49294")
    eF = G(A0 / 2, "0.20548", "14.1189", "6.1977", "3.3662", "0.62517")
    minus_ac = G(1 / (6 * pi ** 2), "0.11125", "10.357", "3.6231", "0.88026", "0.49671")
    return interpolate(eP, eF, -minus_ac, z)


def pw92_c(ra, rb, saa, sab, sbb):
    return (ra + rb) * pw92_eps(ra + rb, (ra - rb) / (ra + rb))


# ---- gradient-corrected correlation ---------------------------------------------------------------------------------
def pbe_c(ra, rb, saa, sab, sbb):
    beta, gamma = mp.mpf("0.066725"), (1 - mp.log(2)) / pi ** 2
    rho = ra + rb
    z = (ra - rb) / rho
    phi = (pw(1 + z, 2 * third) + pw(1 - z, 2 * third)) / 2
    kf = (3 * pi ** 2 * rho) ** third
    ks = mp.sqrt(4 * kf / pi)
    t2 = (saa + 2 * sab + sbb) / (2 * phi * ks * rho) ** 2
    ec = pw92_eps(rho, z)
    A = beta / gamma / (mp.exp(-ec / (gamma * phi ** 3)) - 1)
    H = gamma * phi ** 3 * mp.log(1 + beta / gamma * t2 * (1 + A * t2) / (1 + A * t2 + A ** 2 * t2 ** 2))
    return rho * (ec + H)


def lyp_c(ra, rb, saa, sab, sbb):
    a, b, c, d = mp.mpf("0.04918"), mp.mpf("0.132"), mp.mpf("0.2533"), mp.mpf("0.349")
    cf = mp.mpf(3) / 10 * (3 * pi ** 2) ** (2 * third)
    rho = ra + rb
    grad2 = saa + 2 * sab + sbb                      # |grad rho|^2
    r13 = rho ** (-third)
    omega = mp.exp(-c * r13) / (1 + d * r13) * rho ** (-mp.mpf(11) / 3)
    delta = c * r13 + d * r13 / (1 + d * r13)
    first = -a * 4 / (1 + d * r13) * ra * rb / rho
    inner = (2 ** (mp.mpf(11) / 3) * cf * (pw(ra, 8 * third) + pw(rb, 8 * third))
             + (mp.mpf(47) / 18 - 7 * delta / 18) * grad2
             - (mp.mpf(5) / 2 - delta / 18) * (saa + sbb)
             - (delta - 11) / 9 * (ra / rho * saa + rb / rho * sbb))
    second = -a * b * omega * (ra * rb * inner - mp.mpf(2) / 3 * rho ** 2 * grad2
                               + (mp.mpf(2) / 3 * rho ** 2 - ra ** 2) * sbb + (mp.mpf(2) / 3 * rho ** 2 - rb ** 2) * saa)
    return first + second


ENERGY = {"slater_x": slater_x, "vwn5_c": vwn(VWN5), "vwn_rpa_c": vwn(VWN_RPA), "pw92_c": pw92_c, "pbe_x": pbe_x,
          "pbe_c": pbe_c, "b88_x": b88_x, "lyp_c": lyp_c}


def table(e, rho, sigma, kind):
    sg = -1 if kind == 1 else 1
    ab = 0 if kind == 1 else 1
    h, q = rho / 2, sigma / 4
    rdir = lambda x, u, t: e(h + x + t / 2, h + sg * t / 2, q + 2 * u, q + sg * u, q)
    sdir = lambda x, u, t: e(h + x, h, q + 2 * u + t / 4, q + sg * u + ab * t / 4, q + sg * t / 4)
    o = (mp.mpf(0), mp.mpf(0))
    return [mp.diff(lambda x, t: rdir(x, 0, t), o, (1, 1)), mp.diff(lambda x, t: sdir(x, 0, t), o, (1, 1)),
            mp.diff(lambda u, t: rdir(0, u, t), o, (1, 1)), mp.diff(lambda u, t: sdir(0, u, t), o, (1, 1)),
            mp.diff(lambda u: rdir(0, u, 0), mp.mpf(0))]


def energy_at(e, rho, sigma, z):
    z = mp.mpf(z)
    p, m = (1 + z) / 2, (1 - z) / 2
    return e(rho * p, rho * m, sigma * p * p, sigma * p * m, sigma * m * m)


def main():
    pts = points()
    out = {"rho": np.array([float(r) for r, _, _ in pts]), "sigma": np.array([float(s) for _, s, _ in pts]),
           "s": np.array([s for _, _, s in pts]), "zetas": np.array(ZETAS), "components": np.array(COMPONENTS)}
    for name in COMPONENTS:
        e = ENERGY[name]
        # the inputs the code sees are the doubles stored above: evaluate the reference at exactly those
        dpts = [(mp.mpf(float(r)), mp.mpf(float(s))) for r, s, _ in pts]
        for kind in (1, 2):
            out[f"{name}_kind{kind}"] = np.array([[float(v) for v in table(e, r, s, kind)] for r, s in dpts]).T
        out[f"{name}_energy"] = np.array([[float(energy_at(e, r, s, z)) for r, s in dpts] for z in ZETAS])
        print(name, "done")
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "triplet_kernel_ref.npz"), **out)


if __name__ == "__main__":
    main()
