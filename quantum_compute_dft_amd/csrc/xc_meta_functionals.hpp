// Meta-GGA components: energies per volume of (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb, tau_a, tau_b), fp64.
//
// Two components, tpss_x and tpss_c (Tao, Perdew, Staroverov, Scuseria 2003, written down as recalled: the recipe is
// pinned by exact constraints and limits in tests/test_meta_cpu.py, not by another code).  Templates over the scalar like
// the bodies of xc_spin_functionals.hpp: `double` gives the energy at any polarisation, xc::Dual a first derivative --
// nothing is differentiated by hand.  tau_s = (1/2) sum_i |grad psi_is|^2 of spin s; the closed shell hands over
// (rho/2, rho/2, sigma/4, sigma/4, sigma/4, tau/2, tau/2).
//
//   tpss_x   spin scaling E[ra, rb] = (E[2 ra] + E[2 rb]) / 2 of e = -Cx n^(4/3) F_x(p, z), with sigma -> 4 sigma_ss and
//            tau -> 2 tau_s
//   tpss_c   n eps_revPKZB (1 + d eps_revPKZB z^3) on the clean spin-resolved PBE correlation body (spin_pbe_c), with
//            zeta and xi = |grad zeta| / (2 (3 pi^2 n)^(1/3)) from the densities and the three sigmas
//
// Numerical rules (the 60-digit reference of tests/golden/make_meta_reference.py follows the same ones):
//   * total density below kRhoCut: exactly zero, with all derivatives.  A spin channel below kRhoCut is absent: it adds
//     nothing to the exchange, its share of the sum over spins in eps_revPKZB and its (1 +- zeta)^(-4/3) term of C(zeta, xi)
//     are dropped (the limit of both for a channel that carries neither density nor gradient), so zeta = +-1 divides by
//     nothing.
//   * z = tau_W / tau is clamped to [0, 1].  A one-orbital density has tau = tau_W to rounding, on either side, so the
//     potential must not jump there: for tau < tau_W < 2 tau the VALUE of z is 1 and that of alpha is 0, while their
//     derivative parts stay those of tau_W / tau and (tau - tau_W) / tau_unif (value_held, the rule of sigma_at_cut) --
//     the limit from below, continuous across z = 1.  From tau_W >= 2 tau on, and for tau <= 0 (only a density matrix
//     that is not positive semidefinite gets there), z = 1 and alpha = 0 are constants (derivative zero), as every
//     other clamp in these headers.
//   * no sigma cut-off: p, tau_W = sigma / (8 n) and the reduced gradient of PBE correlation (spin_pbe_c<false>) take sigma
//     as it is -- every expression is smooth at sigma = 0.  (The cut-off of the GGA bodies sets the VALUE of the reduced
//     gradient to zero and keeps the derivative: at the outer grid points, n ~ 1e-11 and sigma < 1e-20 under weights of
//     order one, such a potential is not the derivative of its energy, 1e-8 per point, and z = 1 of a one-electron
//     density would be lost in its tail.)  |grad zeta|^2 below zero (sigmas that belong to no pair of gradients) counts as zero.
//   * sqrt((3z/5)^2 / 2 + p^2 / 2) is zero with zero derivative where its argument is below 1e-40 (p = z = 0).
//   * p is capped at 1e20 (a constant there); F_x has reached 1 + kappa to rounding long before.
//   * the max() of eps~ picks a branch by value; a Dual follows the branch taken.
#pragma once
#include "xc_spin_functionals.hpp"

namespace qcdft {
namespace xc {

struct MetaWeights { double c[2]; };   // order of enum XCMetaComponent (include/dft_solver.h): tpss_x, tpss_c

// The value v with the derivative parts of a.
QCDFT_XC_FN double value_held(double, double v) { return v; }
QCDFT_XC_FN Dual value_held(Dual a, double v) { return {v, a.d}; }
QCDFT_XC_FN Dual2 value_held(Dual2 a, double v) { return {v, a.a, a.b, a.ab}; }

constexpr double kTpssK2 = 9.570780000627304;    // (3 pi^2)^(2/3)

// z = tau_W / tau and alpha = (tau - tau_W) / tau_unif of (n, sigma, tau) under the rules above; tauW = sigma / (8 n).
template <class T>
QCDFT_XC_FN void tpss_z_alpha(T n, T sigma, T tau, T n53, T &z, T &alpha)
{
    const T tauW = sigma / (8.0 * n);
    z = 1.0;
    alpha = 0.0;
    if (tau > 0.0 && tauW < 2.0 * tau) {
        z = tauW / tau;
        alpha = (tau - tauW) / ((0.3 * kTpssK2) * n53);
        if (tauW > tau) {
            z = value_held(z, 1.0);
            alpha = value_held(alpha, 0.0);
        }
        if (z < 0.0) z = 0.0;
    }
}

// n eps of TPSS exchange for an unpolarised density n with sigma = |grad n|^2 and kinetic-energy density tau.
template <class T>
QCDFT_XC_FN T tpss_x_energy(T n, T sigma, T tau)
{
    if (n < kRhoCut) return 0.0;
    constexpr double kappa = 0.804, b = 0.40, c = 1.59096, e = 1.537, mu = 0.21951;
    constexpr double se = 1.2397580409095961;   // sqrt(e)
    const T n13 = cbrt(n);
    const T n53 = n * n13 * n13;
    T p = sigma / ((4.0 * kTpssK2) * n53 * n);
    if (p > 1e20) p = 1e20;
    T z, alpha;
    tpss_z_alpha(n, sigma, tau, n53, z, alpha);
    const T z2 = z * z, p2 = p * p;
    // (alpha - 1) / sqrt(1 + b alpha (alpha - 1)); above alpha = 2 through u = 1 / (alpha - 1), the same function, whose
    // derivative is a sum of terms of one sign (the quotient's loses a factor alpha to cancellation in the tails, z -> 0)
    T fa;
    if (alpha > 2.0) {
        const T u = 1.0 / (alpha - 1.0);
        fa = 1.0 / sqrt(u * u + b * u + b);
    } else {
        fa = (alpha - 1.0) / sqrt(1.0 + b * alpha * (alpha - 1.0));
    }
    const T qb = 0.45 * fa + (2.0 / 3.0) * p;
    const T arg = 0.18 * z2 + 0.5 * p2;         // (3z/5)^2 / 2 + p^2 / 2
    T root = 0.0;
    if (arg > 1e-40) root = sqrt(arg);
    const T opz = 1.0 + z2;
    const T num = ((10.0 / 81.0) + c * z2 / (opz * opz)) * p + (146.0 / 2025.0) * qb * qb - (73.0 / 405.0) * qb * root +
                  ((10.0 / 81.0) * (10.0 / 81.0) / kappa) * p2 + (2.0 * se * (10.0 / 81.0) * 0.36) * z2 + (e * mu) * p2 * p;
    const T den = 1.0 + se * p;
    const T x = num / (den * den);
    const T F = 1.0 + kappa - kappa / (1.0 + x / kappa);
    return n * (-kCx * n13 * F);
}

template <class T>
QCDFT_XC_FN T spin_tpss_x(T ra, T rb, T saa, T sbb, T ta, T tb)
{
    return 0.5 * (tpss_x_energy(2.0 * ra, 4.0 * saa, 2.0 * ta) + tpss_x_energy(2.0 * rb, 4.0 * sbb, 2.0 * tb));
}

template <class T>
QCDFT_XC_FN T spin_tpss_c(T ra, T rb, T saa, T sab, T sbb, T ta, T tb)
{
    const T n = ra + rb;
    if (n < kRhoCut) return 0.0;
    constexpr double d = 2.8;
    const bool pa = !(ra < kRhoCut), pb = !(rb < kRhoCut);
    const T sig = saa + 2.0 * sab + sbb;
    const T n13 = cbrt(n);
    T z, alpha;
    tpss_z_alpha(n, sig, ta + tb, n * n13 * n13, z, alpha);
    const T z2 = z * z;
    const T zeta = (ra - rb) / n;
    // C(zeta, xi): xi^2 (1 +- zeta)^(-4/3) = G / (n^4 kF^2) (n / (2 r_s))^(4/3),  G = n^4 |grad zeta|^2 / 4
    const T ze2 = zeta * zeta;
    const T C0 = 0.53 + ze2 * (0.87 + ze2 * (0.50 + ze2 * 2.26));
    T G = rb * rb * saa - 2.0 * ra * rb * sab + ra * ra * sbb;
    if (G < 0.0) G = 0.0;
    const T n2 = n * n;
    const T xi2 = G / (n2 * n2 * kTpssK2 * n13 * n13);
    T s43 = 0.0;
    if (pa) { const T q = cbrt(n / (2.0 * ra)); s43 = s43 + q * q * q * q; }
    if (pb) { const T q = cbrt(n / (2.0 * rb)); s43 = s43 + q * q * q * q; }
    const T cd = 1.0 + 0.5 * xi2 * s43;
    const T cd2 = cd * cd;
    const T C = C0 / (cd2 * cd2);
    // eps_PBE of the point and of each spin alone (fully polarised), per particle
    const T epbe = spin_pbe_c<false>(ra, rb, saa, sab, sbb) / n;
    T sum = 0.0;
    if (pa) {
        const T zero = 0.0;
        const T ea = spin_pbe_c<false>(ra, zero, saa, zero, zero) / ra;
        sum = sum + (ra / n) * ((ea > epbe) ? ea : epbe);
    }
    if (pb) {
        const T zero = 0.0;
        const T eb = spin_pbe_c<false>(zero, rb, zero, zero, sbb) / rb;
        sum = sum + (rb / n) * ((eb > epbe) ? eb : epbe);
    }
    // eps_PBE (1 + C z^2) - (1 + C) z^2 sum, arranged so that a one-electron density (z = 1, sum = eps_PBE) gives exactly 0
    const T erev = epbe * (1.0 - z2) + (1.0 + C) * z2 * (epbe - sum);
    return n * erev * (1.0 + d * erev * z2 * z);
}

// The weighted sum of the eight components of spin_mix_energy and the two above; a zero weight is a scalar branch around
// the component.  META_ONLY: the eight are left out (the derivative by tau sees the meta components alone).
template <bool META_ONLY, class T>
QCDFT_XC_FN T meta_mix_energy(const MixWeights &m, const MetaWeights &mm, T ra, T rb, T saa, T sab, T sbb, T ta, T tb)
{
    const T rho = ra + rb;
    if (rho < kRhoCut) return 0.0;
    T e = 0.0;
    if (!META_ONLY) e = spin_mix_energy<true>(m, ra, rb, saa, sab, sbb);
    if (mm.c[0] != 0.0) e += mm.c[0] * spin_tpss_x(ra, rb, saa, sbb, ta, tb);
    if (mm.c[1] != 0.0) e += mm.c[1] * spin_tpss_c(ra, rb, saa, sab, sbb, ta, tb);
    return e;
}

// One closed-shell point of the meta-GGA sweep (DFT_ComputeXCMeta) at rho_a = rho_b = rho / 2, sigma_aa = sigma_ab =
// sigma_bb = sigma / 4, tau_a = tau_b = tau / 2: the energy per volume e and its derivatives d = (e_rho, e_sigma, e_tau)
// by xc::Dual, one evaluation after the other.  The coefficients the contraction takes, in mix_point's one-sided
// convention: c0 = w e_rho, c_k = w 4 e_sigma grad_k rho, and ct = w e_tau / 2 for T = sum_k (d_k AO)^T diag(ct) (d_k AO).
struct MetaPoint {
    double e, c[4], ct, d[3];
};

QCDFT_XC_FN MetaPoint meta_point(const MixWeights &m, const MetaWeights &mm, double rho, double gx, double gy, double gz,
                                 double tau, double w)
{
    MetaPoint o = {};
    if (rho < kRhoCut) return o;
    const double h = 0.5 * rho, q = 0.25 * (gx * gx + gy * gy + gz * gz), t = 0.5 * tau;
    {
        const Dual e = meta_mix_energy<false>(m, mm, Dual(h, 0.5), Dual(h, 0.5), Dual(q), Dual(q), Dual(q), Dual(t), Dual(t));
        o.e = e.v;
        o.d[0] = e.d;
    }
    o.d[1] = meta_mix_energy<false>(m, mm, Dual(h), Dual(h), Dual(q, 0.25), Dual(q, 0.25), Dual(q, 0.25), Dual(t), Dual(t)).d;
    if (mm.c[0] != 0.0 || mm.c[1] != 0.0)
        o.d[2] = meta_mix_energy<true>(m, mm, Dual(h), Dual(h), Dual(q), Dual(q), Dual(q), Dual(t, 0.5), Dual(t, 0.5)).d;
    o.c[0] = w * o.d[0];
    const double f = w * 4.0 * o.d[1];
    o.c[1] = f * gx;
    o.c[2] = f * gy;
    o.c[3] = f * gz;
    o.ct = 0.5 * w * o.d[2];
    return o;
}

// One point of the spin-resolved meta-GGA sweep (DFT_ComputeXCMetaSpin), the counterpart of spin_potential_point through
// meta_mix_energy: the energy per volume e and, per spin s (s' the other one),
//     c0_s  = w e_rho_s
//     c_s,k = 2 w (2 e_sigma_ss grad rho_s + e_sigma_ab grad rho_s')_k
//     ct_s  = w e_tau_s / 2
// one-sided, scale 1 (a meta solver is a mix solver: no B3LYP halving); at rho_a = rho_b, grad rho_a = grad rho_b,
// tau_a = tau_b these are meta_point's.  Seven xc::Dual evaluations, one after the other, so that one evaluation's registers
// are live at a time; the two tau directions see the meta components alone.  d[] keeps the derivatives bare, in the order
// (ra, rb, saa, sab, sbb, ta, tb), for the tests.
//
// A channel whose density is below kRhoCut is absent, as in spin_potential_point and qc_meta_energy_spin: its rho, sigma_ss,
// sigma_ab and tau count as exactly 0, its coefficients are exactly 0 and it is not differentiated; the other channel gets
// the zeta = +-1 rules of the bodies above.  Both absent: zeros.
struct MetaSpinPoint {
    double e;
    double a[4], b[4];
    double cta, ctb;
    double d[7];
};

QCDFT_XC_FN MetaSpinPoint meta_spin_point(const MixWeights &m, const MetaWeights &mm, double ra, double rb, double gax, double gay,
                                          double gaz, double gbx, double gby, double gbz, double ta, double tb, double w)
{
    MetaSpinPoint o = {};
    const bool pa = ra >= kRhoCut, pb = rb >= kRhoCut;
    if (!pa && !pb) return o;
    if (!pa) { ra = 0.0; ta = 0.0; }
    if (!pb) { rb = 0.0; tb = 0.0; }
    double saa = 0.0, sab = 0.0, sbb = 0.0;
    if (pa) saa = gax * gax + gay * gay + gaz * gaz;
    if (pb) sbb = gbx * gbx + gby * gby + gbz * gbz;
    if (pa && pb) sab = gax * gbx + gay * gby + gaz * gbz;
    const bool meta = mm.c[0] != 0.0 || mm.c[1] != 0.0;
    if (pa) {
        const Dual e = meta_mix_energy<false>(m, mm, Dual(ra, 1.0), Dual(rb), Dual(saa), Dual(sab), Dual(sbb), Dual(ta), Dual(tb));
        o.e = e.v;
        o.d[0] = e.d;
    }
    if (pb) {
        const Dual e = meta_mix_energy<false>(m, mm, Dual(ra), Dual(rb, 1.0), Dual(saa), Dual(sab), Dual(sbb), Dual(ta), Dual(tb));
        if (!pa) o.e = e.v;
        o.d[1] = e.d;
    }
    if (pa) o.d[2] = meta_mix_energy<false>(m, mm, Dual(ra), Dual(rb), Dual(saa, 1.0), Dual(sab), Dual(sbb), Dual(ta), Dual(tb)).d;
    if (pa && pb) o.d[3] = meta_mix_energy<false>(m, mm, Dual(ra), Dual(rb), Dual(saa), Dual(sab, 1.0), Dual(sbb), Dual(ta), Dual(tb)).d;
    if (pb) o.d[4] = meta_mix_energy<false>(m, mm, Dual(ra), Dual(rb), Dual(saa), Dual(sab), Dual(sbb, 1.0), Dual(ta), Dual(tb)).d;
    if (meta && pa) o.d[5] = meta_mix_energy<true>(m, mm, Dual(ra), Dual(rb), Dual(saa), Dual(sab), Dual(sbb), Dual(ta, 1.0), Dual(tb)).d;
    if (meta && pb) o.d[6] = meta_mix_energy<true>(m, mm, Dual(ra), Dual(rb), Dual(saa), Dual(sab), Dual(sbb), Dual(ta), Dual(tb, 1.0)).d;
    const double f = 2.0 * w;
    if (pa) {
        const double u = 2.0 * o.d[2], v = pb ? o.d[3] : 0.0;
        o.a[0] = w * o.d[0];
        o.a[1] = f * (u * gax + (pb ? v * gbx : 0.0));
        o.a[2] = f * (u * gay + (pb ? v * gby : 0.0));
        o.a[3] = f * (u * gaz + (pb ? v * gbz : 0.0));
        o.cta = 0.5 * w * o.d[5];
    }
    if (pb) {
        const double u = 2.0 * o.d[4], v = pa ? o.d[3] : 0.0;
        o.b[0] = w * o.d[1];
        o.b[1] = f * (u * gbx + (pa ? v * gax : 0.0));
        o.b[2] = f * (u * gby + (pa ? v * gay : 0.0));
        o.b[3] = f * (u * gbz + (pa ? v * gaz : 0.0));
        o.ctb = 0.5 * w * o.d[6];
    }
    return o;
}

} // namespace xc
} // namespace qcdft
