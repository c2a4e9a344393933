// Spin-resolved energy densities of the eight components of xc_functionals.hpp, fp64, and the second-order forward
// type that turns them into the spin-flip (triplet) response table.
//
// Every body returns the energy per volume e(rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb) and is a template over the
// scalar, like the closed-shell bodies beside it (which keep their text: nothing of xc_functionals.hpp changes).
// `double` gives the energy at any polarisation (the host tests look at zeta != 0); `Dual2` (value, two first parts,
// the mixed second part) gives one mixed second derivative and its first derivatives per evaluation -- no first or
// second derivative of a spin-resolved functional is written by hand.  At rho_a = rho_b, sigma_aa = sigma_ab =
// sigma_bb = sigma / 4 every body is rho * eps of its closed-shell counterpart.
//
//   slater_x, pbe_x, b88_x  exact spin scaling E[ra, rb] = (E[2 ra] + E[2 rb]) / 2 with sigma -> 4 sigma_ss
//   vwn5_c, vwn_rpa_c       e_P + alpha_c f(z) / f''(0) (1 - z^4) + (e_F - e_P) f(z) z^4, the paramagnetic, ferromagnetic
//                           and spin-stiffness sets of the respective fit (VWN-RPA: the same interpolation, RPA sets)
//   pw92_c                  the same interpolation with PW92's three sets (its third set fits -alpha_c)
//   pbe_c                   H(rs, z, t) with phi(z), on the spin-resolved uniform-gas energy of pw92_c
//   lyp_c                   the open-shell form of Miehlich, Savin, Stoll and Preuss, arranged by the coefficients of
//                           sigma_aa, sigma_ab, sigma_bb (Johnson, Gill and Pople)
//
// Cut-offs and clamps look at the value, as in the closed-shell bodies; below kRhoCut of the total density everything
// is zero.  The sigma cut-off of PBE exchange and correlation: the closed-shell bodies set the reduced gradient to zero
// at sigma <= kSigmaCut but keep the finite vsigma of that limit, and the shipped response table differentiates them with
// that zero held constant.  The same here: at the cut the value of the reduced gradient is zero, the first Dual2
// direction (which potential: e_sigma) keeps its part, the second (the perturbation) sees a constant.
// B88 is zero below it with all its derivatives, as its closed-shell body is.
#pragma once
#include "xc_functionals.hpp"

namespace qcdft {
namespace xc {

// Second-order forward mode in two directions: v + a e1 + b e2 + ab e1 e2 with e1^2 = e2^2 = 0.
struct Dual2 {
    double v, a, b, ab;
    Dual2() = default;
    QCDFT_XC_FN Dual2(double v_) : v(v_), a(0.0), b(0.0), ab(0.0) {}
    QCDFT_XC_FN Dual2(double v_, double a_, double b_, double ab_) : v(v_), a(a_), b(b_), ab(ab_) {}
};
// f(x) from f, f', f'' at the value
QCDFT_XC_FN Dual2 chain2(Dual2 x, double f, double f1, double f2) { return {f, f1 * x.a, f1 * x.b, f1 * x.ab + f2 * x.a * x.b}; }
QCDFT_XC_FN Dual2 operator-(Dual2 a) { return {-a.v, -a.a, -a.b, -a.ab}; }
QCDFT_XC_FN Dual2 operator+(Dual2 a, Dual2 b) { return {a.v + b.v, a.a + b.a, a.b + b.b, a.ab + b.ab}; }
QCDFT_XC_FN Dual2 operator+(Dual2 a, double b) { return {a.v + b, a.a, a.b, a.ab}; }
QCDFT_XC_FN Dual2 operator+(double a, Dual2 b) { return {a + b.v, b.a, b.b, b.ab}; }
QCDFT_XC_FN Dual2 operator-(Dual2 a, Dual2 b) { return {a.v - b.v, a.a - b.a, a.b - b.b, a.ab - b.ab}; }
QCDFT_XC_FN Dual2 operator-(Dual2 a, double b) { return {a.v - b, a.a, a.b, a.ab}; }
QCDFT_XC_FN Dual2 operator-(double a, Dual2 b) { return {a - b.v, -b.a, -b.b, -b.ab}; }
QCDFT_XC_FN Dual2 operator*(Dual2 a, Dual2 b)
{
    return {a.v * b.v, a.a * b.v + a.v * b.a, a.b * b.v + a.v * b.b, a.ab * b.v + a.a * b.b + a.b * b.a + a.v * b.ab};
}
QCDFT_XC_FN Dual2 operator*(Dual2 a, double b) { return {a.v * b, a.a * b, a.b * b, a.ab * b}; }
QCDFT_XC_FN Dual2 operator*(double a, Dual2 b) { return {a * b.v, a * b.a, a * b.b, a * b.ab}; }
QCDFT_XC_FN Dual2 recip(Dual2 a) { const double i = 1.0 / a.v; return chain2(a, i, -i * i, 2.0 * i * i * i); }
QCDFT_XC_FN Dual2 operator/(Dual2 a, Dual2 b) { return a * recip(b); }
QCDFT_XC_FN Dual2 operator/(Dual2 a, double b) { return {a.v / b, a.a / b, a.b / b, a.ab / b}; }
QCDFT_XC_FN Dual2 operator/(double a, Dual2 b) { return a * recip(b); }
QCDFT_XC_FN Dual2 &operator+=(Dual2 &a, Dual2 b) { a = a + b; return a; }
QCDFT_XC_FN Dual2 &operator*=(Dual2 &a, double b) { a = a * b; return a; }
QCDFT_XC_FN bool operator<(Dual2 a, double b) { return a.v < b; }
QCDFT_XC_FN bool operator>(Dual2 a, double b) { return a.v > b; }
QCDFT_XC_FN bool operator<(Dual2 a, Dual2 b) { return a.v < b.v; }
QCDFT_XC_FN bool operator>(Dual2 a, Dual2 b) { return a.v > b.v; }
QCDFT_XC_FN Dual2 cbrt(Dual2 a) { const double r = ::cbrt(a.v), f1 = r / (3.0 * a.v); return chain2(a, r, f1, -2.0 * f1 / (3.0 * a.v)); }
QCDFT_XC_FN Dual2 sqrt(Dual2 a) { const double r = ::sqrt(a.v), f1 = 0.5 / r; return chain2(a, r, f1, -0.5 * f1 / a.v); }
QCDFT_XC_FN Dual2 log(Dual2 a) { const double i = 1.0 / a.v; return chain2(a, ::log(a.v), i, -i * i); }
QCDFT_XC_FN Dual2 exp(Dual2 a) { const double e = ::exp(a.v); return chain2(a, e, e, e); }
QCDFT_XC_FN Dual2 expm1(Dual2 a) { const double e = ::exp(a.v); return chain2(a, ::expm1(a.v), e, e); }
QCDFT_XC_FN Dual2 atan(Dual2 a) { const double i = 1.0 / (1.0 + a.v * a.v); return chain2(a, ::atan(a.v), i, -2.0 * a.v * i * i); }
QCDFT_XC_FN Dual2 asinh(Dual2 a) { const double i = 1.0 / ::sqrt(1.0 + a.v * a.v); return chain2(a, ::asinh(a.v), i, -a.v * i * i * i); }
QCDFT_XC_FN Dual2 fabs(Dual2 a) { return a.v < 0.0 ? -a : a; }

// sigma at or below its cut-off, as said at the top: value zero, the first direction's part only.
QCDFT_XC_FN double sigma_at_cut(double) { return 0.0; }
QCDFT_XC_FN Dual2 sigma_at_cut(Dual2 a) { return {0.0, a.a, 0.0, 0.0}; }
QCDFT_XC_FN Dual sigma_at_cut(Dual a) { return {0.0, a.d}; }   // first order: the finite vsigma of that limit, as the closed-shell bodies keep it

constexpr double kFpp0 = 1.709920934161365617563962776245;   // f''(0) = 4 / (9 (2^(1/3) - 1))
constexpr double kFden = 0.5198420997897463295344212145565;  // 2^(4/3) - 2

// f(z) = [(1+z)^(4/3) + (1-z)^(4/3) - 2] / (2^(4/3) - 2); a fully polarised side contributes nothing (and no cbrt of 0).
template <class T>
QCDFT_XC_FN T zeta_f(T z)
{
    const T p = 1.0 + z, m = 1.0 - z;
    T s = -2.0;
    if (p > 0.0) s = s + p * cbrt(p);
    if (m > 0.0) s = s + m * cbrt(m);
    return s / kFden;
}

// phi(z) = [(1+z)^(2/3) + (1-z)^(2/3)] / 2
template <class T>
QCDFT_XC_FN T zeta_phi(T z)
{
    const T p = 1.0 + z, m = 1.0 - z;
    T s = 0.0;
    if (p > 0.0) { const T c = cbrt(p); s = s + c * c; }
    if (m > 0.0) { const T c = cbrt(m); s = s + c * c; }
    return 0.5 * s;
}

// The interpolation between the paramagnetic (eP) and ferromagnetic (eF) energies per particle with the spin
// stiffness ac = d^2 eps / d zeta^2 at zeta = 0.
template <class T>
QCDFT_XC_FN T zeta_interp(T eP, T eF, T ac, T z)
{
    const T f = zeta_f(z), z2 = z * z, z4 = z2 * z2;
    return eP + ac * f * (1.0 / kFpp0) * (1.0 - z4) + (eF - eP) * f * z4;
}

template <class T>
QCDFT_XC_FN T spin_slater_x(T ra, T rb)
{
    const T a = 2.0 * ra, b = 2.0 * rb;
    return 0.5 * (a * slater_x(a).e + b * slater_x(b).e);
}

// eps(x) of vwn_form (its energy statements) for one parameter set, by value.
template <class T>
QCDFT_XC_FN T vwn_eps(T x, double A, double b, double c, double x0)
{
    const T X = x * x + b * x + c;
    const double Q = sqrt(4.0 * c - b * b);
    const double X0 = x0 * x0 + b * x0 + c;
    const T at = atan(Q / (2.0 * x + b));
    const T lg = log(x * x / X);
    const T lg0 = log((x - x0) * (x - x0) / X);
    const double w0 = b * x0 / X0;
    return A * (lg + (2.0 * b / Q) * at - w0 * (lg0 + (2.0 * (2.0 * x0 + b) / Q) * at));
}

// VWN: `rpa` selects the three RPA sets (what B3LYP's 0.19 multiplies), else the Monte-Carlo sets of VWN5.
template <class T>
QCDFT_XC_FN T spin_vwn_c(T ra, T rb, bool rpa)
{
    const T rho = ra + rb;
    if (rho < kRhoCut) return 0.0;
    const T rs = cbrt(3.0 / (4.0 * kPi * rho));
    const T x = sqrt(rs);
    const T z = (ra - rb) / rho;
    constexpr double Aa = -1.0 / (6.0 * kPi * kPi);
    if (rpa)
        return rho * zeta_interp(vwn_eps(x, 0.0310907, 13.0720, 42.7198, -0.409286), vwn_eps(x, 0.01554535, 20.1231, 101.578, -0.743294),
                                 vwn_eps(x, Aa, 1.06835, 11.4813, -0.228344), z);
    return rho * zeta_interp(vwn_eps(x, 0.0310907, 3.72744, 12.9352, -0.10498), vwn_eps(x, 0.01554535, 7.06042, 18.0578, -0.32500),
                             vwn_eps(x, Aa, 1.13107, 13.0045, -0.0047584), z);
}

// G(rs) of Perdew and Wang for one parameter set.
template <class T>
QCDFT_XC_FN T pw92_g(T rs, T sq, double A, double a1, double b1, double b2, double b3, double b4)
{
    const T Q = 2.0 * A * (b1 * sq + b2 * rs + b3 * rs * sq + b4 * rs * rs);
    return (-2.0 * A * (1.0 + a1 * rs)) * log(1.0 + 1.0 / Q);
}

// Energy per PARTICLE of the uniform gas at (rho, z), PW92 (modified: the constants to full precision, as pw92_c has them).
template <class T>
QCDFT_XC_FN T pw92_eps_spin(T rho, T z)
{
    const T rs = cbrt(3.0 / (4.0 * kPi * rho));
    const T sq = sqrt(rs);
    const T eP = pw92_g(rs, sq, 0.03109069086965489503, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
    const T eF = pw92_g(rs, sq, 0.01554534543482744751, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
    const T mac = pw92_g(rs, sq, 0.01688686394038962731, 0.11125, 10.357, 3.6231, 0.88026, 0.49671);   // fits -alpha_c
    return zeta_interp(eP, eF, -mac, z);
}

template <class T>
QCDFT_XC_FN T spin_pw92_c(T ra, T rb)
{
    const T rho = ra + rb;
    if (rho < kRhoCut) return 0.0;
    return rho * pw92_eps_spin(rho, (ra - rb) / rho);
}

// rho * eps of pbe_x at (rho, sigma): its energy statements, the reduced gradient at the sigma cut-off as said at the top.
template <class T>
QCDFT_XC_FN T pbe_x_energy(T rho, T sigma)
{
    if (rho < kRhoCut) return 0.0;
    constexpr double kappa = 0.804, mu = 0.2195149727645171;
    const T r13 = cbrt(rho);
    const T kF = cbrt(3.0 * kPi * kPi * rho);
    const T den = 4.0 * kF * kF * rho * rho;
    T s2 = 0.0;
    if (den > 1e-50) s2 = ((sigma > kSigmaCut) ? sigma : sigma_at_cut(sigma)) / den;
    if (s2 > 1e12) s2 = 1e12;
    const T num = 1.0 + mu * s2 / kappa;
    const T F = 1.0 + kappa * (1.0 - 1.0 / num);
    return rho * (-kCx * r13 * F);
}

template <class T>
QCDFT_XC_FN T spin_pbe_x(T ra, T rb, T saa, T sbb)
{
    return 0.5 * (pbe_x_energy(2.0 * ra, 4.0 * saa) + pbe_x_energy(2.0 * rb, 4.0 * sbb));
}

// `ec`: pw92_eps_spin(rho, z), so that a mix which holds PW92 as well evaluates it once.
// CUT = false (the meta-GGA bodies of xc_meta_functionals.hpp): sigma enters as it is, H is smooth at sigma = 0.
template <bool CUT = true, class T>
QCDFT_XC_FN T spin_pbe_c_with(T ec, T rho, T z, T sig)
{
    constexpr double beta = 0.066725, gamma = 0.03109069086965489503;
    const T phi = zeta_phi(z);
    const T phi2 = phi * phi, phi3 = phi2 * phi;
    const T kF = cbrt(3.0 * kPi * kPi * rho);
    const T den16 = 16.0 * kF * rho * rho;
    T t2 = 0.0;
    if (den16 > 1e-50) t2 = (((!CUT || sig > kSigmaCut) ? sig : sigma_at_cut(sig)) * kPi) / (den16 * phi2);
    if (t2 > 1.0e20) t2 = 1.0e20;
    const T x = -ec / (gamma * phi3);
    const T em1 = expm1(x);
    const T A = (fabs(em1) < 1e-20) ? T(1.0e20) : (beta / gamma) / em1;
    const T At2 = A * t2;
    const T Qr = (1.0 + At2) / (1.0 + At2 + At2 * At2);
    const T H = gamma * phi3 * log(1.0 + (beta / gamma) * t2 * Qr);
    return rho * (ec + H);
}

template <bool CUT = true, class T>
QCDFT_XC_FN T spin_pbe_c(T ra, T rb, T saa, T sab, T sbb)
{
    const T rho = ra + rb;
    if (rho < kRhoCut) return 0.0;
    const T z = (ra - rb) / rho;
    return spin_pbe_c_with<CUT>(pw92_eps_spin(rho, z), rho, z, saa + 2.0 * sab + sbb);
}

// rho_s * eps of b88_x for one spin (its energy statements, by value): -beta x^2 rho_s^(4/3) / (1 + 6 beta x asinh x).
template <class T>
QCDFT_XC_FN T b88_x_energy(T rho, T sigma)
{
    if (rho < kRhoCut || sigma < kSigmaCut) return 0.0;
    constexpr double beta = 0.0042;
    const T r13 = cbrt(rho);
    const T r43 = rho * r13;
    const T x = sqrt(sigma) / r43;
    const T term = beta * (x * x) / (1.0 + 6.0 * beta * x * asinh(x));
    return rho * (-term * r13);
}

template <class T>
QCDFT_XC_FN T spin_b88_x(T ra, T rb, T saa, T sbb)
{
    return b88_x_energy(ra, saa) + b88_x_energy(rb, sbb);
}

template <class T>
QCDFT_XC_FN T spin_lyp_c(T ra, T rb, T saa, T sab, T sbb)
{
    const T rho = ra + rb;
    if (rho < 1e-14) return 0.0;     // the cut-off of lyp_c
    constexpr double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    constexpr double CF = 2.87123400018819108;
    constexpr double k113 = 12.699208415745595798;   // 2^(11/3)
    const T rm13 = 1.0 / cbrt(rho);
    const T di = 1.0 / (1.0 + d * rm13);
    const T rm113 = rm13 * rm13 * rm13 * rm13 * rm13 * (rm13 * rm13 * rm13) * (rm13 * rm13 * rm13);
    const T om = exp(-c * rm13) * di * rm113;
    const T delta = c * rm13 + d * rm13 * di;
    const T ab = ra * rb;
    T a83 = 0.0, b83 = 0.0;
    if (ra > 0.0) { const T q = cbrt(ra); a83 = ra * ra * q * q; }
    if (rb > 0.0) { const T q = cbrt(rb); b83 = rb * rb * q * q; }
    const T abw = (a * b) * om;
    const T ninth = ab * (1.0 / 9.0);
    const T Laa = -abw * (ninth * (1.0 - 3.0 * delta - (delta - 11.0) * ra / rho) - rb * rb);
    const T Lbb = -abw * (ninth * (1.0 - 3.0 * delta - (delta - 11.0) * rb / rho) - ra * ra);
    const T Lab = -abw * (ninth * (47.0 - 7.0 * delta) - (4.0 / 3.0) * rho * rho);
    return -4.0 * a * di * ab / rho - (k113 * CF) * abw * ab * (a83 + b83) + Laa * saa + Lab * sab + Lbb * sbb;
}

// The weighted sum (order of MixWeights); a zero weight is a scalar branch around the component, as in mix_point.
// GGA = false: components 4..7 and the sigmas are not looked at.
template <bool GGA, class T>
QCDFT_XC_FN T spin_mix_energy(const MixWeights &m, T ra, T rb, T saa, T sab, T sbb)
{
    const T rho = ra + rb;
    if (rho < kRhoCut) return 0.0;
    T e = 0.0;
    if (m.c[0] != 0.0) e += m.c[0] * spin_slater_x(ra, rb);
    if (m.c[1] != 0.0) e += m.c[1] * spin_vwn_c(ra, rb, false);
    if (m.c[2] != 0.0) e += m.c[2] * spin_vwn_c(ra, rb, true);
    const bool with_pbe_c = GGA && m.c[5] != 0.0;
    if (m.c[3] != 0.0 || with_pbe_c) {
        const T z = (ra - rb) / rho;
        const T ec = pw92_eps_spin(rho, z);
        if (m.c[3] != 0.0) e += m.c[3] * (rho * ec);
        if (with_pbe_c) e += m.c[5] * spin_pbe_c_with(ec, rho, z, saa + 2.0 * sab + sbb);
    }
    if (GGA) {
        if (m.c[4] != 0.0) e += m.c[4] * spin_pbe_x(ra, rb, saa, sbb);
        if (m.c[6] != 0.0) e += m.c[6] * spin_b88_x(ra, rb, saa, sbb);
        if (m.c[7] != 0.0) e += m.c[7] * spin_lyp_c(ra, rb, saa, sab, sbb);
    }
    return e;
}

// One ground-state point of the response table in the five-plane layout of k_fxc_table (no weight), at
// rho_a = rho_b = rho / 2 and sigma_aa = sigma_ab = sigma_bb = sigma / 4.  The perturbation moves
//   kind 1 (triplet, spin flip):  rho_a, rho_b by +- r1 / 2,   sigma_aa, sigma_bb by +- s1 / 4,   sigma_ab not at all
//   kind 2 (singlet):             rho_a, rho_b by    r1 / 2,   all three sigmas by    s1 / 4
// and the planes are the response of the alpha potential: T0 = d(e_ra) / r1, T1 = d(e_ra) / s1, and with
// u = 2 e_saa -+ e_sab the coefficient of the alpha gradient field (e_sab multiplies grad rho_b = -+ the alpha change),
// T2 = du / r1, T3 = du / s1, T4 = u.  One Dual2 evaluation yields T0, one T4 and T2, one T3, one T1 (= T2 / 4 above
// the sigma cut-off: the order of the two derivatives, and a <-> b): each one's registers are live alone.  `which`: a
// bit per evaluation (1, 2, 4, 8), so that a kernel can spread them over launches; a plane is written by the evaluation
// that owns it.
template <bool GGA>
QCDFT_XC_FN void spin_table_point(const MixWeights &m, int kind, int which, double rho, double sigma, double scale,
                                  double *t0, double *t1, double *t2, double *t3, double *t4)
{
    const double sg = kind == 1 ? -1.0 : 1.0;
    const double h = 0.5 * rho, q = 0.25 * sigma;
    if (which & 1) {
        const Dual2 e = spin_mix_energy<GGA>(m, Dual2(h, 1.0, 0.5, 0.0), Dual2(h, 0.0, 0.5 * sg, 0.0), Dual2(q), Dual2(q), Dual2(q));
        *t0 = scale * e.ab;
    }
    if (!GGA) return;
    if (which & 2) {
        const Dual2 e = spin_mix_energy<GGA>(m, Dual2(h, 0.0, 0.5, 0.0), Dual2(h, 0.0, 0.5 * sg, 0.0), Dual2(q, 2.0, 0.0, 0.0),
                                             Dual2(q, sg, 0.0, 0.0), Dual2(q));
        *t2 = scale * e.ab;
        *t4 = scale * e.a;
    }
    if (which & 4) {
        const Dual2 e = spin_mix_energy<GGA>(m, Dual2(h), Dual2(h), Dual2(q, 2.0, 0.25, 0.0),
                                             Dual2(q, sg, kind == 1 ? 0.0 : 0.25, 0.0), Dual2(q, 0.0, 0.25 * sg, 0.0));
        *t3 = scale * e.ab;
    }
    if (which & 8) {
        const Dual2 e = spin_mix_energy<GGA>(m, Dual2(h, 1.0, 0.0, 0.0), Dual2(h), Dual2(q, 0.0, 0.25, 0.0),
                                             Dual2(q, 0.0, kind == 1 ? 0.0 : 0.25, 0.0), Dual2(q, 0.0, 0.25 * sg, 0.0));
        *t1 = scale * e.ab;
    }
}

// One ground-state point of the spin-resolved sweep (DFT_ComputeXCSpin): the energy per volume e and, per spin s (s' the
// other one), the coefficients the Vxc kernels contract with the AO planes, in the layout and the convention of the
// closed-shell point bodies:
//     c0_s  = scale w e_rho_s
//     c_s,k = 2 scale w (2 e_sigma_ss grad rho_s + e_sigma_ab grad rho_s')_k
// one-sided like gga_point / mix_point (the caller averages V_s with its transpose); at rho_a = rho_b, grad rho_a =
// grad rho_b these are w vrho and w 4 vsigma g_k of the closed shell.  `scale`: 1, and B3LYP's 1/2 (builtin_spin_mix), whose
// slabs come out as M + M^T.  The five first derivatives are xc::Dual through the bodies above, one evaluation after the
// other, so that one evaluation's registers are live at a time; d[] keeps them bare (ra, rb, saa, sab, sbb) for the tests.
//
// Polarised points: a channel whose density is below kRhoCut is absent -- its rho, its sigma_ss and sigma_ab count as
// exactly 0, its coefficients are 0 and it is not differentiated (d phi / d zeta of pbe_c diverges at |zeta| = 1, and a
// cbrt(Dual) at 0 is 0/0); the other channel gets the zeta = +-1 limit of the bodies, whose guards (p > 0, ra > 0, the
// cut-offs of the exchange channels) never look at the absent side.  Both absent: zeros.
struct SpinPoint {
    double e;
    double a[4], b[4];
    double d[5];
};

template <bool GGA>
QCDFT_XC_FN SpinPoint spin_potential_point(const MixWeights &m, double ra, double rb, double gax, double gay, double gaz,
                                           double gbx, double gby, double gbz, double w, double scale)
{
    SpinPoint o = {};
    const bool pa = ra >= kRhoCut, pb = rb >= kRhoCut;
    if (!pa && !pb) return o;
    if (!pa) ra = 0.0;
    if (!pb) rb = 0.0;
    double saa = 0.0, sab = 0.0, sbb = 0.0;
    if (GGA) {
        if (pa) saa = gax * gax + gay * gay + gaz * gaz;
        if (pb) sbb = gbx * gbx + gby * gby + gbz * gbz;
        if (pa && pb) sab = gax * gbx + gay * gby + gaz * gbz;
    }
    if (pa) {
        const Dual e = spin_mix_energy<GGA>(m, Dual(ra, 1.0), Dual(rb), Dual(saa), Dual(sab), Dual(sbb));
        o.e = e.v;
        o.d[0] = e.d;
    }
    if (pb) {
        const Dual e = spin_mix_energy<GGA>(m, Dual(ra), Dual(rb, 1.0), Dual(saa), Dual(sab), Dual(sbb));
        if (!pa) o.e = e.v;
        o.d[1] = e.d;
    }
    const double sw = scale * w;
    if (pa) o.a[0] = sw * o.d[0];
    if (pb) o.b[0] = sw * o.d[1];
    if (!GGA) return o;
    if (pa) o.d[2] = spin_mix_energy<GGA>(m, Dual(ra), Dual(rb), Dual(saa, 1.0), Dual(sab), Dual(sbb)).d;
    if (pa && pb) o.d[3] = spin_mix_energy<GGA>(m, Dual(ra), Dual(rb), Dual(saa), Dual(sab, 1.0), Dual(sbb)).d;
    if (pb) o.d[4] = spin_mix_energy<GGA>(m, Dual(ra), Dual(rb), Dual(saa), Dual(sab), Dual(sbb, 1.0)).d;
    const double f = 2.0 * sw;
    if (pa) {
        const double u = 2.0 * o.d[2], v = pb ? o.d[3] : 0.0;
        o.a[1] = f * (u * gax + (pb ? v * gbx : 0.0));
        o.a[2] = f * (u * gay + (pb ? v * gby : 0.0));
        o.a[3] = f * (u * gaz + (pb ? v * gbz : 0.0));
    }
    if (pb) {
        const double u = 2.0 * o.d[4], v = pa ? o.d[3] : 0.0;
        o.b[1] = f * (u * gbx + (pa ? v * gax : 0.0));
        o.b[2] = f * (u * gby + (pa ? v * gay : 0.0));
        o.b[3] = f * (u * gbz + (pa ? v * gaz : 0.0));
    }
    return o;
}

// The second derivatives of the energy at ANY polarisation (DFT_FxcPrepareSpinPol): the table behind the response of the
// two spin potentials of spin_potential_point to a perturbation of the two spin densities.  With x = (ra, rb, saa, sab,
// sbb), g_i = de/dx_i and H_ij = d(g_i)/dx_j: one Dual2 evaluation with the first direction along x_i (the potential's
// variable) and the second along x_j (the perturbation) yields H_ij in its mixed part and g_i in its first part.
//
// SpinVars is the point as spin_potential_point prepares it: a channel below kRhoCut is absent, its rho, its sigma_ss and
// sigma_ab are exactly 0.  A variable of an absent channel (x_3 = sigma_ab belongs to both) is not differentiated: its g
// and its rows and columns of H are exactly 0, so it neither responds nor is responded to; both absent: all zero.
//
// H is symmetric wherever the bodies are smooth.  At a sigma cut-off of PBE exchange or correlation (sigma_at_cut) the
// two orders differ: the first direction keeps its part, the second sees a constant -- the rule of spin_table_point.
// spin_sigma_cut says whether a point sits there (never for an LDA-class functional); callers keep H_ji for i < j beside
// H_ij and evaluate it in its own order at such points.
struct SpinVars {
    double ra, rb, saa, sab, sbb;
    bool pa, pb;
};

template <bool GGA>
QCDFT_XC_FN SpinVars spin_vars(double ra, double rb, double gax, double gay, double gaz, double gbx, double gby, double gbz)
{
    SpinVars x = {0.0, 0.0, 0.0, 0.0, 0.0, ra >= kRhoCut, rb >= kRhoCut};
    if (x.pa) x.ra = ra;
    if (x.pb) x.rb = rb;
    if (GGA) {
        if (x.pa) x.saa = gax * gax + gay * gay + gaz * gaz;
        if (x.pb) x.sbb = gbx * gbx + gby * gby + gbz * gbz;
        if (x.pa && x.pb) x.sab = gax * gbx + gay * gby + gaz * gbz;
    }
    return x;
}

QCDFT_XC_FN bool spin_var_present(const SpinVars &x, int i)
{
    return i == 0 || i == 2 ? x.pa : i == 1 || i == 4 ? x.pb : (x.pa && x.pb);
}

// Generous by a factor of two: a point flagged without need is evaluated in both orders, which is always right.
QCDFT_XC_FN bool spin_sigma_cut(const SpinVars &x)
{
    const double c = 2.0 * kSigmaCut;
    return (x.pa && 4.0 * x.saa <= c) || (x.pb && 4.0 * x.sbb <= c) || (x.saa + 2.0 * x.sab + x.sbb <= c);
}

// H_ij and g_i of one ordered pair; zeros when x_i or x_j belongs to an absent channel.
template <bool GGA>
QCDFT_XC_FN void spin_hessian_entry(const MixWeights &m, const SpinVars &x, int i, int j, double *h, double *gi)
{
    *h = 0.0;
    *gi = 0.0;
    if (!spin_var_present(x, i) || !spin_var_present(x, j)) return;
    const Dual2 e = spin_mix_energy<GGA>(m, Dual2(x.ra, i == 0 ? 1.0 : 0.0, j == 0 ? 1.0 : 0.0, 0.0),
                                         Dual2(x.rb, i == 1 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, 0.0),
                                         Dual2(x.saa, i == 2 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0, 0.0),
                                         Dual2(x.sab, i == 3 ? 1.0 : 0.0, j == 3 ? 1.0 : 0.0, 0.0),
                                         Dual2(x.sbb, i == 4 ? 1.0 : 0.0, j == 4 ? 1.0 : 0.0, 0.0));
    *h = e.ab;
    *gi = e.a;
}

// Plane numbering of the table: the upper triangle of H row by row (nv = 5: 15 planes; nv = 2 for an LDA-class
// functional: 3), and for i < j the position of H_ji among the off-diagonal pairs in the same order (nv = 5: 0..9).
QCDFT_XC_FN constexpr int pol_upper(int nv, int i, int j) { return i * nv - i * (i - 1) / 2 + (j - i); }
QCDFT_XC_FN constexpr int pol_lower(int nv, int i, int j) { return pol_upper(nv, i, j) - (i + 1); }
constexpr int kPolG = 15;       // planes 15..17: g_2, g_3, g_4
constexpr int kPolLower = 18;   // planes 18..27: H_ji, i < j
constexpr int kPolPlanes = 28;  // a gradient functional's table; an LDA-class one has 3

// The component weights and the factor of a built-in solver type (0 LDA, 1 GGA, 2 B3LYP), as its point body mixes
// them: B3LYP's M + M^T with the halved vrho is half the one-sided table.
QCDFT_XC_FN double builtin_spin_mix(int type, MixWeights &m)
{
    for (int k = 0; k < 8; ++k) m.c[k] = 0.0;
    if (type == 0) { m.c[0] = 1.0; m.c[1] = 1.0; return 1.0; }
    if (type == 1) { m.c[4] = 1.0; m.c[5] = 1.0; return 1.0; }
    m.c[0] = 0.80; m.c[6] = 0.72; m.c[2] = 0.19; m.c[7] = 0.81;
    return 0.5;
}

} // namespace xc
} // namespace qcdft
