// Pointwise exchange-correlation functionals, fp64, closed shell.
//
// Device restatement of the ten __device__ functionals of the reference
// (src/dft_solver.cu:61-283) and of the per-point bodies of its three fused
// kernels (:309-344, :382-432, :434-513).  Same constants, same density /
// gradient cut-offs, same algebra; `quirks` selects the reference's shipped
// derivative formulas (true) or the finite-difference-verified ones (false)
// for the two places they differ.
//
// Every body is a template over the scalar: `double` is what the kernels evaluate, `Dual` (value and one directional
// derivative, below) is what the response kernels (xc_response.hip) and the host table (xc_response_host.cpp) push
// through the SAME statements to get the derivatives of the shipped vrho / vsigma -- no second derivative is written
// by hand.  Comparisons, clamps and cut-offs look at the value; a clamped quantity is a constant (derivative zero).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QCDFT_XC_FN __host__ __device__ __forceinline__
#else
#include <cmath>
#define QCDFT_XC_FN inline
#endif

namespace qcdft {
namespace xc {

// Forward-mode automatic differentiation in one direction: v + d * epsilon.
struct Dual {
    double v, d;
    Dual() = default;
    QCDFT_XC_FN Dual(double v_) : v(v_), d(0.0) {}
    QCDFT_XC_FN Dual(double v_, double d_) : v(v_), d(d_) {}
};
QCDFT_XC_FN Dual operator-(Dual a) { return {-a.v, -a.d}; }
QCDFT_XC_FN Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
QCDFT_XC_FN Dual operator+(Dual a, double b) { return {a.v + b, a.d}; }
QCDFT_XC_FN Dual operator+(double a, Dual b) { return {a + b.v, b.d}; }
QCDFT_XC_FN Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
QCDFT_XC_FN Dual operator-(Dual a, double b) { return {a.v - b, a.d}; }
QCDFT_XC_FN Dual operator-(double a, Dual b) { return {a - b.v, -b.d}; }
QCDFT_XC_FN Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
QCDFT_XC_FN Dual operator*(Dual a, double b) { return {a.v * b, a.d * b}; }
QCDFT_XC_FN Dual operator*(double a, Dual b) { return {a * b.v, a * b.d}; }
QCDFT_XC_FN Dual operator/(Dual a, Dual b) { const double q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
QCDFT_XC_FN Dual operator/(Dual a, double b) { return {a.v / b, a.d / b}; }
QCDFT_XC_FN Dual operator/(double a, Dual b) { const double q = a / b.v; return {q, -q * b.d / b.v}; }
QCDFT_XC_FN Dual &operator+=(Dual &a, Dual b) { a = a + b; return a; }
QCDFT_XC_FN Dual &operator*=(Dual &a, double b) { a = a * b; return a; }
QCDFT_XC_FN bool operator<(Dual a, double b) { return a.v < b; }
QCDFT_XC_FN bool operator>(Dual a, double b) { return a.v > b; }
QCDFT_XC_FN bool operator<(Dual a, Dual b) { return a.v < b.v; }
QCDFT_XC_FN bool operator>(Dual a, Dual b) { return a.v > b.v; }
using ::cbrt; using ::sqrt; using ::log; using ::exp; using ::expm1; using ::atan; using ::asinh; using ::fabs;   // beside the Dual overloads, for T = double
QCDFT_XC_FN Dual cbrt(Dual a) { const double r = ::cbrt(a.v); return {r, a.d * r / (3.0 * a.v)}; }
QCDFT_XC_FN Dual sqrt(Dual a) { const double r = ::sqrt(a.v); return {r, a.d / (2.0 * r)}; }
QCDFT_XC_FN Dual log(Dual a) { return {::log(a.v), a.d / a.v}; }
QCDFT_XC_FN Dual exp(Dual a) { const double e = ::exp(a.v); return {e, a.d * e}; }
QCDFT_XC_FN Dual expm1(Dual a) { return {::expm1(a.v), a.d * ::exp(a.v)}; }
QCDFT_XC_FN Dual atan(Dual a) { return {::atan(a.v), a.d / (1.0 + a.v * a.v)}; }
QCDFT_XC_FN Dual asinh(Dual a) { return {::asinh(a.v), a.d / ::sqrt(1.0 + a.v * a.v)}; }
QCDFT_XC_FN Dual fabs(Dual a) { return a.v < 0.0 ? Dual{-a.v, -a.d} : a; }

constexpr double kRhoCut = 1e-12;   // src/dft_solver.cu:12
constexpr double kSigmaCut = 1e-20; // src/dft_solver.cu:13
constexpr double kPi = 3.14159265358979323846;
constexpr double kCx = 0.7385587663820224;

template <class T> struct LdaT { T e, v; };
template <class T> struct GgaT { T e, vr, vs; };
using Lda = LdaT<double>;
using Gga = GgaT<double>;

// Slater exchange, src/dft_solver.cu:61-76 (both spellings give the same values).
template <class T>
QCDFT_XC_FN LdaT<T> slater_x(T rho)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    T e = -kCx * cbrt(rho);
    return {e, (4.0 / 3.0) * e};
}

// Shared VWN form: eps(x) and d eps/dx for parameters (A,b,c,x0).
// `with_atan_terms` = false reproduces src/dft_solver.cu:192-193.
template <class T>
QCDFT_XC_FN void vwn_form(T x, double A, double b, double c, double x0,
                          bool with_atan_terms, T &eps, T &deps_dx)
{
    const T X = x * x + b * x + c;
    const double Q = sqrt(4.0 * c - b * b);
    const double X0 = x0 * x0 + b * x0 + c;
    const T at = atan(Q / (2.0 * x + b));
    const T lg = log(x * x / X);
    const T lg0 = log((x - x0) * (x - x0) / X);
    const double w0 = b * x0 / X0;
    eps = A * (lg + (2.0 * b / Q) * at - w0 * (lg0 + (2.0 * (2.0 * x0 + b) / Q) * at));
    const T dl = 2.0 / x - (2.0 * x + b) / X;
    const T dl0 = 2.0 / (x - x0) - (2.0 * x + b) / X;
    if (with_atan_terms)
        deps_dx = A * (dl - b / X - w0 * (dl0 - (2.0 * x0 + b) / X));
    else
        deps_dx = A * (dl - w0 * dl0);
}

// VWN5 paramagnetic, src/dft_solver.cu:180-205 (parameters :21-24).
template <class T>
QCDFT_XC_FN LdaT<T> vwn5_c(T rho, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    const T rs = cbrt(3.0 / (4.0 * kPi * rho));
    const T x = sqrt(rs);
    T e, de;
    vwn_form(x, 0.0310907, 3.72744, 12.9352, -0.10498, !quirks, e, de);
    return {e, e - (rs / 3.0) * (de / (2.0 * x))};
}

// VWN-RPA as used by B3LYP, src/dft_solver.cu:106-138 (parameters :38-41).
template <class T>
QCDFT_XC_FN LdaT<T> vwn_rpa_c(T rho)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    const T rs = cbrt(3.0 / (4.0 * kPi * rho));
    const T x = sqrt(rs);
    T e, de;
    vwn_form(x, 0.0310907, 13.0720, 42.7198, -0.409286, true, e, de);
    return {e, e - (rs / 3.0) * (de / (2.0 * x))};
}

// PW92 (modified), src/dft_solver.cu:207-220 (parameters :25-31).
template <class T>
QCDFT_XC_FN LdaT<T> pw92_c(T rho)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    constexpr double A = 0.03109069086965489503;
    constexpr double a1 = 0.21370, b1 = 7.5957, b2 = 3.5876, b3 = 1.6382, b4 = 0.49294;
    const T rs = cbrt(3.0 / (4.0 * kPi * rho));
    const T sq = sqrt(rs);
    const T Q = 2.0 * A * (b1 * sq + b2 * rs + b3 * rs * sq + b4 * rs * rs);
    const T Qp = 2.0 * A * (0.5 * b1 / sq + b2 + 1.5 * b3 * sq + 2.0 * b4 * rs);
    const T lg = log(1.0 + 1.0 / Q);
    const T f = -2.0 * A * (1.0 + a1 * rs);
    const T e = f * lg;
    const T de = -2.0 * A * a1 * lg + f * (1.0 / (1.0 + 1.0 / Q)) * (-1.0 / (Q * Q)) * Qp;
    return {e, e - (rs / 3.0) * de};
}

// PBE exchange, src/dft_solver.cu:222-242.
template <class T>
QCDFT_XC_FN GgaT<T> pbe_x(T rho, T sigma)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0};
    constexpr double kappa = 0.804, mu = 0.2195149727645171;
    const T r13 = cbrt(rho);
    const T r43 = rho * r13;
    const T kF = cbrt(3.0 * kPi * kPi * rho);
    const T den = 4.0 * kF * kF * rho * rho;
    T s2 = 0.0;
    if (sigma > kSigmaCut && den > 1e-50) s2 = sigma / den;
    if (s2 > 1e12) s2 = 1e12;
    const T num = 1.0 + mu * s2 / kappa;
    const T F = 1.0 + kappa * (1.0 - 1.0 / num);
    const T e = -kCx * r13 * F;
    const T dF = mu / (num * num);
    GgaT<T> o;
    o.e = e;
    o.vs = (-kCx * r43) * dF * (1.0 / den);
    o.vr = (4.0 / 3.0) * e - (8.0 / 3.0) * (-kCx * r43) * s2 * dF / rho;
    return o;
}

// PBE correlation, src/dft_solver.cu:244-283.
// `l` = pw92_c(rho), so that a caller which needs PW92 on its own as well evaluates it once.
template <class T>
QCDFT_XC_FN GgaT<T> pbe_c_with(const LdaT<T> l, T rho, T sigma, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0};
    constexpr double beta = 0.066725, gamma = 0.03109069086965489503;
    const T kF = cbrt(3.0 * kPi * kPi * rho);
    const T den16 = 16.0 * kF * rho * rho;
    T t2 = 0.0;
    if (sigma > kSigmaCut && den16 > 1e-50) t2 = (sigma * kPi) / den16;
    if (t2 > 1.0e20) t2 = 1.0e20;
    const T x = -l.e / gamma;
    const T em1 = expm1(x);
    const T A = (fabs(em1) < 1e-20) ? T(1.0e20) : (beta / gamma) / em1;
    const T At2 = A * t2;
    const T num = 1.0 + At2;
    const T den = 1.0 + At2 + At2 * At2;
    const T Qr = num / den;
    const T tl = 1.0 + (beta / gamma) * t2 * Qr;
    const T H = gamma * log(tl);
    const T Qp = (den - num * (1.0 + 2.0 * At2)) / (den * den);
    const T pre = gamma / tl * (beta / gamma);
    const T dH_dt2 = pre * (Qr + At2 * Qp);
    const T dH_dA = pre * t2 * t2 * Qp;
    const T dt2_ds = (den16 > 1e-50) ? kPi / den16 : T(0.0);
    T dx_drho = (l.v - l.e) / (rho * gamma); // :277 as shipped
    if (!quirks) dx_drho = -dx_drho;              // x = -ec/gamma
    const T dA_drho = (-A * exp(x) / em1) * dx_drho;
    const T dt2_drho = t2 * (-7.0 / 3.0) / rho;
    GgaT<T> o;
    o.e = l.e + H;
    o.vs = rho * dH_dt2 * dt2_ds;
    o.vr = l.v + H + rho * (dH_dA * dA_drho + dH_dt2 * dt2_drho);
    return o;
}

template <class T>
QCDFT_XC_FN GgaT<T> pbe_c(T rho, T sigma, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0};
    return pbe_c_with(pw92_c(rho), rho, sigma, quirks);
}

// Becke-88 gradient correction, per-spin arguments, src/dft_solver.cu:78-104.
template <class T>
QCDFT_XC_FN GgaT<T> b88_x(T rho, T sigma)
{
    if (rho < kRhoCut || sigma < kSigmaCut) return {0.0, 0.0, 0.0};
    constexpr double beta = 0.0042; // :43
    const T r13 = cbrt(rho);
    const T r43 = rho * r13;
    const T g = sqrt(sigma);
    const T x = g / r43;
    const T x2 = x * x;
    const T as = asinh(x);
    const T den = 1.0 + 6.0 * beta * x * as;
    const T term = beta * x2 / den;
    const T dden = 6.0 * beta * (as + x / sqrt(1.0 + x2));
    const T dF = beta * (2.0 * x * den - x2 * dden) / (den * den);
    const T dE = r43 * (-dF);
    GgaT<T> o;
    o.e = -term * r13;
    o.vs = dE * (1.0 / (2.0 * r43 * g));
    o.vr = (4.0 / 3.0) * ((r43 * (-term)) / rho) - (4.0 / 3.0) * dE * (x / rho);
    return o;
}

// Closed-shell LYP, src/dft_solver.cu:140-178 (constants :45-49).
template <class T>
QCDFT_XC_FN GgaT<T> lyp_c(T rho, T sigma)
{
    if (rho < 1e-14) return {0.0, 0.0, 0.0};
    constexpr double a = 0.04918, b = 0.132, c = 0.2533, d = 0.349;
    constexpr double CF = 2.87123400018819108;
    const T rm13 = 1.0 / cbrt(rho);
    const T rm53 = rm13 * rm13 * rm13 * rm13 * rm13;
    const T ev = exp(-c * rm13);
    const T den = 1.0 + d * rm13;
    const T di = 1.0 / den;
    const T G = ev * di;
    const T delta = c * rm13 + d * rm13 * di;
    const T gb = 3.0 + 7.0 * delta;
    const double k72 = a * b / 72.0;
    const T H = -a * rho * di - a * b * CF * rho * G + k72 * sigma * rm53 * G * gb;
    const T d_rm13 = -(1.0 / 3.0) * rm13 / rho;
    const T d_den = d * d_rm13;
    const T d_G = G * delta / (3.0 * rho);
    const T d_delta = c * d_rm13 + d * (d_rm13 * di - rm13 * di * di * d_den);
    const T d_H1 = -a * (den - rho * d_den) * (di * di);
    const T d_H2a = -a * b * CF * (G + rho * d_G);
    const T tdv = (-5.0 / (3.0 * rho)) * gb + (delta / (3.0 * rho)) * gb + 7.0 * d_delta;
    GgaT<T> o;
    o.e = H / rho;
    o.vr = d_H1 + d_H2a + k72 * sigma * (rm53 * G) * tdv;
    o.vs = k72 * rm53 * G * gb;
    return o;
}

// What one grid point contributes: the energy density rho*eps and the four
// coefficients of B[g,:] = c0*phi + c1*dphi/dx + c2*dphi/dy + c3*dphi/dz.
template <class T> struct PointXCT { T exc, c0, c1, c2, c3; };
using PointXC = PointXCT<double>;

// lda_fused_kernel body, src/dft_solver.cu:317-342.
template <class T>
QCDFT_XC_FN PointXCT<T> lda_point(T rho, double w, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0, 0.0, 0.0};
    const LdaT<T> x = slater_x(rho), c = vwn5_c(rho, quirks);
    return {rho * (x.e + c.e), w * (x.v + c.v), 0.0, 0.0, 0.0};
}

// gga_fused_kernel body, src/dft_solver.cu:391-430 (factor 4 at :429).
template <class T>
QCDFT_XC_FN PointXCT<T> gga_point(T rho, T sigma, T gx, T gy, T gz, double w, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0, 0.0, 0.0};
    const GgaT<T> x = pbe_x(rho, sigma), c = pbe_c(rho, sigma, quirks);
    const T f = w * 4.0 * (x.vs + c.vs);
    return {rho * (x.e + c.e), w * (x.vr + c.vr), f * gx, f * gy, f * gz};
}

// b3lyp_fused_kernel body, src/dft_solver.cu:444-511 (mixing :33-36, the 0.5
// of :468 and :492, factor 2 at :510).
template <class T>
QCDFT_XC_FN PointXCT<T> b3lyp_point(T rho, T sigma, T gx, T gy, T gz, double w)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0, 0.0, 0.0};
    constexpr double cL = 0.80, cB = 0.72, cV = 0.19, cY = 0.81;
    const LdaT<T> xl = slater_x(rho);
    GgaT<T> xb = b88_x(0.5 * rho, 0.25 * sigma);
    xb.vs *= 0.5;
    const LdaT<T> cv = vwn_rpa_c(rho);
    const GgaT<T> cy = lyp_c(rho, sigma);
    const T eps = cL * xl.e + cB * xb.e + cV * cv.e + cY * cy.e;
    const T vr = 0.5 * (cL * xl.v + cB * xb.vr + cV * cv.v + cY * cy.vr);
    const T f = w * 2.0 * (cB * xb.vs + cY * cy.vs);
    return {rho * eps, w * vr, f * gx, f * gy, f * gz};
}

// A weighted sum of the eight components above (solver type SOLVER_MIX; order = enum XCComponent of
// include/dft_solver.h).  GGA convention whatever the components: vrho whole, factor 4 on vsigma, a one-sided
// matrix that the caller averages with its transpose -- so (V + V^T)/2 with B3LYP's four coefficients is what
// b3lyp_point's halved vrho, factor 2 and M + M^T give.  B88 enters in its closed-shell form, as in b3lyp_point.
// The weights are kernel arguments, the same for every lane: a zero weight is a scalar branch around the whole
// component (PBE0 pays for no exp of LYP, no atan / log of VWN).  GGA = false: components 4..7 are not looked at.
struct MixWeights { double c[8]; };

template <bool GGA, class T>
QCDFT_XC_FN PointXCT<T> mix_point(const MixWeights &m, T rho, T sigma, T gx, T gy, T gz, double w, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0, 0.0, 0.0, 0.0};
    T e = 0.0, vr = 0.0, vs = 0.0;
    if (m.c[0] != 0.0) { const LdaT<T> x = slater_x(rho);       e += m.c[0] * x.e; vr += m.c[0] * x.v; }
    if (m.c[1] != 0.0) { const LdaT<T> x = vwn5_c(rho, quirks); e += m.c[1] * x.e; vr += m.c[1] * x.v; }
    if (m.c[2] != 0.0) { const LdaT<T> x = vwn_rpa_c(rho);      e += m.c[2] * x.e; vr += m.c[2] * x.v; }
    const bool with_pbe_c = GGA && m.c[5] != 0.0;
    if (m.c[3] != 0.0 || with_pbe_c) {
        const LdaT<T> l = pw92_c(rho);                          // once for PW92 itself and inside PBE correlation
        if (m.c[3] != 0.0) { e += m.c[3] * l.e; vr += m.c[3] * l.v; }
        if (with_pbe_c) { const GgaT<T> x = pbe_c_with(l, rho, sigma, quirks); e += m.c[5] * x.e; vr += m.c[5] * x.vr; vs += m.c[5] * x.vs; }
    }
    if (GGA) {
        if (m.c[4] != 0.0) { const GgaT<T> x = pbe_x(rho, sigma); e += m.c[4] * x.e; vr += m.c[4] * x.vr; vs += m.c[4] * x.vs; }
        if (m.c[6] != 0.0) { const GgaT<T> x = b88_x(0.5 * rho, 0.25 * sigma); e += m.c[6] * x.e; vr += m.c[6] * x.vr; vs += m.c[6] * (0.5 * x.vs); }
        if (m.c[7] != 0.0) { const GgaT<T> x = lyp_c(rho, sigma); e += m.c[7] * x.e; vr += m.c[7] * x.vr; vs += m.c[7] * x.vs; }
    }
    const T f = w * 4.0 * vs;
    return {rho * e, w * vr, f * gx, f * gy, f * gz};
}

// The two scalars of a point body without the weight, the gradient and the energy: c0 = w P, c_k = w Q g_k.  P and Q
// are the same sums the *_point bodies above multiply into c0..c3 (their factors 4 and 2 are powers of two, so w Q is
// bit for bit the body's w * 4 * vs; tests/test_fxc_cpu.py holds the two against each other).  With T = Dual these are
// what the linear response of Vxc differentiates.  An LDA-class body has Q = 0.
template <class T> struct PQT { T p, q; };

template <class T>
QCDFT_XC_FN PQT<T> lda_pq(T rho, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    const LdaT<T> x = slater_x(rho), c = vwn5_c(rho, quirks);
    return {x.v + c.v, 0.0};
}

template <class T>
QCDFT_XC_FN PQT<T> gga_pq(T rho, T sigma, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    const GgaT<T> x = pbe_x(rho, sigma), c = pbe_c(rho, sigma, quirks);
    return {x.vr + c.vr, 4.0 * (x.vs + c.vs)};
}

template <class T>
QCDFT_XC_FN PQT<T> b3lyp_pq(T rho, T sigma)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    constexpr double cL = 0.80, cB = 0.72, cV = 0.19, cY = 0.81;
    const LdaT<T> xl = slater_x(rho);
    GgaT<T> xb = b88_x(0.5 * rho, 0.25 * sigma);
    xb.vs *= 0.5;
    const LdaT<T> cv = vwn_rpa_c(rho);
    const GgaT<T> cy = lyp_c(rho, sigma);
    return {0.5 * (cL * xl.v + cB * xb.vr + cV * cv.v + cY * cy.vr), 2.0 * (cB * xb.vs + cY * cy.vs)};
}

template <bool GGA, class T>
QCDFT_XC_FN PQT<T> mix_pq(const MixWeights &m, T rho, T sigma, bool quirks)
{
    if (rho < kRhoCut) return {0.0, 0.0};
    T vr = 0.0, vs = 0.0;
    if (m.c[0] != 0.0) { const LdaT<T> x = slater_x(rho);       vr += m.c[0] * x.v; }
    if (m.c[1] != 0.0) { const LdaT<T> x = vwn5_c(rho, quirks); vr += m.c[1] * x.v; }
    if (m.c[2] != 0.0) { const LdaT<T> x = vwn_rpa_c(rho);      vr += m.c[2] * x.v; }
    const bool with_pbe_c = GGA && m.c[5] != 0.0;
    if (m.c[3] != 0.0 || with_pbe_c) {
        const LdaT<T> l = pw92_c(rho);
        if (m.c[3] != 0.0) vr += m.c[3] * l.v;
        if (with_pbe_c) { const GgaT<T> x = pbe_c_with(l, rho, sigma, quirks); vr += m.c[5] * x.vr; vs += m.c[5] * x.vs; }
    }
    if (GGA) {
        if (m.c[4] != 0.0) { const GgaT<T> x = pbe_x(rho, sigma); vr += m.c[4] * x.vr; vs += m.c[4] * x.vs; }
        if (m.c[6] != 0.0) { const GgaT<T> x = b88_x(0.5 * rho, 0.25 * sigma); vr += m.c[6] * x.vr; vs += m.c[6] * (0.5 * x.vs); }
        if (m.c[7] != 0.0) { const GgaT<T> x = lyp_c(rho, sigma); vr += m.c[7] * x.vr; vs += m.c[7] * x.vs; }
    }
    return {vr, 4.0 * vs};
}

} // namespace xc
} // namespace qcdft
