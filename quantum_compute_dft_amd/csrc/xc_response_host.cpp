// Host counterpart of xc_response.hip and xc_response_pol.hip (lib/libqcfxc.so, built with g++): the same bodies of xc_functionals.hpp,
// the same two dual evaluations per point.  response.fxc_apply_host() and a CPU CPKS run assemble V1 from it; the CPU
// tests hold it against finite differences of the oracle.  type: 0 LDA, 1 GGA, 2 B3LYP, 3 mix (eight weights).
#include "xc_functionals.hpp"
#include "xc_spin_functionals.hpp"
#include "xc_meta_functionals.hpp"

using namespace qcdft;

namespace {

xc::MixWeights weights(const double *mix8)
{
    xc::MixWeights m = {};
    if (mix8)
        for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    return m;
}

bool mix_gga(const xc::MixWeights &m)
{
    return m.c[4] != 0.0 || m.c[5] != 0.0 || m.c[6] != 0.0 || m.c[7] != 0.0;
}

template <class T>
xc::PQT<T> pq(int type, const xc::MixWeights &m, bool gga, T r, T s, bool quirks)
{
    if (type == 0) return xc::lda_pq(r, quirks);
    if (type == 1) return xc::gga_pq(r, s, quirks);
    if (type == 2) return xc::b3lyp_pq(r, s);
    return gga ? xc::mix_pq<true>(m, r, s, quirks) : xc::mix_pq<false>(m, r, s, quirks);
}

} // namespace

extern "C" {

// out (5, n): P_rho, P_sigma, Q_rho, Q_sigma, Q (no weight).  An LDA-class functional leaves planes 1..4 zero.
int qc_fxc_table(int type, const double *mix8, int quirks, long long n, const double *rho, const double *sigma, double *out)
{
    if (type < 0 || type > 3 || (type == 3 && !mix8) || n < 0 || !rho || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const bool gga = type == 1 || type == 2 || (type == 3 && mix_gga(m));
    if (gga && !sigma) return -1;
    for (long long g = 0; g < n; ++g) {
        const double r = rho[g], s = gga ? sigma[g] : 0.0;
        const xc::PQT<xc::Dual> a = pq(type, m, gga, xc::Dual(r, 1.0), xc::Dual(s, 0.0), quirks != 0);
        out[g] = a.p.d;
        out[2 * n + g] = a.q.d;
        out[4 * n + g] = a.q.v;
        if (gga) {
            const xc::PQT<xc::Dual> b = pq(type, m, gga, xc::Dual(r, 0.0), xc::Dual(s, 1.0), quirks != 0);
            out[n + g] = b.p.d;
            out[3 * n + g] = b.q.d;
        } else {
            out[n + g] = 0.0;
            out[3 * n + g] = 0.0;
        }
    }
    return 0;
}

// out (2, n): P, Q evaluated in double, and the value parts of the dual evaluation in out_dual (2, n).
int qc_fxc_pq(int type, const double *mix8, int quirks, long long n, const double *rho, const double *sigma, double *out,
              double *out_dual)
{
    if (type < 0 || type > 3 || (type == 3 && !mix8) || n < 0 || !rho || !sigma || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const bool gga = type == 1 || type == 2 || (type == 3 && mix_gga(m));
    for (long long g = 0; g < n; ++g) {
        const xc::PQT<double> a = pq(type, m, gga, rho[g], sigma[g], quirks != 0);
        out[g] = a.p;
        out[n + g] = a.q;
        if (out_dual) {
            const xc::PQT<xc::Dual> d = pq(type, m, gga, xc::Dual(rho[g], 1.0), xc::Dual(sigma[g], 0.5), quirks != 0);
            out_dual[g] = d.p.v;
            out_dual[n + g] = d.q.v;
        }
    }
    return 0;
}

// out (5, n): exc, c0..c3 of the point bodies the kernels run (lda_point / gga_point / b3lyp_point / mix_point), in double.
int qc_xc_point(int type, const double *mix8, int quirks, long long n, const double *rho, const double *sigma,
                const double *grad3, const double *w, double *out)
{
    if (type < 0 || type > 3 || (type == 3 && !mix8) || n < 0 || !rho || !sigma || !grad3 || !w || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const bool gga = mix_gga(m);
    for (long long g = 0; g < n; ++g) {
        const double gx = grad3[3 * g], gy = grad3[3 * g + 1], gz = grad3[3 * g + 2];
        xc::PointXC p;
        if (type == 0)      p = xc::lda_point(rho[g], w[g], quirks != 0);
        else if (type == 1) p = xc::gga_point(rho[g], sigma[g], gx, gy, gz, w[g], quirks != 0);
        else if (type == 2) p = xc::b3lyp_point(rho[g], sigma[g], gx, gy, gz, w[g]);
        else if (gga)       p = xc::mix_point<true>(m, rho[g], sigma[g], gx, gy, gz, w[g], quirks != 0);
        else                p = xc::mix_point<false>(m, rho[g], 0.0, 0.0, 0.0, 0.0, w[g], quirks != 0);
        out[g] = p.exc;
        out[n + g] = p.c0;
        out[2 * n + g] = p.c1;
        out[3 * n + g] = p.c2;
        out[4 * n + g] = p.c3;
    }
    return 0;
}

// The table of the spin-resolved energy bodies, out (5, n) in the layout of qc_fxc_table (no weight): kind 1 the
// spin-flip (triplet) response, kind 2 the singlet response through the same bodies.  A built-in type enters as its
// component weights and its factor, as in launch_fxc_table_spin.  No `quirks`: a derivative of the energy.
int qc_fxc_table_spin(int type, const double *mix8, int kind, long long n, const double *rho, const double *sigma, double *out)
{
    if (type < 0 || type > 3 || (type == 3 && !mix8) || (kind != 1 && kind != 2) || n < 0 || !rho || !out) return -1;
    xc::MixWeights m = weights(mix8);
    const double scale = type == 3 ? 1.0 : xc::builtin_spin_mix(type, m);
    const bool gga = mix_gga(m);
    if (gga && !sigma) return -1;
    for (long long g = 0; g < n; ++g) {
        double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (gga) xc::spin_table_point<true>(m, kind, 15, rho[g], sigma[g], scale, t, t + 1, t + 2, t + 3, t + 4);
        else     xc::spin_table_point<false>(m, kind, 15, rho[g], 0.0, scale, t, t + 1, t + 2, t + 3, t + 4);
        for (int k = 0; k < 5; ++k) out[k * n + g] = t[k];
    }
    return 0;
}

// The table of the open-shell response (k_fxc_table_pol of xc_response_pol.hip) at any polarisation,
// bare: no weight and no factor of the built-in type.  h (25, n): H_ij = d^2 e / dx_i dx_j at row 5 i + j, x = (ra, rb,
// saa, sab, sbb), every ordered pair evaluated with x_i first (the two orders differ only at a sigma cut-off); g1 (5, n):
// de / dx_i.  ga3 / gb3: three per point, interleaved (may be null for an LDA-class functional, whose sigma rows and
// columns stay zero).  An absent channel (density below the cut-off): zeros in its rows, columns and g.
int qc_fxc_table_pol(int type, const double *mix8, long long n, const double *ra, const double *rb, const double *ga3,
                     const double *gb3, double *h, double *g1)
{
    if (type < 0 || type > 3 || (type == 3 && !mix8) || n < 0 || !ra || !rb || !h || !g1) return -1;
    xc::MixWeights m = weights(mix8);
    if (type != 3) (void)xc::builtin_spin_mix(type, m);
    const bool gga = mix_gga(m);
    if (gga && (!ga3 || !gb3)) return -1;
    const int nv = gga ? 5 : 2;
    for (long long k = 0; k < 25 * n; ++k) h[k] = 0.0;
    for (long long k = 0; k < 5 * n; ++k) g1[k] = 0.0;
    for (long long g = 0; g < n; ++g) {
        const xc::SpinVars x = gga ? xc::spin_vars<true>(ra[g], rb[g], ga3[3 * g], ga3[3 * g + 1], ga3[3 * g + 2], gb3[3 * g],
                                                         gb3[3 * g + 1], gb3[3 * g + 2])
                                   : xc::spin_vars<false>(ra[g], rb[g], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
        for (int i = 0; i < nv; ++i)
            for (int j = 0; j < nv; ++j) {
                double hij, gi;
                if (gga) xc::spin_hessian_entry<true>(m, x, i, j, &hij, &gi);
                else     xc::spin_hessian_entry<false>(m, x, i, j, &hij, &gi);
                h[(5 * i + j) * n + g] = hij;
                if (i == j) g1[i * n + g] = gi;
            }
    }
    return 0;
}

// out (n): the energy per volume of the eight weights at any (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb).
int qc_spin_energy(const double *mix8, long long n, const double *ra, const double *rb, const double *saa, const double *sab,
                   const double *sbb, double *out)
{
    if (!mix8 || n < 0 || !ra || !rb || !saa || !sab || !sbb || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const bool gga = mix_gga(m);
    for (long long g = 0; g < n; ++g)
        out[g] = gga ? xc::spin_mix_energy<true>(m, ra[g], rb[g], saa[g], sab[g], sbb[g])
                     : xc::spin_mix_energy<false>(m, ra[g], rb[g], 0.0, 0.0, 0.0);
    return 0;
}

// One point of the spin-resolved sweep, xc::spin_potential_point as k_xc_points_spin runs it (a built-in type enters as
// its component weights and its factor, as in launch_xc_points_spin).  ga3 / gb3: three per point, interleaved (may be
// null for an LDA-class functional).  out (14, n): e (no weight); c0..c3 of alpha; c0..c3 of beta; the bare derivatives
// of e by rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb (zero for an absent channel).
int qc_xc_point_spin(int type, const double *mix8, long long n, const double *ra, const double *rb, const double *ga3,
                     const double *gb3, const double *w, double *out)
{
    if (type < 0 || type > 3 || (type == 3 && !mix8) || n < 0 || !ra || !rb || !w || !out) return -1;
    xc::MixWeights m = weights(mix8);
    const double scale = type == 3 ? 1.0 : xc::builtin_spin_mix(type, m);
    const bool gga = mix_gga(m);
    if (gga && (!ga3 || !gb3)) return -1;
    for (long long g = 0; g < n; ++g) {
        xc::SpinPoint p;
        if (gga)
            p = xc::spin_potential_point<true>(m, ra[g], rb[g], ga3[3 * g], ga3[3 * g + 1], ga3[3 * g + 2], gb3[3 * g],
                                               gb3[3 * g + 1], gb3[3 * g + 2], w[g], scale);
        else
            p = xc::spin_potential_point<false>(m, ra[g], rb[g], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, w[g], scale);
        out[g] = p.e;
        for (int k = 0; k < 4; ++k) {
            out[(1 + k) * n + g] = p.a[k];
            out[(5 + k) * n + g] = p.b[k];
        }
        for (int k = 0; k < 5; ++k) out[(9 + k) * n + g] = p.d[k];
    }
    return 0;
}

// One closed-shell point of the meta-GGA sweep, xc::meta_point as k_xc_points_meta runs it: the eight weights, the two
// meta weights, grad3 three per point (interleaved).  out (10, n): e (no weight); c0..c3; ct; e_rho, e_sigma, e_tau (bare).
int qc_meta_point(const double *mix8, const double *meta2, long long n, const double *rho, const double *grad3, const double *tau,
                  const double *w, double *out)
{
    if (!mix8 || !meta2 || n < 0 || !rho || !grad3 || !tau || !w || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    for (long long g = 0; g < n; ++g) {
        const xc::MetaPoint p = xc::meta_point(m, mm, rho[g], grad3[3 * g], grad3[3 * g + 1], grad3[3 * g + 2], tau[g], w[g]);
        out[g] = p.e;
        for (int k = 0; k < 4; ++k) out[(1 + k) * n + g] = p.c[k];
        out[5 * n + g] = p.ct;
        for (int k = 0; k < 3; ++k) out[(6 + k) * n + g] = p.d[k];
    }
    return 0;
}

// One point of the spin-resolved meta-GGA sweep, xc::meta_spin_point as k_xc_points_meta_spin runs it.  ga3 / gb3: three per
// point, interleaved.  out (18, n): e (no weight); c0..c3 of alpha; c0..c3 of beta; ct of alpha, of beta; the bare
// derivatives of e by rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb, tau_a, tau_b (zero for an absent channel).
int qc_meta_point_spin(const double *mix8, const double *meta2, long long n, const double *ra, const double *rb, const double *ga3,
                       const double *gb3, const double *ta, const double *tb, const double *w, double *out)
{
    if (!mix8 || !meta2 || n < 0 || !ra || !rb || !ga3 || !gb3 || !ta || !tb || !w || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    for (long long g = 0; g < n; ++g) {
        const xc::MetaSpinPoint p = xc::meta_spin_point(m, mm, ra[g], rb[g], ga3[3 * g], ga3[3 * g + 1], ga3[3 * g + 2], gb3[3 * g],
                                                        gb3[3 * g + 1], gb3[3 * g + 2], ta[g], tb[g], w[g]);
        out[g] = p.e;
        for (int k = 0; k < 4; ++k) {
            out[(1 + k) * n + g] = p.a[k];
            out[(5 + k) * n + g] = p.b[k];
        }
        out[9 * n + g] = p.cta;
        out[10 * n + g] = p.ctb;
        for (int k = 0; k < 7; ++k) out[(11 + k) * n + g] = p.d[k];
    }
    return 0;
}

// The energy per volume of the ten weights at any (rho_a, rho_b, sigma_aa, sigma_ab, sigma_bb, tau_a, tau_b) into out (n),
// and (grad non-null) its seven first derivatives into grad (7, n) by xc::Dual.  A variable of an absent channel (density
// below the cut-off; sigma_ab belongs to both) is not differentiated: its derivative is exactly 0, as in spin_potential_point.
int qc_meta_energy_spin(const double *mix8, const double *meta2, long long n, const double *ra, const double *rb, const double *saa,
                        const double *sab, const double *sbb, const double *ta, const double *tb, double *out, double *grad)
{
    if (!mix8 || !meta2 || n < 0 || !ra || !rb || !saa || !sab || !sbb || !ta || !tb || !out) return -1;
    const xc::MixWeights m = weights(mix8);
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    for (long long g = 0; g < n; ++g) {
        const double x[7] = {ra[g], rb[g], saa[g], sab[g], sbb[g], ta[g], tb[g]};
        out[g] = xc::meta_mix_energy<false>(m, mm, x[0], x[1], x[2], x[3], x[4], x[5], x[6]);
        if (!grad) continue;
        const bool pa = x[0] >= xc::kRhoCut, pb = x[1] >= xc::kRhoCut;
        const bool present[7] = {pa, pb, pa, pa && pb, pb, pa, pb};
        for (int i = 0; i < 7; ++i) {
            grad[i * n + g] = 0.0;
            if (!present[i]) continue;
            xc::Dual v[7];
            for (int k = 0; k < 7; ++k) v[k] = xc::Dual(x[k], k == i ? 1.0 : 0.0);
            grad[i * n + g] = xc::meta_mix_energy<false>(m, mm, v[0], v[1], v[2], v[3], v[4], v[5], v[6]).d;
        }
    }
    return 0;
}

} // extern "C"
