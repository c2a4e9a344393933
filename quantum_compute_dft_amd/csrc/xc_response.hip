// Pointwise part of the linear response of Vxc (DFT_FxcPrepare / DFT_FxcApply, dft_api.hip).
//
// With c0 = w P(rho, sigma) and c_k = w Q(rho, sigma) g_k the coefficients k_xc_points hands to the Vxc kernels
// (P, Q: xc::*_pq, the scalars of the point bodies), a perturbation (rho1, g1) of the density changes them by
//
//     sigma1 = 2 g . g1
//     c0'  = w (P_rho rho1 + P_sigma sigma1)
//     c_k' = w [(Q_rho rho1 + Q_sigma sigma1) g_k + Q g1_k]
//
// k_fxc_table evaluates the five weighted scalars once per ground state, by pushing xc::Dual through the shipped
// bodies in the directions (1, 0) and (0, 1) of (rho, sigma) -- one after the other, so that one evaluation's
// registers are live at a time; k_fxc_coef is the arithmetic above per perturbation.  Everything else of the
// response (densities of dm1, contraction with the AO planes, slab reduce) is the ground-state sweep's kernels.
#include "xc_functionals.hpp"
#include "xc_spin_functionals.hpp"
#include "xc_response_launch.hpp"

namespace qcdft {

namespace {

template <int TYPE>
__device__ __forceinline__ xc::PQT<xc::Dual> fxc_eval(xc::Dual r, xc::Dual s, bool quirks)
{
    if (TYPE == 0) return xc::lda_pq(r, quirks);
    if (TYPE == 1) return xc::gga_pq(r, s, quirks);
    return xc::b3lyp_pq(r, s);
}

} // namespace

// TYPE 0 LDA (one plane), 1 GGA(PBE), 2 B3LYP.  A point below the density cut-off leaves zeros (the bodies return
// constants there).
template <int TYPE>
__global__ __launch_bounds__(256) void k_fxc_table(long ngrid, const double *__restrict__ rho,
                                                   const double *__restrict__ sigma,
                                                   const double *__restrict__ w, double *__restrict__ table,
                                                   int quirks)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const double wt = w[g], r = rho[g];
    const size_t n = (size_t)ngrid;
    if (TYPE == 0) {
        const xc::PQT<xc::Dual> a = fxc_eval<0>(xc::Dual(r, 1.0), xc::Dual(0.0), quirks != 0);
        table[g] = wt * a.p.d;
        return;
    }
    const double s = sigma[g];
    {
        const xc::PQT<xc::Dual> a = fxc_eval<TYPE>(xc::Dual(r, 1.0), xc::Dual(s, 0.0), quirks != 0);
        table[g] = wt * a.p.d;
        table[2 * n + g] = wt * a.q.d;
        table[4 * n + g] = wt * a.q.v;
    }
    {
        const xc::PQT<xc::Dual> a = fxc_eval<TYPE>(xc::Dual(r, 0.0), xc::Dual(s, 1.0), quirks != 0);
        table[n + g] = wt * a.p.d;
        table[3 * n + g] = wt * a.q.d;
    }
}

// SOLVER_MIX: the same around xc::mix_pq; the weights travel by value, as in k_xc_points_mix.
template <bool GGA>
__global__ __launch_bounds__(256) void k_fxc_table_mix(long ngrid, const double *__restrict__ rho,
                                                       const double *__restrict__ sigma,
                                                       const double *__restrict__ w, double *__restrict__ table,
                                                       int quirks, xc::MixWeights m)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const double wt = w[g], r = rho[g];
    const size_t n = (size_t)ngrid;
    if (!GGA) {
        const xc::PQT<xc::Dual> a = xc::mix_pq<false>(m, xc::Dual(r, 1.0), xc::Dual(0.0), quirks != 0);
        table[g] = wt * a.p.d;
        return;
    }
    const double s = sigma[g];
    {
        const xc::PQT<xc::Dual> a = xc::mix_pq<true>(m, xc::Dual(r, 1.0), xc::Dual(s, 0.0), quirks != 0);
        table[g] = wt * a.p.d;
        table[2 * n + g] = wt * a.q.d;
        table[4 * n + g] = wt * a.q.v;
    }
    {
        const xc::PQT<xc::Dual> a = xc::mix_pq<true>(m, xc::Dual(r, 0.0), xc::Dual(s, 1.0), quirks != 0);
        table[n + g] = wt * a.p.d;
        table[3 * n + g] = wt * a.q.d;
    }
}

// The table of the spin-resolved energy bodies (xc_spin_functionals.hpp) in the same five planes, for k_fxc_coef as it
// stands: kind 1 the spin-flip (triplet) response of the alpha potential, kind 2 the singlet response through the same
// bodies (equal to k_fxc_table's at quirks = 0).  Second derivatives of the ENERGY by xc::Dual2, one evaluation live at
// a time; WHICH (a bit per evaluation) spreads the evaluations over launches, each with its own register budget.  Built-in types arrive
// as their component weights and `scale` (B3LYP: 1/2, its M + M^T convention).
template <bool GGA, int WHICH>
__global__ __launch_bounds__(256) void k_fxc_table_spin(long ngrid, const double *__restrict__ rho,
                                                        const double *__restrict__ sigma,
                                                        const double *__restrict__ w, double *__restrict__ table,
                                                        int kind, double scale, xc::MixWeights m)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const size_t n = (size_t)ngrid;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
    xc::spin_table_point<GGA>(m, kind, WHICH, rho[g], GGA ? sigma[g] : 0.0, scale * w[g], &t0, &t1, &t2, &t3, &t4);
    if (WHICH & 1) table[g] = t0;
    if (!GGA) return;
    if (WHICH & 2) {
        table[2 * n + g] = t2;
        table[4 * n + g] = t4;
    }
    if (WHICH & 4) table[3 * n + g] = t3;
    if (WHICH & 8) table[n + g] = t1;
}

// Arithmetic only.  g0 / g1: three per point, interleaved (what the density kernels write).
template <bool GGA>
__global__ __launch_bounds__(256) void k_fxc_coef(long ngrid, const double *__restrict__ table,
                                                  const double *__restrict__ g0, const double *__restrict__ rho1,
                                                  const double *__restrict__ g1, double *__restrict__ coef)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const size_t n = (size_t)ngrid;
    const double r1 = rho1[g];
    if (!GGA) {
        coef[g] = table[g] * r1;
        return;
    }
    const double ax = g0[3 * g], ay = g0[3 * g + 1], az = g0[3 * g + 2];
    const double bx = g1[3 * g], by = g1[3 * g + 1], bz = g1[3 * g + 2];
    const double s1 = 2.0 * (ax * bx + ay * by + az * bz);
    const double q = table[4 * n + g];
    const double f = table[2 * n + g] * r1 + table[3 * n + g] * s1;
    coef[g] = table[g] * r1 + table[n + g] * s1;
    coef[n + g] = f * ax + q * bx;
    coef[2 * n + g] = f * ay + q * by;
    coef[3 * n + g] = f * az + q * bz;
}

hipError_t launch_fxc_table(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho,
                            const double *sigma, const double *w, double *table, int quirks)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    if (type == 0)      hipLaunchKernelGGL(k_fxc_table<0>, g, b, 0, st, ngrid, rho, sigma, w, table, quirks);
    else if (type == 1) hipLaunchKernelGGL(k_fxc_table<1>, g, b, 0, st, ngrid, rho, sigma, w, table, quirks);
    else if (type == 2) hipLaunchKernelGGL(k_fxc_table<2>, g, b, 0, st, ngrid, rho, sigma, w, table, quirks);
    else {
        xc::MixWeights m;
        for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
        if (gga) hipLaunchKernelGGL(k_fxc_table_mix<true>, g, b, 0, st, ngrid, rho, sigma, w, table, quirks, m);
        else     hipLaunchKernelGGL(k_fxc_table_mix<false>, g, b, 0, st, ngrid, rho, sigma, w, table, quirks, m);
    }
    return hipGetLastError();
}

hipError_t launch_fxc_table_spin(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho,
                                 const double *sigma, const double *w, double *table, int kind)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    xc::MixWeights m;
    double scale = 1.0;
    if (type == 3) for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    else           scale = xc::builtin_spin_mix(type, m);
    if (!gga) {
        hipLaunchKernelGGL((k_fxc_table_spin<false, 1>), g, b, 0, st, ngrid, rho, sigma, w, table, kind, scale, m);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_fxc_table_spin<true, 1>), g, b, 0, st, ngrid, rho, sigma, w, table, kind, scale, m);
    hipLaunchKernelGGL((k_fxc_table_spin<true, 2>), g, b, 0, st, ngrid, rho, sigma, w, table, kind, scale, m);
    hipLaunchKernelGGL((k_fxc_table_spin<true, 4>), g, b, 0, st, ngrid, rho, sigma, w, table, kind, scale, m);
    hipLaunchKernelGGL((k_fxc_table_spin<true, 8>), g, b, 0, st, ngrid, rho, sigma, w, table, kind, scale, m);
    return hipGetLastError();
}

hipError_t launch_fxc_coef(hipStream_t st, bool gga, long ngrid, const double *table, const double *g0,
                           const double *rho1, const double *g1, double *coef)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    if (gga) hipLaunchKernelGGL(k_fxc_coef<true>, g, b, 0, st, ngrid, table, g0, rho1, g1, coef);
    else     hipLaunchKernelGGL(k_fxc_coef<false>, g, b, 0, st, ngrid, table, g0, rho1, g1, coef);
    return hipGetLastError();
}

} // namespace qcdft
