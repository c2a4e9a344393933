// Pointwise part of the open-shell linear response of Vxc (DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol, dft_api.hip).
//
// DFT_ComputeXCSpin contracts, per spin s (s' the other one), c0_s = scale w g_{rho_s} and
// c_s,k = 2 scale w (2 g_{sigma_ss} grad rho_s + g_{sigma_ab} grad rho_s')_k with the AO planes, g_i = de/dx_i of
// xc::spin_mix_energy at x = (ra, rb, saa, sab, sbb) (xc::spin_potential_point).  A perturbation (ra1, grad ra1, rb1,
// grad rb1) of the two densities moves x by
//
//     x1 = (ra1, rb1, 2 grad ra . grad ra1, grad ra . grad rb1 + grad rb . grad ra1, 2 grad rb . grad rb1)
//
// and the coefficients by, with t_i = sum_j H_ij x1_j and H_ij = d g_i / d x_j,
//
//     c0_a' = t_0                       c0_b' = t_1
//     c_a,k' = 2 [2 t_2 grad ra + 2 g_2 grad ra1 + t_3 grad rb + g_3 grad rb1]_k
//     c_b,k' = 2 [2 t_4 grad rb + 2 g_4 grad rb1 + t_3 grad ra + g_3 grad ra1]_k
//
// k_fxc_table_pol evaluates scale w H and scale w g once per ground state: xc::Dual2 through the shipped energy bodies
// (xc::spin_hessian_entry), nothing differentiated by hand, one evaluation's registers live at a time; WHICH (a bit per
// pair of the upper triangle, in plane order, then a bit per pair in the other order) spreads the evaluations over
// launches, each instantiation with its own register budget and none with scratch.  k_fxc_coef_pol is the arithmetic above per perturbation.
//
// Planes (SoA, ngrid each).  LDA-class: H_00, H_01, H_11.  Gradient functionals: 0..14 the upper triangle H_ij (i <= j)
// row by row, first direction x_i; 15..17 g_2, g_3, g_4; 18..27 H_ji for the ten pairs i < j in the same order, first
// direction x_j.  The last ten are extra planes for the sigma cut-offs of PBE exchange and correlation, where the order
// of the two derivatives matters (the first direction is the potential's variable, the perturbation sees a constant, as
// in xc::spin_table_point): bits 15..24 of WHICH evaluate them at such points and copy H_ij everywhere else, so that
// k_fxc_coef_pol reads H_ij as "potential i, perturbation j" without asking where the point sits.
//
// A channel below the density cut-off is absent (xc::spin_vars): its g and its rows and columns of H are exactly 0.
#include "xc_functionals.hpp"
#include "xc_spin_functionals.hpp"
#include "xc_response_pol_launch.hpp"

namespace qcdft {

namespace {

template <bool GGA>
__device__ __forceinline__ xc::SpinVars load_vars(long g, const double *__restrict__ rho_a, const double *__restrict__ rho_b,
                                                  const double *__restrict__ g_a, const double *__restrict__ g_b)
{
    if (GGA)
        return xc::spin_vars<true>(rho_a[g], rho_b[g], g_a[3 * g], g_a[3 * g + 1], g_a[3 * g + 2], g_b[3 * g], g_b[3 * g + 1],
                                   g_b[3 * g + 2]);
    return xc::spin_vars<false>(rho_a[g], rho_b[g], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0);
}

} // namespace

template <bool GGA, int WHICH>
__global__ __launch_bounds__(256) void k_fxc_table_pol(long ngrid, const double *__restrict__ rho_a,
                                                       const double *__restrict__ rho_b, const double *__restrict__ g_a,
                                                       const double *__restrict__ g_b, const double *__restrict__ w,
                                                       double *table, double scale, xc::MixWeights m)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const size_t n = (size_t)ngrid;
    const xc::SpinVars x = load_vars<GGA>(g, rho_a, rho_b, g_a, g_b);
    const double sw = scale * w[g];
    constexpr int NV = GGA ? 5 : 2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int j = i; j < NV; ++j) {
            const int p = xc::pol_upper(NV, i, j);
            if (!((WHICH >> p) & 1)) continue;
            double h, gi;
            xc::spin_hessian_entry<GGA>(m, x, i, j, &h, &gi);
            table[(size_t)p * n + g] = sw * h;
            if (GGA && i == j && i >= 2) table[(size_t)(xc::kPolG + i - 2) * n + g] = sw * gi;
        }
    }
    // Bits 15..24: the ten planes H_ji, i < j, of a gradient functional -- a copy of H_ij except at a sigma cut-off,
    // where the pair is evaluated with x_j first.  Such a launch runs behind the one that wrote H_ij (stream order).
    if (GGA && (WHICH >> 15)) {
        const bool cut = xc::spin_sigma_cut(x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = i + 1; j < 5; ++j) {
                const int q = xc::pol_lower(5, i, j);
                if (!((WHICH >> (15 + q)) & 1)) continue;
                double h = table[(size_t)xc::pol_upper(5, i, j) * n + g];
                if (cut) {
                    double gj;
                    xc::spin_hessian_entry<GGA>(m, x, j, i, &h, &gj);
                    h *= sw;
                }
                table[(size_t)(xc::kPolLower + q) * n + g] = h;
            }
        }
    }
}

// Arithmetic only.  g0_* / g1_*: three per point, interleaved (what the density kernels write).
template <bool GGA>
__global__ __launch_bounds__(256) void k_fxc_coef_pol(long ngrid, const double *__restrict__ table,
                                                      const double *__restrict__ g0_a, const double *__restrict__ g0_b,
                                                      const double *__restrict__ rho1_a, const double *__restrict__ rho1_b,
                                                      const double *__restrict__ g1_a, const double *__restrict__ g1_b,
                                                      double *__restrict__ coef_a, double *__restrict__ coef_b)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const size_t n = (size_t)ngrid;
    const double ra1 = rho1_a[g], rb1 = rho1_b[g];
    if (!GGA) {
        const double h01 = table[n + g];
        coef_a[g] = table[g] * ra1 + h01 * rb1;
        coef_b[g] = h01 * ra1 + table[2 * n + g] * rb1;
        return;
    }
    double a0[3], b0[3], a1[3], b1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a0[k] = g0_a[3 * g + k]; b0[k] = g0_b[3 * g + k];
        a1[k] = g1_a[3 * g + k]; b1[k] = g1_b[3 * g + k];
    }
    const double x1[5] = {ra1, rb1, 2.0 * (a0[0] * a1[0] + a0[1] * a1[1] + a0[2] * a1[2]),
                          (a0[0] * b1[0] + a0[1] * b1[1] + a0[2] * b1[2]) + (b0[0] * a1[0] + b0[1] * a1[1] + b0[2] * a1[2]),
                          2.0 * (b0[0] * b1[0] + b0[1] * b1[1] + b0[2] * b1[2])};
    double t[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int p = i <= j ? xc::pol_upper(5, i, j) : xc::kPolLower + xc::pol_lower(5, j, i);
            s += table[(size_t)p * n + g] * x1[j];
        }
        t[i] = s;
    }
    const double g2 = table[(size_t)xc::kPolG * n + g], g3 = table[(size_t)(xc::kPolG + 1) * n + g],
                 g4 = table[(size_t)(xc::kPolG + 2) * n + g];
    coef_a[g] = t[0];
    coef_b[g] = t[1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        coef_a[(size_t)(1 + k) * n + g] = 2.0 * (2.0 * t[2] * a0[k] + 2.0 * g2 * a1[k] + t[3] * b0[k] + g3 * b1[k]);
        coef_b[(size_t)(1 + k) * n + g] = 2.0 * (2.0 * t[4] * b0[k] + 2.0 * g4 * b1[k] + t[3] * a0[k] + g3 * a1[k]);
    }
}

int fxc_pol_planes(bool gga) { return gga ? xc::kPolPlanes : 3; }

namespace {

template <int P>
void launch_upper(hipStream_t st, dim3 g, long ngrid, const double *rho_a, const double *rho_b, const double *g_a, const double *g_b,
                  const double *w, double *table, double scale, const xc::MixWeights &m)
{
    hipLaunchKernelGGL((k_fxc_table_pol<true, 1 << P>), g, dim3(256), 0, st, ngrid, rho_a, rho_b, g_a, g_b, w, table, scale, m);
    if constexpr (P + 1 < 25) launch_upper<P + 1>(st, g, ngrid, rho_a, rho_b, g_a, g_b, w, table, scale, m);
}

} // namespace

hipError_t launch_fxc_table_pol(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho_a,
                                const double *rho_b, const double *g_a, const double *g_b, const double *w, double *table)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    xc::MixWeights m;
    double scale = 1.0;
    if (type == 3) for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    else           scale = xc::builtin_spin_mix(type, m);
    if (!gga) {
        hipLaunchKernelGGL((k_fxc_table_pol<false, 1>), g, b, 0, st, ngrid, rho_a, rho_b, g_a, g_b, w, table, scale, m);
        hipLaunchKernelGGL((k_fxc_table_pol<false, 2>), g, b, 0, st, ngrid, rho_a, rho_b, g_a, g_b, w, table, scale, m);
        hipLaunchKernelGGL((k_fxc_table_pol<false, 4>), g, b, 0, st, ngrid, rho_a, rho_b, g_a, g_b, w, table, scale, m);
        return hipGetLastError();
    }
    launch_upper<0>(st, g, ngrid, rho_a, rho_b, g_a, g_b, w, table, scale, m);   // one pair per launch: 15 of the upper triangle, then the 10 in the other order
    return hipGetLastError();
}

hipError_t launch_fxc_coef_pol(hipStream_t st, bool gga, long ngrid, const double *table, const double *g0_a, const double *g0_b,
                               const double *rho1_a, const double *rho1_b, const double *g1_a, const double *g1_b,
                               double *coef_a, double *coef_b)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    if (gga) hipLaunchKernelGGL(k_fxc_coef_pol<true>, g, b, 0, st, ngrid, table, g0_a, g0_b, rho1_a, rho1_b, g1_a, g1_b, coef_a, coef_b);
    else     hipLaunchKernelGGL(k_fxc_coef_pol<false>, g, b, 0, st, ngrid, table, g0_a, g0_b, rho1_a, rho1_b, g1_a, g1_b, coef_a, coef_b);
    return hipGetLastError();
}

} // namespace qcdft
