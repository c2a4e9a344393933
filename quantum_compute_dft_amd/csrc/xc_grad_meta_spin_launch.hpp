// Host interface of the XC force of a meta-GGA at two spin densities (xc_grad_meta_spin.hip): the contraction of the spin
// meta point's coefficient planes c0..c3, ct of either spin with the ten AO planes, and the energy per volume of that point.
// Compiled in their own translation unit, beside xc_grad_meta.hip, whose kernels stay as they are.
#pragma once
#include "xc_grad_meta_launch.hpp"

namespace qcdft {

// Widest K chunk (basis functions) of the six tiles a workgroup of k_xc_grad_meta_spin keeps in LDS (AO, Q_a, Q_b, three
// gradient planes): 8 (6 x 16 x 161 + 3 NP + 160) bytes <= 160 KB up to NP = 1616, so nao = 1150 fits (176 would stop at
// NP = 1104).
constexpr int XCGMS_KC_MAX = 160;

// Workgroups of one k_xc_grad_meta_spin launch for this shape (= slabs of (nao, 3) it writes), its K chunk and its LDS.
XcGradPlan xc_grad_meta_spin_plan(int num_cu, long ngrid, int nao);

// out (nao, 3) = sum_s [ G_gga[c_s0..c_s3; Dp_s] - 2 sum_g ct_s sum_k hess_xk Y_sk ],  Y_sk = (d_k AO) Dp_s, both spins in one
// pass over the ten planes (k_xc_grad_meta_spin) and a fixed-order slab sum.  coef_s: c0..c3 SoA (ngrid each), one-sided;
// ct_s (ngrid) = w e_tau_s / 2; Dp_s the zero-padded symmetric matrices (NP, NP).  slabs: room for nwg * 3 * nao doubles.
hipError_t launch_xc_grad_meta_spin_fused(hipStream_t st, const XcGradPlan &p, long ngrid, int nao, const double *ao, const double *ao_grad,
                                          const double *hess, const double *coef_a, const double *coef_b, const double *ct_a,
                                          const double *ct_b, const double *Dp_a, const double *Dp_b, double *slabs, double *out);

// The plain form the fused kernel is held to: per spin k_xc_grad<true, 1> on c_s0..c_s3 (plan pg, fac = 1) into pg.nwg slabs,
// then the tau term alone (k_xc_grad_meta<false>, plan pt) into pt.nwg more -- alpha's two sets, then beta's -- and one
// fixed-order sum over all four.  slabs: room for 2 (pg.nwg + pt.nwg) * 3 * nao doubles.
hipError_t launch_xc_grad_meta_spin_plain(hipStream_t st, const XcGradPlan &pg, const XcGradPlan &pt, long ngrid, int nao, const double *ao,
                                          const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                                          const double *ct_a, const double *ct_b, const double *Dp_a, const double *Dp_b, double *slabs,
                                          double *out);

// e[g] = the energy per volume of xc::meta_spin_point at (rho_s, grad rho_s, tau_s)[g], unit weight (k_xc_edens_meta_spin).
// grad_s: three per point, interleaved, as the density kernels write them.
hipError_t launch_xc_edens_meta_spin(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho_a,
                                     const double *rho_b, const double *grad_a, const double *grad_b, const double *tau_a,
                                     const double *tau_b, double *e);

} // namespace qcdft
