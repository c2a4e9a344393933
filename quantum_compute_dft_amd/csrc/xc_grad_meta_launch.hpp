// Host interface of the XC force of a functional that reads tau (xc_grad_meta.hip): the contraction of the meta point's
// coefficient planes c0..c3, ct with the ten AO planes, and the energy per volume of the meta point.  Compiled in their
// own translation unit, beside xc_grad.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "xc_grad_launch.hpp"

namespace qcdft {

// Widest K chunk (basis functions) of the tiles a workgroup of k_xc_grad_meta keeps in LDS.  Five tiles (AO, Q, three
// gradient planes): 8 (5 x 16 x 209 + 3 NP + 80) bytes <= 160 KB up to NP = 1216, so nao = 1150 fits (224 would stop at
// NP = 800).  Three tiles (the gradient planes alone): XCGS_KC_MAX's 320, good up to NP = 1680.
constexpr int XCGM_KC_MAX = 208;
constexpr int XCGT_KC_MAX = 320;

// Workgroups of one k_xc_grad_meta<full> launch for this shape (= slabs of (nao, 3) it writes), its K chunk and its LDS.
XcGradPlan xc_grad_meta_plan(int num_cu, bool full, long ngrid, int nao);

// full: out (nao, 3) = G_gga[c0..c3] - 2 sum_g ct sum_k hess_xk Y_k,  Y_k = (d_k AO) Dp, everything in one pass over the ten
// planes (k_xc_grad_meta<true>) and a fixed-order slab sum.  coef: c0..c3 SoA (ngrid each) in the one-sided convention,
// ct (ngrid) = w e_tau / 2, Dp the zero-padded symmetric matrix (NP, NP).  slabs: room for nwg * 3 * nao doubles.
hipError_t launch_xc_grad_meta_fused(hipStream_t st, const XcGradPlan &p, long ngrid, int nao, const double *ao, const double *ao_grad,
                                     const double *hess, const double *coef, const double *ct, const double *Dp, double *slabs, double *out);

// The plain form the fused kernel is held to: k_xc_grad<true, 1> on c0..c3 (plan pg, fac = 1) into pg.nwg slabs, the tau
// term alone (k_xc_grad_meta<false>, plan pt) into pt.nwg more, one fixed-order sum over both sets.  slabs: room for
// (pg.nwg + pt.nwg) * 3 * nao doubles.
hipError_t launch_xc_grad_meta_plain(hipStream_t st, const XcGradPlan &pg, const XcGradPlan &pt, long ngrid, int nao, const double *ao,
                                     const double *ao_grad, const double *hess, const double *coef, const double *ct, const double *Dp,
                                     double *slabs, double *out);

// The tau term alone without the sum, for a caller that sums slab sets of several kernels (xc_grad_meta_spin.hip):
// k_xc_grad_meta<false> (plan pt) into pt.nwg slabs of (nao, 3).
hipError_t launch_xc_grad_tau_slabs(hipStream_t st, const XcGradPlan &pt, long ngrid, int nao, const double *ao_grad, const double *hess,
                                    const double *ct, const double *Dp, double *slabs);

// e[g] = the energy per volume of xc::meta_point's body at (rho, grad rho, tau)[g], unit weight (k_xc_edens_meta).
// grad: three per point, interleaved, as the density kernels write it.
hipError_t launch_xc_edens_meta(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho, const double *grad,
                                const double *tau, double *e);

} // namespace qcdft
