// Host interface of the XC part of the nuclear gradient (xc_grad.hip): the second-derivative AO planes and the
// contraction of the sweep's coefficient planes with them.  Compiled in their own translation unit, like xc_occ.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "ao_kernels.hpp"

namespace qcdft {

constexpr int XCG_ROWS = 16;      // grid rows per tile of k_xc_grad (one MFMA block of rows)
constexpr int XCG_KC_MAX = 512;   // widest K chunk (basis functions) of the AO / Q tiles a workgroup keeps in LDS, one spin
constexpr int XCGS_KC_MAX = 320;  // the same with two spins in one kernel: three tiles (AO, Q of either spin)
constexpr int AOH_PT = 8;         // grid points per workgroup of k_eval_ao_hess (six planes x 8 x 127 doubles = 48 KB of LDS)

// hess (6, ngrid, nao): xx, xy, xz, yy, yz, zz of every AO at every point; the shell table as launch_eval_ao takes it
// (blocks of at most AO_CW columns, `maxcol` the widest).
hipError_t launch_eval_ao_hess(hipStream_t st, long ngrid, int nao, int nchunk, int maxcol, const AoShell *sh,
                               const double *pexp, const double *pcoef, const AoChunk *chunks, const double *coords,
                               double *hess);

// Workgroups of one k_xc_grad launch for this shape (= slabs of (nao, 3) it writes), its K chunk and its LDS.  nspin: the
// (coef, D) pairs the kernel takes at once -- 1 for launch_xc_grad and launch_xc_grad_spin, 2 for launch_xc_grad_spin_fused.
struct XcGradPlan {
    int NP = 0, kc = 0, ldk = 0, nwg = 0;
    size_t lds = 0;
};
XcGradPlan xc_grad_plan(int num_cu, bool gga, int nspin, long ngrid, int nao);

// out (nao, 3) = -fac * sum_g [ grad_x (Q D) + (sum_k c_k hess_xk) (AO D) ],  Q = 2 c0 AO + sum_k c_k grad_k, from the
// coefficient planes coef (c0..c3 SoA, ngrid each; c0 alone when !gga), the zero-padded symmetric Dp (NP, NP) and the
// planes; slabs: room for nwg * 3 * nao doubles.  hess may be null when !gga.  A fixed-order slab sum finishes.
// Every launcher refuses an LDS request above 160 KB.
hipError_t launch_xc_grad(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                          const double *ao_grad, const double *hess, const double *coef, const double *Dp, double *slabs,
                          double *out);

// The same once per spin, summed: out = G(coef_a, Dp_a) + G(coef_b, Dp_b).  slabs: room for 2 * nwg * 3 * nao doubles (alpha's
// slabs, then beta's); one fixed-order sum over both sets finishes.  The plan of one spin.
hipError_t launch_xc_grad_spin(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                               const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                               const double *Dp_a, const double *Dp_b, double *slabs, double *out);

// The two launches in one (k_xc_grad with both pairs): the plan of two spins, slabs: room for nwg * 3 * nao doubles.
hipError_t launch_xc_grad_spin_fused(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                                     const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                                     const double *Dp_a, const double *Dp_b, double *slabs, double *out);

// The two halves of launch_xc_grad on their own, for a caller that sums slab sets of several kernels (xc_grad_meta.hip):
// k_xc_grad<true, 1> into p.nwg slabs of (nao, 3) without the sum, and the fixed-order sum of `nslab` slabs into out.
hipError_t launch_xc_grad_gga_slabs(hipStream_t st, const XcGradPlan &p, double fac, long ngrid, int nao, const double *ao,
                                    const double *ao_grad, const double *hess, const double *coef, const double *Dp, double *slabs);
hipError_t launch_xc_grad_sum(hipStream_t st, int nao, int nslab, const double *slabs, double *out);

} // namespace qcdft
