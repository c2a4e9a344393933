// Host interface of the pointwise kernels of the open-shell response of Vxc (xc_response_pol.hip; DFT_FxcPrepareSpinPol /
// DFT_FxcApplySpinPol in dft_api.hip).  Compiled in their own translation unit, like xc_response.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace qcdft {

// Planes of the table (SoA, ngrid each): 28 for a functional that reads the gradient, 3 for an LDA-class one.
int fxc_pol_planes(bool gga);

// The table from the two spin densities and their gradients (3 per point, interleaved; null when !gga) and the weights.
// type: 0 LDA, 1 GGA, 2 B3LYP, 3 mix (`mix8`: its eight weights).  Independent of `quirks`: derivatives of the energy.
hipError_t launch_fxc_table_pol(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho_a,
                                const double *rho_b, const double *g_a, const double *g_b, const double *w, double *table);

// coef_a / coef_b (c0'..c3' SoA, the layout of k_xc_points_spin; c0' alone when !gga) from the table, the ground-state
// gradients and rho1 / grad rho1 of the two perturbations as the density kernels leave them.
hipError_t launch_fxc_coef_pol(hipStream_t st, bool gga, long ngrid, const double *table, const double *g0_a, const double *g0_b,
                               const double *rho1_a, const double *rho1_b, const double *g1_a, const double *g1_b,
                               double *coef_a, double *coef_b);

} // namespace qcdft
