// Host interface of the pointwise kernel of the spin-resolved sweep (xc_spin.hip, DFT_ComputeXCSpin): from the two spin
// densities and their gradients to the coefficient planes of the alpha and the beta potential and the partials of Exc.
// Compiled in its own translation unit, like xc_response.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace qcdft {

// Partials of Exc the launch leaves: one per 256 grid points, as k_xc_points.
inline long spin_points_blocks(long ngrid) { return (ngrid + 255) / 256; }

// coef_a / coef_b: c0..c3 SoA, ngrid each (the layout of k_xc_points; c0 alone when !gga), in the convention of the
// solver type (xc::spin_potential_point).  grad_a / grad_b: three per point, interleaved, as the density kernels write
// them; null when !gga.  type: 0 LDA, 1 GGA, 2 B3LYP, 3 mix (`mix8`: its eight weights).  partial: spin_points_blocks(ngrid).
hipError_t launch_xc_points_spin(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho_a,
                                 const double *rho_b, const double *grad_a, const double *grad_b, const double *w,
                                 double *coef_a, double *coef_b, double *partial);

} // namespace qcdft
