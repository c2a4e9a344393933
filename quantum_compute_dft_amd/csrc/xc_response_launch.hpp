// Host interface of the pointwise linear-response kernels (xc_response.hip): the derivative table of the
// functional at the ground-state density and the coefficients of the response of Vxc to a perturbed density.
// Compiled in their own translation unit, like xc_occ.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace qcdft {

constexpr int FXC_PLANES = 5;   // w P_rho, w P_sigma, w Q_rho, w Q_sigma, w Q (SoA, ngrid each); an LDA-class table has the first only

// table[k * ngrid + g] from rho, sigma and the weights.  type: 0 LDA, 1 GGA, 2 B3LYP, 3 mix (`mix8`: its eight
// weights, `gga`: it reads sigma).  sigma may be null for an LDA-class functional.
hipError_t launch_fxc_table(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho,
                            const double *sigma, const double *w, double *table, int quirks);

// The same five planes from the spin-resolved energy bodies (xc_spin_functionals.hpp): kind 1 the spin-flip (triplet)
// response, kind 2 the singlet response through those bodies.  Independent of `quirks`: a derivative of the energy.
hipError_t launch_fxc_table_spin(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho,
                                 const double *sigma, const double *w, double *table, int kind);

// coef (c0'..c3' SoA, the layout of k_xc_points; c0' alone when !gga) from the table, the ground-state gradient g0
// (3 per point, interleaved), and rho1 / g1 of the perturbation as the density kernels leave them.
hipError_t launch_fxc_coef(hipStream_t st, bool gga, long ngrid, const double *table, const double *g0,
                           const double *rho1, const double *g1, double *coef);

} // namespace qcdft
