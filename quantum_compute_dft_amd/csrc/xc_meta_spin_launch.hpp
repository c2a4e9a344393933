// Host interface of the spin-resolved meta-GGA kernels (xc_meta_spin.hip): the kinetic-energy densities of both spins in
// one launch and the pointwise functional at any polarisation.  The tau term of the potential and the one-spin k_tau are
// those of xc_meta_launch.hpp.
#pragma once
#include "xc_meta_launch.hpp"

namespace qcdft {

// tau_plan's shape with room for the row sums of two spins (red[2][4][16]).
TauPlan tau_spin_plan(int num_cu, long ngrid, int nao);

// tau_s[g] = (1/2) sum_k sum_mu,nu Dp_s[mu, nu] (d_k AO)[g, mu] (d_k AO)[g, nu], s = alpha, beta, from one staging of the
// three gradient planes ao_grad (3, ngrid, nao) and the two zero-padded symmetric matrices Dp_a, Dp_b (NP, NP).  Per spin
// the operations and their order are k_tau's.  Refuses an LDS request above 160 KB.
hipError_t launch_tau_spin(hipStream_t st, const TauPlan &p, long ngrid, int nao, const double *ao_grad, const double *Dp_a,
                           const double *Dp_b, double *tau_a, double *tau_b);

// xc::meta_spin_point at every grid point: coef_a, coef_b (4, ngrid) = c0..c3 of each spin, ct_a, ct_b (ngrid), one Exc
// partial per block of 256 points (meta_points_blocks).  grad_a / grad_b: three per point, interleaved, as the density
// kernels write them.
hipError_t launch_xc_points_meta_spin(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho_a,
                                      const double *rho_b, const double *grad_a, const double *grad_b, const double *tau_a,
                                      const double *tau_b, const double *w, double *coef_a, double *coef_b, double *ct_a,
                                      double *ct_b, double *partial);

} // namespace qcdft
