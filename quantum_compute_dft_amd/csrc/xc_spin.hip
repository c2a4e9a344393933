// Pointwise part of the spin-resolved (open-shell) sweep, DFT_ComputeXCSpin (dft_api.hip).
//
// Per grid point: rho_a, rho_b and their gradients in, the coefficient planes of the alpha and of the beta potential and
// w e out -- xc::spin_potential_point (xc_spin_functionals.hpp), the first derivatives of the spin-resolved energy
// bodies by xc::Dual, evaluated one after the other.  Everything else of the call (the two densities, the two
// contractions with the AO planes, the slab reduces) is the closed-shell sweep's kernels, which are linear in what
// they are handed and do not know about spin.
#include "xc_functionals.hpp"
#include "xc_spin_functionals.hpp"
#include "xc_spin_launch.hpp"

namespace qcdft {

// Each block leaves one deterministic partial of sum_g w_g e_g, in the reduction shape of k_xc_points.  Built-in types
// arrive as their component weights and `scale` (B3LYP: 1/2, its M + M^T convention).
template <bool GGA>
__global__ __launch_bounds__(256) void k_xc_points_spin(long ngrid, const double *__restrict__ rho_a,
                                                        const double *__restrict__ rho_b,
                                                        const double *__restrict__ grad_a,
                                                        const double *__restrict__ grad_b,
                                                        const double *__restrict__ w, double *__restrict__ coef_a,
                                                        double *__restrict__ coef_b, double *__restrict__ partial,
                                                        double scale, xc::MixWeights m)
{
    __shared__ double red[4];
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (g < ngrid) {
        const size_t n = (size_t)ngrid;
        const double wt = w[g];
        xc::SpinPoint p;
        if (GGA)
            p = xc::spin_potential_point<true>(m, rho_a[g], rho_b[g], grad_a[3 * g], grad_a[3 * g + 1], grad_a[3 * g + 2],
                                               grad_b[3 * g], grad_b[3 * g + 1], grad_b[3 * g + 2], wt, scale);
        else
            p = xc::spin_potential_point<false>(m, rho_a[g], rho_b[g], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, wt, scale);
        coef_a[g] = p.a[0];
        coef_b[g] = p.b[0];
        if (GGA) {
            coef_a[n + g] = p.a[1]; coef_a[2 * n + g] = p.a[2]; coef_a[3 * n + g] = p.a[3];
            coef_b[n + g] = p.b[1]; coef_b[2 * n + g] = p.b[2]; coef_b[3 * n + g] = p.b[3];
        }
        e = wt * p.e;
    }
    for (int k = 32; k >= 1; k >>= 1) e += __shfl_down(e, k, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

hipError_t launch_xc_points_spin(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho_a,
                                 const double *rho_b, const double *grad_a, const double *grad_b, const double *w,
                                 double *coef_a, double *coef_b, double *partial)
{
    const dim3 g((unsigned)spin_points_blocks(ngrid)), b(256);
    xc::MixWeights m;
    double scale = 1.0;
    if (type == 3) for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    else           scale = xc::builtin_spin_mix(type, m);
    if (gga) hipLaunchKernelGGL(k_xc_points_spin<true>, g, b, 0, st, ngrid, rho_a, rho_b, grad_a, grad_b, w, coef_a, coef_b, partial, scale, m);
    else     hipLaunchKernelGGL(k_xc_points_spin<false>, g, b, 0, st, ngrid, rho_a, rho_b, grad_a, grad_b, w, coef_a, coef_b, partial, scale, m);
    return hipGetLastError();
}

} // namespace qcdft
