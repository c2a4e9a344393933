// Host interface of the meta-GGA kernels (xc_meta.hip): the kinetic-energy density, the pointwise functional with its
// tau coefficient, and the tau term of the potential.  Compiled in their own translation unit, like xc_grad.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace qcdft {

constexpr int META_ROWS = 16;      // grid rows per tile of k_tau (one MFMA block of rows)
constexpr int META_KC_MAX = 384;   // widest K chunk of the three gradient-plane tiles k_tau keeps in LDS (3 x 16 x 385 doubles = 144 KB)
constexpr int META_VG = 32;        // grid rows per staging step of k_vxc_tau

// Workgroups of one k_tau launch for this shape, its K chunk and its LDS.
struct TauPlan {
    int NP = 0, kc = 0, ldk = 0, nwg = 0;
    size_t lds = 0;
};
TauPlan tau_plan(int num_cu, long ngrid, int nao);

// tau[g] = (1/2) sum_k sum_mu,nu Dp[mu, nu] (d_k AO)[g, mu] (d_k AO)[g, nu] from the three gradient planes ao_grad
// (3, ngrid, nao) and the zero-padded symmetric Dp (NP, NP).  Refuses an LDS request above 160 KB.
hipError_t launch_tau(hipStream_t st, const TauPlan &p, long ngrid, int nao, const double *ao_grad, const double *Dp, double *tau);

inline long meta_points_blocks(long ngrid) { return (ngrid + 255) / 256; }

// xc::meta_point at every grid point: coef (4, ngrid) = c0..c3, ct (ngrid), one Exc partial per block of 256 points.
// grad: three per point, interleaved, as the density kernels write it.
hipError_t launch_xc_points_meta(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho,
                                 const double *grad, const double *tau, const double *w, double *coef, double *ct, double *partial);

// How k_vxc_tau cuts the grid: nslab chunks of `chunk` rows (a multiple of META_VG), one (nao, nao) slab each.
struct VxcTauPlan {
    int nslab = 0, nblk = 0;
    long chunk = 0;
};
VxcTauPlan vxc_tau_plan(int num_cu, long ngrid, int nao);

// vxc (nao, nao) += sum_k (d_k AO)^T diag(ct) (d_k AO): per-chunk slabs, then a fixed-order sum added to vxc.
// slabs: room for nslab * nao * nao doubles.
hipError_t launch_vxc_tau(hipStream_t st, const VxcTauPlan &p, long ngrid, int nao, const double *ao_grad, const double *ct,
                          double *slabs, double *vxc);

// vxc[i] += t[i], i < n (the plain form of the tau term adds its three contractions with this)
hipError_t launch_meta_add(hipStream_t st, long n, const double *t, double *vxc);

} // namespace qcdft
