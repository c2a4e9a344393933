// Host interface of the grid response of the nuclear gradient (becke.hip): the fixed-r derivatives of the Becke cell
// function contracted with a per-point weight, and the energy per volume of the functional at the points of a density.
// Compiled in their own translation unit, like xc_grad.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace qcdft {

constexpr int BECKE_TP_MAX = 64;                 // grid points per tile of k_becke_wgrad at few atoms ...
constexpr int BECKE_TP_MIN = 8;                  // ... and at many: the tile halves while its two (points, natm) arrays exceed
constexpr size_t BECKE_TILE_BYTES = 60 * 1024;   // this many bytes of LDS (64 points to 60 atoms, 32 to 120, 16 to 240, 8 beyond)
constexpr size_t BECKE_LDS_MAX = 160 * 1024;     // what a workgroup may ask for: the entry refuses beyond (natm > 1005)

// Points per tile, workgroups (= slabs of (natm, 3) the kernel writes) and dynamic LDS bytes for this shape.
struct BeckePlan {
    int tp = 0, nwg = 0;
    size_t lds = 0;
};
BeckePlan becke_plan(int num_cu, long ngrid, int natm);

// out (natm, 3) = sum_g f_g D_B cell_g: D_B cell_g the derivative of the cell function of point g's owner by R_B at fixed
// r for B != owner, minus the sum of those for B = owner.  atoms (natm, 3); a_tab, invr_tab (natm, natm): the radius
// adjustment a_CD and 1 / R_CD (any finite value on the diagonal: it is not read); owner values are clamped to
// [0, natm).  cell (ngrid) may be null.  slabs: room for nwg * 3 * natm doubles; a fixed-order slab sum finishes.
hipError_t launch_becke_wgrad(hipStream_t st, const BeckePlan &p, long ngrid, int natm, const double *atoms, const double *a_tab,
                              const double *invr_tab, const double *coords, const int *owner, const double *f, double *cell,
                              double *slabs, double *out);

// e (ngrid): the energy per volume the pointwise kernel of the sweep (k_xc_points / k_xc_points_mix) evaluates at this
// density, without the weight.  type 0 LDA, 1 GGA, 2 B3LYP, 3 mix (mix8: its eight weights).  sigma / grad: read by a
// gradient-corrected functional only.
hipError_t launch_xc_edens(hipStream_t st, int type, bool gga, const double *mix8, int quirks, long ngrid, const double *rho,
                           const double *sigma, const double *grad, double *e);

// The same of the spin-resolved pointwise kernel (k_xc_points_spin); grad_a / grad_b: three per point, interleaved.
hipError_t launch_xc_edens_spin(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho_a,
                                const double *rho_b, const double *grad_a, const double *grad_b, double *e);

} // namespace qcdft
