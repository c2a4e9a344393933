// Grid response of the analytic nuclear gradient (DFT_BeckeWeightGradient / DFT_ComputeXCEnergyDensity[Spin], dft_api.hip).
//
// Exc = sum_g w0_g cell_g e_g with cell_g = P_own(r_g) / sum_C P_C(r_g) the Becke cell function of the point's own atom
// (grid_gen.becke_weights: P_C = prod_{D != C} s_CD, s = (1 - p(p(p(nu)))) / 2, nu = mu + a_CD (1 - mu^2),
// mu_CD = (d_C - d_D) / R_CD, p(x) = (3 x - x^3) / 2).  k_becke_wgrad contracts f_g = w0_g e_g with the derivatives of
// cell_g by the atom positions at fixed r:
//
//     dP_C/dR_B = q_CB (u_B + mu_CB n_CB)  (B != C),   dP_C/dR_C = -sum_D q_CD (u_C + mu_CD n_CD),
//     q_CB = (P_C / s_CB) t_CB / R_CB,   t = ds/dmu = -1/2 p'(p(p(nu))) p'(p(nu)) p'(nu) (1 - 2 a mu),
//
// u_B = (r - R_B) / d_B, n_CB = (R_C - R_B) / R_CB.  With c_C = (delta_{C,own} - cell) / Z, E_C = c_C P_C and the
// antisymmetric W_CB = (E_C t / s_CB - E_B t / s_BC) / R_CB  (s_BC = 1 - s_CB and t_BC = t_CB: nu_BC = -nu_CB)
//
//     dcell/dR_B = u_B sum_C W_CB + sum_C W_CB mu_CB n_CB.
//
// The owner's own entry is minus the sum of the others (the cell function is translationally invariant and the point
// moves with its owner).  t / s is taken as 0 where s == 0 (there t vanishes with it): no division by a cell function
// or a switching factor that can be zero; a point on a nucleus has u = 0.
//
// A workgroup owns tiles of `tp` points.  Phase one leaves d_C and P_C of the tile's points in LDS ((tp, natm) each);
// phase two gives every (point, B) pair to one thread, which walks C; the tp lanes of one B are neighbours in a wave and
// are summed by shuffles, one lane adds into the workgroup's (natm, 3) in LDS; the owners' shares go through LDS in a
// fixed order.  One slab per workgroup, k_becke_wgrad_sum adds the slabs in slab order: the same call twice gives the
// same bits.  No floating-point atomics.  fp64 VALU: the work is 60-odd flops and one division per (point, C, B).
//
// k_xc_edens / k_xc_edens_mix / k_xc_edens_spin: e_g of the bodies k_xc_points / k_xc_points_mix / k_xc_points_spin run
// (unit weight), for f_g.
#include "becke_launch.hpp"
#include "xc_functionals.hpp"
#include "xc_spin_functionals.hpp"
#include <algorithm>

namespace qcdft {

namespace {

constexpr int BK_FIXED = 3 * 256 + 3 * BECKE_TP_MAX + 6 * BECKE_TP_MAX;   // doubles of LDS beside the tile arrays and the accumulator

__device__ __forceinline__ double becke_p(double x) { return (3.0 - x * x) * x * 0.5; }

} // namespace

// Dynamic LDS: dl[tp * natm], pl[tp * natm], acc[3 * natm], fold[3 * 256], F[3 * 64], px, py, pz, fl, zinv, cl [64 each],
// ownl[64] (int).  tp: a power of two, 8..64; thread tid works for point tid % tp and the atoms tid / tp + k (256 / tp).
__global__ __launch_bounds__(256) void k_becke_wgrad(long ngrid, int natm, int tp, const double *__restrict__ atoms,
                                                     const double *__restrict__ atab, const double *__restrict__ rtab,
                                                     const double *__restrict__ coords, const int *__restrict__ owner,
                                                     const double *__restrict__ f, double *__restrict__ cell_out,
                                                     double *__restrict__ slabs)
{
    extern __shared__ double lds[];
    double *dl = lds;
    double *pl = dl + (size_t)tp * natm;
    double *acc = pl + (size_t)tp * natm;
    double *fold = acc + 3 * natm;
    double *F = fold + 3 * 256;
    double *px = F + 3 * BECKE_TP_MAX, *py = px + BECKE_TP_MAX, *pz = py + BECKE_TP_MAX, *fl = pz + BECKE_TP_MAX,
           *zinv = fl + BECKE_TP_MAX, *cl = zinv + BECKE_TP_MAX;
    int *ownl = (int *)(cl + BECKE_TP_MAX);
    const int tid = threadIdx.x, gl = tid & (tp - 1), slot = tid / tp, nslot = 256 / tp;
    const long ntile = (ngrid + tp - 1) / tp;

    for (int i = tid; i < 3 * natm; i += 256) acc[i] = 0.0;

    for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const long g0 = tl * tp;
        __syncthreads();   // the previous tile's readers of the point data are done
        if (tid < tp) {
            const long g = g0 + tid, gc = min(g, ngrid - 1);   // points past the grid repeat the last one with f = 0
            px[tid] = coords[3 * gc];
            py[tid] = coords[3 * gc + 1];
            pz[tid] = coords[3 * gc + 2];
            fl[tid] = g < ngrid ? f[gc] : 0.0;
            ownl[tid] = min(max(owner[gc], 0), natm - 1);
        }
        __syncthreads();
        const double x = px[gl], y = py[gl], z = pz[gl];
        const int own = ownl[gl];
        for (int C = slot; C < natm; C += nslot) {
            const double dx = x - atoms[3 * C], dy = y - atoms[3 * C + 1], dz = z - atoms[3 * C + 2];
            dl[C * tp + gl] = sqrt(dx * dx + dy * dy + dz * dz);
        }
        __syncthreads();
        for (int C = slot; C < natm; C += nslot) {
            const double dC = dl[C * tp + gl];
            const double *ar = atab + (size_t)C * natm, *rr = rtab + (size_t)C * natm;
            double P = 1.0;
            for (int D = 0; D < natm; ++D) {
                if (D == C) continue;
                const double mu = (dC - dl[D * tp + gl]) * rr[D];
                const double nu = mu + ar[D] * (1.0 - mu * mu);
                P *= 0.5 * (1.0 - becke_p(becke_p(becke_p(nu))));
            }
            pl[C * tp + gl] = P;
        }
        __syncthreads();
        if (tid < tp) {
            double Z = 0.0;
            for (int C = 0; C < natm; ++C) Z += pl[C * tp + tid];
            const double c = pl[ownl[tid] * tp + tid] / Z;
            zinv[tid] = 1.0 / Z;
            cl[tid] = c;
            if (cell_out && g0 + tid < ngrid) cell_out[g0 + tid] = c;
        }
        __syncthreads();
        const double fg = fl[gl], zi = zinv[gl], cg = cl[gl];
        double ox = 0.0, oy = 0.0, oz = 0.0;   // the owner's share of this thread's atoms
        for (int B0 = 0; B0 < natm; B0 += nslot) {   // the same trip count for every thread: the shuffles below are whole
            const int B = B0 + slot;
            double vx = 0.0, vy = 0.0, vz = 0.0;
            if (B < natm && B != own && fg != 0.0) {
                const double dB = dl[B * tp + gl], EB = -cg * zi * pl[B * tp + gl];
                const double bx = atoms[3 * B], by = atoms[3 * B + 1], bz = atoms[3 * B + 2];
                double A = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
                for (int C = 0; C < natm; ++C) {
                    if (C == B) continue;
                    const double invR = rtab[(size_t)C * natm + B], a = atab[(size_t)C * natm + B];
                    const double EC = ((C == own ? 1.0 : 0.0) - cg) * zi * pl[C * tp + gl];
                    const double mu = (dl[C * tp + gl] - dB) * invR;
                    const double nu = mu + a * (1.0 - mu * mu);
                    const double p1 = becke_p(nu), p2 = becke_p(p1), p3 = becke_p(p2);
                    const double s = 0.5 * (1.0 - p3), sb = 0.5 * (1.0 + p3);
                    const double t = -1.6875 * (1.0 - p2 * p2) * (1.0 - p1 * p1) * (1.0 - nu * nu) * (1.0 - 2.0 * a * mu);
                    const double ss = s * sb;
                    const double q = ss != 0.0 ? t / ss : 0.0;
                    // t / s_CB and t / s_BC; where one factor is exactly 0 the other is exactly 1
                    const double r1 = sb == 0.0 ? t : q * sb, r2 = s == 0.0 ? t : q * s;
                    const double W = (EC * r1 - EB * r2) * invR;
                    const double m = W * mu * invR;
                    A += W;
                    nx += m * (atoms[3 * C] - bx);
                    ny += m * (atoms[3 * C + 1] - by);
                    nz += m * (atoms[3 * C + 2] - bz);
                }
                const double ud = dB > 0.0 ? A / dB : 0.0;
                vx = fg * (ud * (x - bx) + nx);
                vy = fg * (ud * (y - by) + ny);
                vz = fg * (ud * (z - bz) + nz);
                ox -= vx;
                oy -= vy;
                oz -= vz;
            }
            for (int m = tp >> 1; m >= 1; m >>= 1) {   // the tp lanes of one atom are neighbours in a wave
                vx += __shfl_xor(vx, m, 64);
                vy += __shfl_xor(vy, m, 64);
                vz += __shfl_xor(vz, m, 64);
            }
            if (gl == 0 && B < natm) {   // atom B belongs to this thread in every tile: no other writer
                acc[3 * B] += vx;
                acc[3 * B + 1] += vy;
                acc[3 * B + 2] += vz;
            }
        }
        fold[3 * tid] = ox;
        fold[3 * tid + 1] = oy;
        fold[3 * tid + 2] = oz;
        __syncthreads();
        if (tid < 3 * tp) {   // the share of point tid / 3, summed over the slots in slot order
            const int p = tid / 3, k = tid - 3 * p;
            double s = 0.0;
            for (int sl = 0; sl < nslot; ++sl) s += fold[3 * (sl * tp + p) + k];
            F[tid] = s;
        }
        __syncthreads();
        for (int i = tid; i < 3 * natm; i += 256) {   // ... and to the points' owners, in point order
            const int A = i / 3, k = i - 3 * A;
            double s = 0.0;
            for (int p = 0; p < tp; ++p)
                if (ownl[p] == A) s += F[3 * p + k];
            acc[i] += s;
        }
    }
    __syncthreads();
    double *slab = slabs + (size_t)blockIdx.x * 3 * natm;
    for (int i = tid; i < 3 * natm; i += 256) slab[i] = acc[i];
}

// out[i] = sum of the slabs in slab order, i < n
__global__ __launch_bounds__(256) void k_becke_wgrad_sum(int n, int nslab, const double *__restrict__ slabs,
                                                         double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += slabs[(size_t)k * n + i];
    out[i] = s;
}

// TYPE 0 LDA, 1 GGA(PBE), 2 B3LYP: the point bodies of k_xc_points with unit weight; only the energy is kept.
template <int TYPE>
__global__ __launch_bounds__(256) void k_xc_edens(long ngrid, const double *__restrict__ rho, const double *__restrict__ sigma,
                                                  const double *__restrict__ grad, double *__restrict__ e_out, int quirks)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    const double r = rho[g];
    xc::PointXC p;
    if (TYPE == 0) {
        p = xc::lda_point(r, 1.0, quirks != 0);
    } else {
        const double ax = grad[3 * g], ay = grad[3 * g + 1], az = grad[3 * g + 2];
        if (TYPE == 1) p = xc::gga_point(r, sigma[g], ax, ay, az, 1.0, quirks != 0);
        else           p = xc::b3lyp_point(r, sigma[g], ax, ay, az, 1.0);
    }
    e_out[g] = p.exc;
}

// SOLVER_MIX: the same around xc::mix_point, as k_xc_points_mix
template <bool GGA>
__global__ __launch_bounds__(256) void k_xc_edens_mix(long ngrid, const double *__restrict__ rho, const double *__restrict__ sigma,
                                                      const double *__restrict__ grad, double *__restrict__ e_out, int quirks,
                                                      xc::MixWeights m)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    xc::PointXC p;
    if (GGA) p = xc::mix_point<true>(m, rho[g], sigma[g], grad[3 * g], grad[3 * g + 1], grad[3 * g + 2], 1.0, quirks != 0);
    else     p = xc::mix_point<false>(m, rho[g], 0.0, 0.0, 0.0, 0.0, 1.0, quirks != 0);
    e_out[g] = p.exc;
}

// The spin-resolved body of k_xc_points_spin with unit weight; only the energy is kept.
template <bool GGA>
__global__ __launch_bounds__(256) void k_xc_edens_spin(long ngrid, const double *__restrict__ rho_a, const double *__restrict__ rho_b,
                                                       const double *__restrict__ grad_a, const double *__restrict__ grad_b,
                                                       double *__restrict__ e_out, double scale, xc::MixWeights m)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    xc::SpinPoint p;
    if (GGA)
        p = xc::spin_potential_point<true>(m, rho_a[g], rho_b[g], grad_a[3 * g], grad_a[3 * g + 1], grad_a[3 * g + 2],
                                           grad_b[3 * g], grad_b[3 * g + 1], grad_b[3 * g + 2], 1.0, scale);
    else
        p = xc::spin_potential_point<false>(m, rho_a[g], rho_b[g], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, scale);
    e_out[g] = p.e;
}

BeckePlan becke_plan(int num_cu, long ngrid, int natm)
{
    BeckePlan p;
    p.tp = BECKE_TP_MAX;
    while (p.tp > BECKE_TP_MIN && sizeof(double) * 2 * (size_t)p.tp * natm > BECKE_TILE_BYTES) p.tp /= 2;
    p.lds = sizeof(double) * (2 * (size_t)p.tp * natm + 3 * (size_t)natm + BK_FIXED) + sizeof(int) * BECKE_TP_MAX;
    const long ntile = (ngrid + p.tp - 1) / p.tp;
    const long per_cu = std::max<long>(1, std::min<long>(4, (long)(BECKE_LDS_MAX / (p.lds + 512))));
    p.nwg = (int)std::max<long>(1, std::min<long>(ntile, per_cu * num_cu));
    return p;
}

hipError_t launch_becke_wgrad(hipStream_t st, const BeckePlan &p, long ngrid, int natm, const double *atoms, const double *a_tab,
                              const double *invr_tab, const double *coords, const int *owner, const double *f, double *cell,
                              double *slabs, double *out)
{
    if (p.lds > BECKE_LDS_MAX || p.tp < BECKE_TP_MIN || p.tp > BECKE_TP_MAX || (p.tp & (p.tp - 1))) return hipErrorInvalidValue;
    static size_t allowed = 48 * 1024;   // dynamic LDS above the default needs the attribute once
    if (p.lds > allowed) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_becke_wgrad, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        allowed = p.lds;
    }
    hipLaunchKernelGGL(k_becke_wgrad, dim3((unsigned)p.nwg), dim3(256), p.lds, st, ngrid, natm, p.tp, atoms, a_tab, invr_tab, coords,
                       owner, f, cell, slabs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n = 3 * natm;
    hipLaunchKernelGGL(k_becke_wgrad_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, p.nwg, slabs, out);
    return hipGetLastError();
}

hipError_t launch_xc_edens(hipStream_t st, int type, bool gga, const double *mix8, int quirks, long ngrid, const double *rho,
                           const double *sigma, const double *grad, double *e)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    switch (type) {
    case 0: hipLaunchKernelGGL(k_xc_edens<0>, g, b, 0, st, ngrid, rho, sigma, grad, e, quirks); break;
    case 1: hipLaunchKernelGGL(k_xc_edens<1>, g, b, 0, st, ngrid, rho, sigma, grad, e, quirks); break;
    case 2: hipLaunchKernelGGL(k_xc_edens<2>, g, b, 0, st, ngrid, rho, sigma, grad, e, quirks); break;
    default: {
        xc::MixWeights m;
        for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
        if (gga) hipLaunchKernelGGL(k_xc_edens_mix<true>, g, b, 0, st, ngrid, rho, sigma, grad, e, quirks, m);
        else     hipLaunchKernelGGL(k_xc_edens_mix<false>, g, b, 0, st, ngrid, rho, sigma, grad, e, quirks, m);
    }
    }
    return hipGetLastError();
}

hipError_t launch_xc_edens_spin(hipStream_t st, int type, bool gga, const double *mix8, long ngrid, const double *rho_a,
                                const double *rho_b, const double *grad_a, const double *grad_b, double *e)
{
    const dim3 g((unsigned)((ngrid + 255) / 256)), b(256);
    xc::MixWeights m;
    double scale = 1.0;
    if (type == 3) for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    else           scale = xc::builtin_spin_mix(type, m);
    if (gga) hipLaunchKernelGGL(k_xc_edens_spin<true>, g, b, 0, st, ngrid, rho_a, rho_b, grad_a, grad_b, e, scale, m);
    else     hipLaunchKernelGGL(k_xc_edens_spin<false>, g, b, 0, st, ngrid, rho_a, rho_b, grad_a, grad_b, e, scale, m);
    return hipGetLastError();
}

} // namespace qcdft
