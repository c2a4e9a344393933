// XC part of the analytic nuclear gradient of a meta-GGA at two spin densities (DFT_ComputeXCGradientMetaSpin /
// DFT_ComputeXCEnergyDensityMetaSpin, dft_api.hip).
//
// The closed-shell meta terms (xc_grad_meta.hip) once per spin, with the spin point's coefficients (k_xc_points_meta_spin:
// one-sided, ct_s = w e_tau_s / 2) and D_s the symmetric part of dm_s:
//
//     G[mu, x] = - sum_s sum_g [ d_x phi (Q_s D_s) + (sum_k c_sk d_xk phi)(AO D_s) + 2 ct_s sum_k d_xk phi Y_sk ][g, mu]
//     Q_s = 2 c_s0 AO + sum_k c_sk d_k AO,   Y_sk = (d_k AO) D_s.
//
// k_xc_grad_meta_spin: k_xc_grad_meta<true>'s shape with both spins in one pass over the ten planes.  A workgroup (4 waves)
// owns tiles of 16 grid rows; wave w takes the column tiles w, w + 4, ... on v_mfma_f64_16x16x4 with the B operands (D_a,
// D_b, zero-padded to NP = 16 ceil(nao / 16)) straight from L2; one (nao, 3) slab per workgroup, summed in slab order by
// launch_xc_grad_sum: no atomics, a call is bitwise reproducible.  Six staged tiles -- AO, Q_a, Q_b and the three gradient
// planes, the AO and gradient tiles staged once for both spins -- and ten accumulators X_s, Z_s, Y_sx, Y_sy, Y_sz: the two
// B loads of a step (the same offset into D_a and D_b) feed five MFMAs each.  The epilogue reads each gradient and Hessian
// element once; per spin its operations are k_xc_grad_meta<true>'s.  Rows past the grid and columns past nao are staged as
// zeros and masked in the epilogue: no out-of-range read.
//
// k_xc_edens_meta_spin: the energy per volume of xc::meta_spin_point at unit weight, one point per thread; a channel below
// the cut-off is absent exactly as in the sweep.
#include "xc_meta_functionals.hpp"
#include "xc_grad_meta_spin_launch.hpp"
#include "device_util.hpp"
#include <algorithm>

namespace qcdft {

// Dynamic LDS: T[6][16 * ldk] (AO, Q_a, Q_b, d_x, d_y, d_z), Gs[3 * NP], cs[160]: c0..c3 of the 16 rows for alpha, the same for
// beta, then ct_a, ct_b.  kc: K chunk, a multiple of 16; ldk = kc | 1.
__global__ __launch_bounds__(256) void k_xc_grad_meta_spin(long ngrid, int nao, int NP, int kc, int ldk, const double *__restrict__ ao,
                                                           const double *__restrict__ gx, const double *__restrict__ gy,
                                                           const double *__restrict__ gz, const double *__restrict__ hess,
                                                           const double *__restrict__ coef_a, const double *__restrict__ coef_b,
                                                           const double *__restrict__ ct_a, const double *__restrict__ ct_b,
                                                           const double *__restrict__ Dp_a, const double *__restrict__ Dp_b,
                                                           double *__restrict__ slabs)
{
    extern __shared__ double lds[];
    const int qsz = XCG_ROWS * ldk;     // one staged tile
    double *T = lds;
    double *Gs = T + 6 * qsz;
    double *cs = Gs + 3 * NP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const size_t ng = (size_t)ngrid, plane = ng * nao;
    const int nct = NP / 16, nround = (nct + 3) / 4, nchunk = (NP + kc - 1) / kc;
    const long ntile = (ngrid + XCG_ROWS - 1) / XCG_ROWS;

    for (int i = tid; i < 3 * NP; i += 256) Gs[i] = 0.0;

    for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const long g0 = tl * XCG_ROWS;
        __syncthreads();   // the previous tile's readers of cs and of the staged rows are done
        if (tid < 160) {
            const int k = tid >> 4, r = tid & 15;
            const long g = g0 + r;
            const double *src = k < 4 ? coef_a + k * ng : k < 8 ? coef_b + (k - 4) * ng : k == 8 ? ct_a : ct_b;
            cs[tid] = g < ngrid ? src[g] : 0.0;
        }
        __syncthreads();
        for (int rd = 0; rd < nround; ++rd) {
            const int j = rd * 4 + wave;
            const bool active = j < nct;   // wave-uniform
            d4 acc[2][5];                  // X, Z, Y_x, Y_y, Y_z of either spin
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < 5; ++t) acc[s][t] = (d4){0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < nchunk; ++c) {
                const int k0 = c * kc, kw = min(kc, NP - k0);
                if (nchunk > 1 || rd == 0) {   // block-uniform: one staging per tile while the whole row fits
                    if (nchunk > 1 || rd > 0) __syncthreads();
                    for (int idx = tid; idx < XCG_ROWS * kw; idx += 256) {
                        const int r = idx / kw, k = idx - r * kw;
                        const long g = g0 + r;
                        const int col = k0 + k;
                        double a = 0.0, qa = 0.0, qb = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
                        if (g < ngrid && col < nao) {
                            const size_t o = (size_t)g * nao + col;
                            vx = gx[o]; vy = gy[o]; vz = gz[o];
                            a = ao[o];
                            const double *c4 = cs + r;
                            qa = 2.0 * c4[0] * a + c4[16] * vx + c4[32] * vy + c4[48] * vz;
                            qb = 2.0 * c4[64] * a + c4[80] * vx + c4[96] * vy + c4[112] * vz;
                        }
                        double *t0 = T + r * ldk + k;
                        t0[0] = a;
                        t0[qsz] = qa;
                        t0[2 * qsz] = qb;
                        t0[3 * qsz] = vx;
                        t0[4 * qsz] = vy;
                        t0[5 * qsz] = vz;
                    }
                    __syncthreads();
                }
                if (active) {
                    const double *arow = T + li * ldk + lk;
                    const size_t bo = (size_t)(k0 + lk) * NP + 16 * j + li;
                    const double *bcol_a = Dp_a + bo, *bcol_b = Dp_b + bo;
                    for (int ks = 0; ks < kw; ks += 4) {
                        const double ba = bcol_a[(size_t)ks * NP], bb = bcol_b[(size_t)ks * NP];
                        const double a = arow[ks], vx = arow[3 * qsz + ks], vy = arow[4 * qsz + ks], vz = arow[5 * qsz + ks];
                        acc[0][0] = mfma_f64(a, ba, acc[0][0]);
                        acc[1][0] = mfma_f64(a, bb, acc[1][0]);
                        acc[0][1] = mfma_f64(arow[qsz + ks], ba, acc[0][1]);
                        acc[1][1] = mfma_f64(arow[2 * qsz + ks], bb, acc[1][1]);
                        acc[0][2] = mfma_f64(vx, ba, acc[0][2]);
                        acc[1][2] = mfma_f64(vx, bb, acc[1][2]);
                        acc[0][3] = mfma_f64(vy, ba, acc[0][3]);
                        acc[1][3] = mfma_f64(vy, bb, acc[1][3]);
                        acc[0][4] = mfma_f64(vz, ba, acc[0][4]);
                        acc[1][4] = mfma_f64(vz, bb, acc[1][4]);
                    }
                }
            }
            const int mu = 16 * j + li;
            double sx = 0.0, sy = 0.0, sz = 0.0;
            if (active && mu < nao) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = lk + 4 * r;
                    const long g = g0 + row;
                    if (g < ngrid) {
                        const size_t o = (size_t)g * nao + mu;
                        const double hxx = hess[o], hxy = hess[plane + o], hxz = hess[2 * plane + o],
                                     hyy = hess[3 * plane + o], hyz = hess[4 * plane + o], hzz = hess[5 * plane + o];
                        const double Z = acc[0][1][r] + acc[1][1][r];
                        sx += gx[o] * Z;
                        sy += gy[o] * Z;
                        sz += gz[o] * Z;
#pragma unroll
                        for (int s = 0; s < 2; ++s) {   // k_xc_grad_meta<true>'s lines, in its order of operations
                            const double *c4 = cs + 64 * s + row;
                            const double c1 = c4[16], c2 = c4[32], c3 = c4[48], X = acc[s][0][r];
                            sx += (c1 * hxx + c2 * hxy + c3 * hxz) * X;
                            sy += (c1 * hxy + c2 * hyy + c3 * hyz) * X;
                            sz += (c1 * hxz + c2 * hyz + c3 * hzz) * X;
                            const double t2 = 2.0 * cs[128 + 16 * s + row];
                            const double Yx = acc[s][2][r], Yy = acc[s][3][r], Yz = acc[s][4][r];
                            sx += t2 * (hxx * Yx + hxy * Yy + hxz * Yz);
                            sy += t2 * (hxy * Yx + hyy * Yy + hyz * Yz);
                            sz += t2 * (hxz * Yx + hyz * Yy + hzz * Yz);
                        }
                    }
                }
            }
            // the four lanes that share a column (lk = 0..3): every lane gets the total, lk = 0 keeps it
            sx += __shfl_xor(sx, 16, 64); sx += __shfl_xor(sx, 32, 64);
            sy += __shfl_xor(sy, 16, 64); sy += __shfl_xor(sy, 32, 64);
            sz += __shfl_xor(sz, 16, 64); sz += __shfl_xor(sz, 32, 64);
            if (active && lk == 0) {   // column tile j belongs to this wave in every tile of rows: no other writer
                Gs[3 * mu] += sx;
                Gs[3 * mu + 1] += sy;
                Gs[3 * mu + 2] += sz;
            }
        }
    }
    __syncthreads();
    double *slab = slabs + (size_t)blockIdx.x * 3 * nao;
    for (int i = tid; i < 3 * nao; i += 256) slab[i] = -Gs[i];
}

__global__ __launch_bounds__(256) void k_xc_edens_meta_spin(long ngrid, const double *__restrict__ rho_a, const double *__restrict__ rho_b,
                                                            const double *__restrict__ grad_a, const double *__restrict__ grad_b,
                                                            const double *__restrict__ tau_a, const double *__restrict__ tau_b,
                                                            double *__restrict__ e, xc::MixWeights m, xc::MetaWeights mm)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    e[g] = xc::meta_spin_point(m, mm, rho_a[g], rho_b[g], grad_a[3 * g], grad_a[3 * g + 1], grad_a[3 * g + 2], grad_b[3 * g],
                               grad_b[3 * g + 1], grad_b[3 * g + 2], tau_a[g], tau_b[g], 1.0).e;
}

XcGradPlan xc_grad_meta_spin_plan(int num_cu, long ngrid, int nao)
{
    XcGradPlan p;
    p.NP = ((nao + 15) / 16) * 16;
    p.kc = std::min(p.NP, XCGMS_KC_MAX);
    p.ldk = p.kc | 1;
    p.lds = sizeof(double) * ((size_t)6 * XCG_ROWS * p.ldk + 3 * (size_t)p.NP + 160);
    const long ntile = (ngrid + XCG_ROWS - 1) / XCG_ROWS;
    const long per_cu = std::max<long>(1, std::min<long>(8, (160 * 1024) / (long)(p.lds + 512)));
    p.nwg = (int)std::min<long>(ntile, per_cu * num_cu);
    return p;
}

hipError_t launch_xc_grad_meta_spin_fused(hipStream_t st, const XcGradPlan &p, long ngrid, int nao, const double *ao, const double *ao_grad,
                                          const double *hess, const double *coef_a, const double *coef_b, const double *ct_a,
                                          const double *ct_b, const double *Dp_a, const double *Dp_b, double *slabs, double *out)
{
    if (p.lds > 160 * 1024 || p.nwg <= 0) return hipErrorInvalidValue;
    static size_t allowed = 48 * 1024;
    if (p.lds > allowed) {   // dynamic LDS above the default needs the attribute once
        const hipError_t e = hipFuncSetAttribute((const void *)k_xc_grad_meta_spin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        allowed = p.lds;
    }
    const size_t plane = (size_t)ngrid * nao;
    hipLaunchKernelGGL(k_xc_grad_meta_spin, dim3((unsigned)p.nwg), dim3(256), p.lds, st, ngrid, nao, p.NP, p.kc, p.ldk, ao, ao_grad,
                       ao_grad + plane, ao_grad + 2 * plane, hess, coef_a, coef_b, ct_a, ct_b, Dp_a, Dp_b, slabs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_xc_grad_sum(st, nao, p.nwg, slabs, out);
}

hipError_t launch_xc_grad_meta_spin_plain(hipStream_t st, const XcGradPlan &pg, const XcGradPlan &pt, long ngrid, int nao, const double *ao,
                                          const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                                          const double *ct_a, const double *ct_b, const double *Dp_a, const double *Dp_b, double *slabs,
                                          double *out)
{
    const size_t sg = (size_t)pg.nwg * 3 * nao, stau = (size_t)pt.nwg * 3 * nao;
    const double *const coef[2] = {coef_a, coef_b}, *const ct[2] = {ct_a, ct_b}, *const Dp[2] = {Dp_a, Dp_b};
    for (int s = 0; s < 2; ++s) {
        double *base = slabs + s * (sg + stau);
        hipError_t e = launch_xc_grad_gga_slabs(st, pg, 1.0, ngrid, nao, ao, ao_grad, hess, coef[s], Dp[s], base);
        if (e != hipSuccess) return e;
        e = launch_xc_grad_tau_slabs(st, pt, ngrid, nao, ao_grad, hess, ct[s], Dp[s], base + sg);
        if (e != hipSuccess) return e;
    }
    return launch_xc_grad_sum(st, nao, 2 * (pg.nwg + pt.nwg), slabs, out);
}

hipError_t launch_xc_edens_meta_spin(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho_a,
                                     const double *rho_b, const double *grad_a, const double *grad_b, const double *tau_a,
                                     const double *tau_b, double *e)
{
    xc::MixWeights m;
    for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    hipLaunchKernelGGL(k_xc_edens_meta_spin, dim3((unsigned)((ngrid + 255) / 256)), dim3(256), 0, st, ngrid, rho_a, rho_b, grad_a, grad_b,
                       tau_a, tau_b, e, m, mm);
    return hipGetLastError();
}

} // namespace qcdft
