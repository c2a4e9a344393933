// XC part of the analytic nuclear gradient of a meta-GGA (DFT_ComputeXCGradientMeta / DFT_ComputeXCEnergyDensityMeta,
// dft_api.hip).
//
// Under the column replacement that defines G (include/dft_solver.h) tau = (1/2) sum_k sum (d_k phi_mu) D (d_k phi_nu)
// changes through d_k phi_mu -> d_k phi_mu - t d_xk phi_mu alone, so with ct = w e_tau / 2 (k_xc_points_meta) and
// Y_k = (d_k AO) D (D symmetric)
//
//     G_meta[mu, x] = G_gga[mu, x; c0..c3] - 2 sum_g ct sum_k d_xk phi_mu Y_k[g, mu]:
//
// the six Hessian planes the GGA force reads already, no third derivatives.
//
// k_xc_grad_meta<FULL>: k_xc_grad's shape (xc_grad.hip).  A workgroup (4 waves) owns tiles of 16 grid rows; wave w takes
// the column tiles w, w + 4, ... on v_mfma_f64_16x16x4 with the B operand (D, zero-padded to NP = 16 ceil(nao / 16))
// straight from L2; one (nao, 3) slab per workgroup, k_xc_grad_reduce sums the slabs in a fixed order: no atomics, a call
// is bitwise reproducible.
//   FULL = false, the tau term alone: the rows of the three gradient planes are staged (k_tau's tiles), Y_x, Y_y, Y_z are
//     formed together and the epilogue reads each Hessian element once for s_x += 2 ct (hxx Y_x + hxy Y_y + hxz Y_z), ...
//   FULL = true, the whole force in one pass over the ten planes: five staged tiles -- AO, Q = 2 c0 AO + sum_k c_k d_k AO
//     and the three gradient planes -- and five accumulators X, Z, Y_x, Y_y, Y_z fed by one B load; the epilogue is
//     k_xc_grad<true, 1>'s plus the tau lines, the gradient and Hessian elements read once.
// Rows past the grid and columns past nao are staged as zeros and masked in the epilogue: no out-of-range read.
//
// k_xc_edens_meta: the energy per volume of xc::meta_point's body (meta_mix_energy at the closed-shell variables) at unit
// weight, one point per thread.
#include "xc_meta_functionals.hpp"
#include "xc_grad_meta_launch.hpp"
#include "device_util.hpp"
#include <algorithm>

namespace qcdft {

// Dynamic LDS: T[NT][16 * ldk] (FULL: AO, Q, d_x, d_y, d_z; else d_x, d_y, d_z), Gs[3 * NP], cs (FULL: c0..c3 of the 16
// rows, then ct; else ct).  kc: K chunk, a multiple of 16; ldk = kc | 1.  coef is not read when !FULL, ao neither.
template <bool FULL>
__global__ __launch_bounds__(256) void k_xc_grad_meta(long ngrid, int nao, int NP, int kc, int ldk, const double *__restrict__ ao,
                                                      const double *__restrict__ gx, const double *__restrict__ gy,
                                                      const double *__restrict__ gz, const double *__restrict__ hess,
                                                      const double *__restrict__ coef, const double *__restrict__ ct,
                                                      const double *__restrict__ Dp, double *__restrict__ slabs)
{
    constexpr int NT = FULL ? 5 : 3;    // staged tiles = accumulators
    constexpr int TG = FULL ? 2 : 0;    // the first gradient-plane tile
    constexpr int NC = FULL ? 80 : 16;  // doubles of cs
    extern __shared__ double lds[];
    const int qsz = XCG_ROWS * ldk;     // one staged tile
    double *T = lds;
    double *Gs = T + NT * qsz;
    double *cs = Gs + 3 * NP;
    const double *cts = cs + NC - 16;   // ct of the 16 rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const size_t ng = (size_t)ngrid, plane = ng * nao;
    const int nct = NP / 16, nround = (nct + 3) / 4, nchunk = (NP + kc - 1) / kc;
    const long ntile = (ngrid + XCG_ROWS - 1) / XCG_ROWS;

    for (int i = tid; i < 3 * NP; i += 256) Gs[i] = 0.0;

    for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const long g0 = tl * XCG_ROWS;
        __syncthreads();   // the previous tile's readers of cs and of the staged rows are done
        if (tid < NC) {
            const int k = tid >> 4, r = tid & 15;
            const long g = g0 + r;
            const double *src = (FULL && k < 4) ? coef + k * ng : ct;
            cs[tid] = g < ngrid ? src[g] : 0.0;
        }
        __syncthreads();
        for (int rd = 0; rd < nround; ++rd) {
            const int j = rd * 4 + wave;
            const bool active = j < nct;   // wave-uniform
            d4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < nchunk; ++c) {
                const int k0 = c * kc, kw = min(kc, NP - k0);
                if (nchunk > 1 || rd == 0) {   // block-uniform: one staging per tile while the whole row fits
                    if (nchunk > 1 || rd > 0) __syncthreads();
                    for (int idx = tid; idx < XCG_ROWS * kw; idx += 256) {
                        const int r = idx / kw, k = idx - r * kw;
                        const long g = g0 + r;
                        const int col = k0 + k;
                        double a = 0.0, q = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
                        if (g < ngrid && col < nao) {
                            const size_t o = (size_t)g * nao + col;
                            vx = gx[o]; vy = gy[o]; vz = gz[o];
                            if (FULL) {
                                a = ao[o];
                                const double *c4 = cs + r;
                                q = 2.0 * c4[0] * a + c4[16] * vx + c4[32] * vy + c4[48] * vz;
                            }
                        }
                        double *t0 = T + r * ldk + k;
                        if (FULL) {
                            t0[0] = a;
                            t0[qsz] = q;
                        }
                        t0[TG * qsz] = vx;
                        t0[(TG + 1) * qsz] = vy;
                        t0[(TG + 2) * qsz] = vz;
                    }
                    __syncthreads();
                }
                if (active) {
                    const double *arow = T + li * ldk + lk;
                    const double *bcol = Dp + (size_t)(k0 + lk) * NP + 16 * j + li;
                    for (int ks = 0; ks < kw; ks += 4) {
                        const double b = bcol[(size_t)ks * NP];
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[t] = mfma_f64(arow[t * qsz + ks], b, acc[t]);
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
                        if (FULL) {   // k_xc_grad<true, 1>'s lines, in its order of operations
                            const double *c4 = cs + row;
                            const double Z = acc[1][r], X = acc[0][r];
                            sx += gx[o] * Z;
                            sy += gy[o] * Z;
                            sz += gz[o] * Z;
                            const double c1 = c4[16], c2 = c4[32], c3 = c4[48];
                            sx += (c1 * hxx + c2 * hxy + c3 * hxz) * X;
                            sy += (c1 * hxy + c2 * hyy + c3 * hyz) * X;
                            sz += (c1 * hxz + c2 * hyz + c3 * hzz) * X;
                        }
                        const double t2 = 2.0 * cts[row];
                        const double Yx = acc[TG][r], Yy = acc[TG + 1][r], Yz = acc[TG + 2][r];
                        sx += t2 * (hxx * Yx + hxy * Yy + hxz * Yz);
                        sy += t2 * (hxy * Yx + hyy * Yy + hyz * Yz);
                        sz += t2 * (hxz * Yx + hyz * Yy + hzz * Yz);
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

__global__ __launch_bounds__(256) void k_xc_edens_meta(long ngrid, const double *__restrict__ rho, const double *__restrict__ grad,
                                                       const double *__restrict__ tau, double *__restrict__ e, xc::MixWeights m,
                                                       xc::MetaWeights mm)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngrid) return;
    e[g] = xc::meta_point(m, mm, rho[g], grad[3 * g], grad[3 * g + 1], grad[3 * g + 2], tau[g], 1.0).e;
}

XcGradPlan xc_grad_meta_plan(int num_cu, bool full, long ngrid, int nao)
{
    XcGradPlan p;
    p.NP = ((nao + 15) / 16) * 16;
    p.kc = std::min(p.NP, full ? XCGM_KC_MAX : XCGT_KC_MAX);
    p.ldk = p.kc | 1;
    p.lds = sizeof(double) * ((size_t)(full ? 5 : 3) * XCG_ROWS * p.ldk + 3 * (size_t)p.NP + (full ? 80 : 16));
    const long ntile = (ngrid + XCG_ROWS - 1) / XCG_ROWS;
    const long per_cu = std::max<long>(1, std::min<long>(8, (160 * 1024) / (long)(p.lds + 512)));
    p.nwg = (int)std::min<long>(ntile, per_cu * num_cu);
    return p;
}

namespace {

// k_xc_grad_meta<FULL> alone: one slab of (nao, 3) per workgroup into `slabs`
template <bool FULL>
hipError_t launch_slabs(hipStream_t st, const XcGradPlan &p, long ngrid, int nao, const double *ao, const double *ao_grad,
                        const double *hess, const double *coef, const double *ct, const double *Dp, double *slabs)
{
    if (p.lds > 160 * 1024 || p.nwg <= 0) return hipErrorInvalidValue;
    static size_t allowed = 48 * 1024;   // of this instantiation
    if (p.lds > allowed) {               // dynamic LDS above the default needs the attribute once
        const hipError_t e = hipFuncSetAttribute((const void *)k_xc_grad_meta<FULL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        allowed = p.lds;
    }
    const size_t plane = (size_t)ngrid * nao;
    hipLaunchKernelGGL(k_xc_grad_meta<FULL>, dim3((unsigned)p.nwg), dim3(256), p.lds, st, ngrid, nao, p.NP, p.kc, p.ldk, ao, ao_grad,
                       ao_grad + plane, ao_grad + 2 * plane, hess, coef, ct, Dp, slabs);
    return hipGetLastError();
}

} // namespace

hipError_t launch_xc_grad_meta_fused(hipStream_t st, const XcGradPlan &p, long ngrid, int nao, const double *ao, const double *ao_grad,
                                     const double *hess, const double *coef, const double *ct, const double *Dp, double *slabs, double *out)
{
    const hipError_t e = launch_slabs<true>(st, p, ngrid, nao, ao, ao_grad, hess, coef, ct, Dp, slabs);
    if (e != hipSuccess) return e;
    return launch_xc_grad_sum(st, nao, p.nwg, slabs, out);
}

hipError_t launch_xc_grad_meta_plain(hipStream_t st, const XcGradPlan &pg, const XcGradPlan &pt, long ngrid, int nao, const double *ao,
                                     const double *ao_grad, const double *hess, const double *coef, const double *ct, const double *Dp,
                                     double *slabs, double *out)
{
    hipError_t e = launch_xc_grad_gga_slabs(st, pg, 1.0, ngrid, nao, ao, ao_grad, hess, coef, Dp, slabs);
    if (e != hipSuccess) return e;
    e = launch_slabs<false>(st, pt, ngrid, nao, ao, ao_grad, hess, coef, ct, Dp, slabs + (size_t)pg.nwg * 3 * nao);
    if (e != hipSuccess) return e;
    return launch_xc_grad_sum(st, nao, pg.nwg + pt.nwg, slabs, out);
}

hipError_t launch_xc_grad_tau_slabs(hipStream_t st, const XcGradPlan &pt, long ngrid, int nao, const double *ao_grad, const double *hess,
                                    const double *ct, const double *Dp, double *slabs)
{
    return launch_slabs<false>(st, pt, ngrid, nao, nullptr, ao_grad, hess, nullptr, ct, Dp, slabs);
}

hipError_t launch_xc_edens_meta(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho, const double *grad,
                                const double *tau, double *e)
{
    xc::MixWeights m;
    for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    hipLaunchKernelGGL(k_xc_edens_meta, dim3((unsigned)((ngrid + 255) / 256)), dim3(256), 0, st, ngrid, rho, grad, tau, e, m, mm);
    return hipGetLastError();
}

} // namespace qcdft
