// Spin-resolved part of the meta-GGA sweep (DFT_ComputeTauSpin / DFT_ComputeXCMetaSpin, dft_api.hip).
//
// k_tau_spin: k_tau (xc_meta.hip) for the matrices of both spins at once.  The rows of the three gradient planes of a tile
// are staged once and serve both spins; each MFMA step reads its A operand from LDS once and the B operand of each spin
// (Dp_a, Dp_b, zero-padded to NP) from L2, into six accumulators; the epilogue runs per spin.  Per spin the operations and
// their order are k_tau's, the four waves meet through red[2][4][16] in the same fixed order, every tau_s[g] has one
// writer, no atomics.  Rows past the grid and columns past nao are staged as zeros and masked in the epilogue: no
// out-of-range read.
//
// k_xc_points_meta_spin: xc::meta_spin_point per grid point (xc_meta_functionals.hpp), seven derivatives by xc::Dual.
#include "xc_meta_functionals.hpp"
#include "xc_meta_spin_launch.hpp"
#include "device_util.hpp"
#include <algorithm>

namespace qcdft {

// Dynamic LDS: Gs[3][16 * ldk], red[2][4][16].  kc: K chunk, a multiple of 16; ldk = kc | 1.
__global__ __launch_bounds__(256) void k_tau_spin(long ngrid, int nao, int NP, int kc, int ldk, const double *__restrict__ gx,
                                                  const double *__restrict__ gy, const double *__restrict__ gz,
                                                  const double *__restrict__ Dpa, const double *__restrict__ Dpb,
                                                  double *__restrict__ tau_a, double *__restrict__ tau_b)
{
    extern __shared__ double lds[];
    const int qsz = META_ROWS * ldk;   // one staged tile
    double *Gs = lds;                  // plane k at Gs + k * qsz
    double *red = Gs + 3 * qsz;        // the row sums of spin s, wave w at red + 64 s + 16 w
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nct = NP / 16, nround = (nct + 3) / 4, nchunk = (NP + kc - 1) / kc;
    const long ntile = (ngrid + META_ROWS - 1) / META_ROWS;

    for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const long g0 = tl * META_ROWS;
        __syncthreads();   // the previous tile's readers of the staged rows and of red are done
        double tsa[4] = {0.0, 0.0, 0.0, 0.0}, tsb[4] = {0.0, 0.0, 0.0, 0.0};   // rows lk + 4 r, summed over this wave's column tiles
        for (int rd = 0; rd < nround; ++rd) {
            const int j = rd * 4 + wave;
            const bool active = j < nct;   // wave-uniform
            d4 aa[3], ab[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                aa[k] = (d4){0.0, 0.0, 0.0, 0.0};
                ab[k] = (d4){0.0, 0.0, 0.0, 0.0};
            }
            for (int c = 0; c < nchunk; ++c) {
                const int k0 = c * kc, kw = min(kc, NP - k0);
                if (nchunk > 1 || rd == 0) {   // block-uniform: one staging per tile while the whole row fits
                    if (nchunk > 1) __syncthreads();
                    for (int idx = tid; idx < META_ROWS * kw; idx += 256) {
                        const int r = idx / kw, k = idx - r * kw;
                        const long g = g0 + r;
                        const int col = k0 + k;
                        double vx = 0.0, vy = 0.0, vz = 0.0;
                        if (g < ngrid && col < nao) {
                            const size_t o = (size_t)g * nao + col;
                            vx = gx[o]; vy = gy[o]; vz = gz[o];
                        }
                        Gs[r * ldk + k] = vx;
                        Gs[qsz + r * ldk + k] = vy;
                        Gs[2 * qsz + r * ldk + k] = vz;
                    }
                    __syncthreads();
                }
                if (active) {
                    const double *arow = Gs + li * ldk + lk;
                    const size_t bo = (size_t)(k0 + lk) * NP + 16 * j + li;
                    const double *bca = Dpa + bo, *bcb = Dpb + bo;
                    for (int ks = 0; ks < kw; ks += 4) {
                        const double ba = bca[(size_t)ks * NP], bb = bcb[(size_t)ks * NP];
                        const double ax = arow[ks], ay = arow[qsz + ks], az = arow[2 * qsz + ks];
                        aa[0] = mfma_f64(ax, ba, aa[0]);
                        aa[1] = mfma_f64(ay, ba, aa[1]);
                        aa[2] = mfma_f64(az, ba, aa[2]);
                        ab[0] = mfma_f64(ax, bb, ab[0]);
                        ab[1] = mfma_f64(ay, bb, ab[1]);
                        ab[2] = mfma_f64(az, bb, ab[2]);
                    }
                }
            }
            const int mu = 16 * j + li;
            if (active && mu < nao) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = lk + 4 * r;
                    const long g = g0 + row;
                    if (g < ngrid) {
                        double vx, vy, vz;
                        if (nchunk == 1) {   // the whole row is still staged
                            const double *q = Gs + row * ldk + mu;
                            vx = q[0]; vy = q[qsz]; vz = q[2 * qsz];
                        } else {
                            const size_t o = (size_t)g * nao + mu;
                            vx = gx[o]; vy = gy[o]; vz = gz[o];
                        }
                        tsa[r] += aa[0][r] * vx + aa[1][r] * vy + aa[2][r] * vz;
                        tsb[r] += ab[0][r] * vx + ab[1][r] * vy + ab[2][r] * vz;
                    }
                }
            }
        }
        // the 16 lanes that share a row (li = 0..15): every lane gets the total, li = 0 keeps it
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = tsa[r], u = tsb[r];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            u += __shfl_xor(u, 1, 64); u += __shfl_xor(u, 2, 64); u += __shfl_xor(u, 4, 64); u += __shfl_xor(u, 8, 64);
            if (li == 0) {
                red[16 * wave + lk + 4 * r] = v;
                red[64 + 16 * wave + lk + 4 * r] = u;
            }
        }
        __syncthreads();
        if (tid < 2 * META_ROWS) {
            const int sp = tid >> 4, row = tid & 15;
            if (g0 + row < ngrid) {
                const double *q = red + 64 * sp + row;
                (sp ? tau_b : tau_a)[g0 + row] = 0.5 * ((q[0] + q[16]) + (q[32] + q[48]));
            }
        }
    }
}

// Each block leaves one deterministic partial of sum_g w_g e_g, in the reduction shape of k_xc_points_meta.
__global__ __launch_bounds__(256) void k_xc_points_meta_spin(long ngrid, const double *__restrict__ rho_a, const double *__restrict__ rho_b,
                                                             const double *__restrict__ grad_a, const double *__restrict__ grad_b,
                                                             const double *__restrict__ tau_a, const double *__restrict__ tau_b,
                                                             const double *__restrict__ w, double *__restrict__ coef_a,
                                                             double *__restrict__ coef_b, double *__restrict__ ct_a,
                                                             double *__restrict__ ct_b, double *__restrict__ partial, xc::MixWeights m,
                                                             xc::MetaWeights mm)
{
    __shared__ double red[4];
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (g < ngrid) {
        const size_t n = (size_t)ngrid;
        const double wt = w[g];
        const xc::MetaSpinPoint p = xc::meta_spin_point(m, mm, rho_a[g], rho_b[g], grad_a[3 * g], grad_a[3 * g + 1], grad_a[3 * g + 2],
                                                        grad_b[3 * g], grad_b[3 * g + 1], grad_b[3 * g + 2], tau_a[g], tau_b[g], wt);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            coef_a[k * n + g] = p.a[k];
            coef_b[k * n + g] = p.b[k];
        }
        ct_a[g] = p.cta;
        ct_b[g] = p.ctb;
        e = wt * p.e;
    }
    for (int k = 32; k >= 1; k >>= 1) e += __shfl_down(e, k, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

TauPlan tau_spin_plan(int num_cu, long ngrid, int nao)
{
    TauPlan p = tau_plan(num_cu, ngrid, nao);
    p.lds += sizeof(double) * 64;   // the second spin's row sums
    const long ntile = (ngrid + META_ROWS - 1) / META_ROWS;
    const long per_cu = std::max<long>(1, std::min<long>(8, (160 * 1024) / (long)(p.lds + 512)));
    p.nwg = (int)std::min<long>(ntile, per_cu * num_cu);
    return p;
}

hipError_t launch_tau_spin(hipStream_t st, const TauPlan &p, long ngrid, int nao, const double *ao_grad, const double *Dp_a,
                           const double *Dp_b, double *tau_a, double *tau_b)
{
    if (p.lds > 160 * 1024 || p.nwg <= 0) return hipErrorInvalidValue;
    static size_t allowed = 48 * 1024;
    if (p.lds > allowed) {   // dynamic LDS above the default needs the attribute once
        const hipError_t e = hipFuncSetAttribute((const void *)k_tau_spin, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        allowed = p.lds;
    }
    const size_t plane = (size_t)ngrid * nao;
    hipLaunchKernelGGL(k_tau_spin, dim3((unsigned)p.nwg), dim3(256), p.lds, st, ngrid, nao, p.NP, p.kc, p.ldk, ao_grad, ao_grad + plane,
                       ao_grad + 2 * plane, Dp_a, Dp_b, tau_a, tau_b);
    return hipGetLastError();
}

hipError_t launch_xc_points_meta_spin(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho_a,
                                      const double *rho_b, const double *grad_a, const double *grad_b, const double *tau_a,
                                      const double *tau_b, const double *w, double *coef_a, double *coef_b, double *ct_a,
                                      double *ct_b, double *partial)
{
    xc::MixWeights m;
    for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    hipLaunchKernelGGL(k_xc_points_meta_spin, dim3((unsigned)meta_points_blocks(ngrid)), dim3(256), 0, st, ngrid, rho_a, rho_b, grad_a,
                       grad_b, tau_a, tau_b, w, coef_a, coef_b, ct_a, ct_b, partial, m, mm);
    return hipGetLastError();
}

} // namespace qcdft
