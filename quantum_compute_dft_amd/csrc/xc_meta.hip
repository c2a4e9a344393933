// Meta-GGA part of the closed-shell sweep (DFT_ComputeTau / DFT_ComputeXCMeta, dft_api.hip).
//
// A meta-GGA reads, beside rho and grad rho, the kinetic-energy density
//
//     tau(g) = (1/2) sum_k sum_mu,nu D[mu, nu] (d_k phi_mu)(g) (d_k phi_nu)(g),
//
// and its potential gains the term T = sum_k (d_k AO)^T diag(ct) (d_k AO), ct = w e_tau / 2 (dExc / dD of the tau
// dependence; symmetric).  rho, grad rho and the rho / sigma part of the potential are the sweep's own kernels.
//
// k_tau: a workgroup (4 waves) owns tiles of 16 grid rows, k_xc_grad's shape.  The rows of the three gradient planes of a
// tile are staged once in LDS (all columns while NP <= META_KC_MAX; wider bases go through K chunks and restage per round
// of column tiles); wave w takes the column tiles w, w + 4, ... and forms Y_k = (d_k AO) D of each on v_mfma_f64_16x16x4
// with the B operand (D, zero-padded to NP = 16 ceil(nao / 16)) straight from L2.  The epilogue multiplies Y_k with the
// plane elements at the positions of the result layout and sums over columns: 16 lanes by shuffles, the column tiles of
// a wave in registers, the four waves through LDS in a fixed order.  Rows past the grid and columns past nao are staged
// as zeros and masked in the epilogue: no out-of-range read.  No atomics: every tau[g] has one writer.
//
// k_xc_points_meta: xc::meta_point per grid point (xc_meta_functionals.hpp), the derivatives by xc::Dual.
//
// k_vxc_tau: blockIdx.x = a chunk of grid rows, blockIdx.y = a pair (a block <= b block) of 128-wide column blocks.  Per
// 32 grid rows and per plane k, ct (d_k AO)[:, a block] and (d_k AO)[:, b block] are staged in LDS (k_vxc_mfma's layout)
// and the four waves add 4 x 4 MFMA tiles each into the 128 x 128 block, which stays in registers over all three planes
// and the whole chunk: one pass over the planes.  A block above the diagonal is stored twice (T is symmetric), so every
// slab element has one writer; k_vxc_tau_reduce adds the slabs in slab order to what the rho / sigma stage wrote.
#include "xc_meta_functionals.hpp"
#include "xc_meta_launch.hpp"
#include "device_util.hpp"
#include <algorithm>

namespace qcdft {

// Dynamic LDS: Gs[3][16 * ldk], red[4][16].  kc: K chunk, a multiple of 16; ldk = kc | 1.
__global__ __launch_bounds__(256) void k_tau(long ngrid, int nao, int NP, int kc, int ldk, const double *__restrict__ gx,
                                             const double *__restrict__ gy, const double *__restrict__ gz,
                                             const double *__restrict__ Dp, double *__restrict__ tau)
{
    extern __shared__ double lds[];
    const int qsz = META_ROWS * ldk;   // one staged tile
    double *Gs = lds;                  // plane k at Gs + k * qsz
    double *red = Gs + 3 * qsz;        // the row sums of wave w at red + 16 w
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int nct = NP / 16, nround = (nct + 3) / 4, nchunk = (NP + kc - 1) / kc;
    const long ntile = (ngrid + META_ROWS - 1) / META_ROWS;

    for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const long g0 = tl * META_ROWS;
        __syncthreads();   // the previous tile's readers of the staged rows and of red are done
        double ts[4] = {0.0, 0.0, 0.0, 0.0};   // rows lk + 4 r, summed over this wave's column tiles
        for (int rd = 0; rd < nround; ++rd) {
            const int j = rd * 4 + wave;
            const bool active = j < nct;   // wave-uniform
            d4 acc[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = (d4){0.0, 0.0, 0.0, 0.0};
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
                    const double *bcol = Dp + (size_t)(k0 + lk) * NP + 16 * j + li;
                    for (int ks = 0; ks < kw; ks += 4) {
                        const double b = bcol[(size_t)ks * NP];
                        acc[0] = mfma_f64(arow[ks], b, acc[0]);
                        acc[1] = mfma_f64(arow[qsz + ks], b, acc[1]);
                        acc[2] = mfma_f64(arow[2 * qsz + ks], b, acc[2]);
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
                        ts[r] += acc[0][r] * vx + acc[1][r] * vy + acc[2][r] * vz;
                    }
                }
            }
        }
        // the 16 lanes that share a row (li = 0..15): every lane gets the total, li = 0 keeps it
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = ts[r];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            if (li == 0) red[16 * wave + lk + 4 * r] = v;
        }
        __syncthreads();
        if (tid < META_ROWS && g0 + tid < ngrid)
            tau[g0 + tid] = 0.5 * ((red[tid] + red[16 + tid]) + (red[32 + tid] + red[48 + tid]));
    }
}

// Each block leaves one deterministic partial of sum_g w_g e_g, in the reduction shape of k_xc_points.
__global__ __launch_bounds__(256) void k_xc_points_meta(long ngrid, const double *__restrict__ rho, const double *__restrict__ grad,
                                                        const double *__restrict__ tau, const double *__restrict__ w,
                                                        double *__restrict__ coef, double *__restrict__ ct,
                                                        double *__restrict__ partial, xc::MixWeights m, xc::MetaWeights mm)
{
    __shared__ double red[4];
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (g < ngrid) {
        const size_t n = (size_t)ngrid;
        const double wt = w[g];
        const xc::MetaPoint p = xc::meta_point(m, mm, rho[g], grad[3 * g], grad[3 * g + 1], grad[3 * g + 2], tau[g], wt);
        coef[g] = p.c[0];
        coef[n + g] = p.c[1];
        coef[2 * n + g] = p.c[2];
        coef[3 * n + g] = p.c[3];
        ct[g] = p.ct;
        e = wt * p.e;
    }
    for (int k = 32; k >= 1; k >>= 1) e += __shfl_down(e, k, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void k_vxc_tau(long ngrid, int nao, long chunk, int nblk, const double *__restrict__ gx,
                                                 const double *__restrict__ gy, const double *__restrict__ gz,
                                                 const double *__restrict__ ct, double *__restrict__ slabs)
{
    constexpr int G = META_VG, LD = 144;
    __shared__ double Ps[G * LD];
    __shared__ double Qs[G * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wa = wave >> 1, wb = wave & 1;
    int by = 0, rem = blockIdx.y;   // the pair: by <= bz
    while (rem >= nblk - by) { rem -= nblk - by; ++by; }
    const int bz = by + rem;
    const int a0 = by * 128, b0 = bz * 128;
    const long glo = (long)blockIdx.x * chunk;
    const long ghi = min(ngrid, glo + chunk);

    bool act_a[4], act_b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        act_a[i] = a0 + (4 * wa + i) * 16 < nao;
        act_b[i] = b0 + (4 * wb + i) * 16 < nao;
    }
    d4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};

    for (long gt = glo; gt < ghi; gt += G) {
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
            const double *pl = k == 0 ? gx : k == 1 ? gy : gz;
            {
                const int c = tid & 127, r0 = tid >> 7;
                const int ca = a0 + c, cb = b0 + c;
#pragma unroll 4
                for (int p = 0; p < 16; ++p) {
                    const int r = r0 + 2 * p;
                    const long g = gt + r;
                    double q = 0.0, pv = 0.0;
                    if (g < ghi) {
                        if (ca < nao) q = ct[g] * pl[(size_t)g * nao + ca];
                        if (cb < nao) pv = pl[(size_t)g * nao + cb];
                    }
                    Qs[r * LD + c] = q;
                    Ps[r * LD + c] = pv;
                }
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < G / 4; ++ks) {
                const int row = (ks * 4 + lk) * LD + li;
                double af[4], bf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    af[i] = Qs[row + (4 * wa + i) * 16];
                    bf[i] = Ps[row + (4 * wb + i) * 16];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (act_a[i] && act_b[j]) acc[i][j] = mfma_f64(af[i], bf[j], acc[i][j]);
            }
            __syncthreads();
        }
    }

    double *slab = slabs + (size_t)blockIdx.x * nao * nao;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = b0 + (4 * wb + j) * 16 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = a0 + (4 * wa + i) * 16 + lk + 4 * r;
                if (a < nao && b < nao) {
                    slab[(size_t)a * nao + b] = acc[i][j][r];
                    if (by != bz) slab[(size_t)b * nao + a] = acc[i][j][r];
                }
            }
        }
}

// vxc[i] += the sum of the slabs in slab order, i < n
__global__ __launch_bounds__(256) void k_vxc_tau_reduce(long n, int nslab, const double *__restrict__ slabs, double *__restrict__ vxc)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += slabs[(size_t)k * n + i];
    vxc[i] += s;
}

__global__ __launch_bounds__(256) void k_meta_add(long n, const double *__restrict__ t, double *__restrict__ vxc)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) vxc[i] += t[i];
}

TauPlan tau_plan(int num_cu, long ngrid, int nao)
{
    TauPlan p;
    p.NP = ((nao + 15) / 16) * 16;
    p.kc = std::min(p.NP, META_KC_MAX);
    p.ldk = p.kc | 1;
    p.lds = sizeof(double) * (3 * (size_t)META_ROWS * p.ldk + 64);
    const long ntile = (ngrid + META_ROWS - 1) / META_ROWS;
    const long per_cu = std::max<long>(1, std::min<long>(8, (160 * 1024) / (long)(p.lds + 512)));
    p.nwg = (int)std::min<long>(ntile, per_cu * num_cu);
    return p;
}

hipError_t launch_tau(hipStream_t st, const TauPlan &p, long ngrid, int nao, const double *ao_grad, const double *Dp, double *tau)
{
    if (p.lds > 160 * 1024 || p.nwg <= 0) return hipErrorInvalidValue;
    static size_t allowed = 48 * 1024;
    if (p.lds > allowed) {   // dynamic LDS above the default needs the attribute once
        const hipError_t e = hipFuncSetAttribute((const void *)k_tau, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
        allowed = p.lds;
    }
    const size_t plane = (size_t)ngrid * nao;
    hipLaunchKernelGGL(k_tau, dim3((unsigned)p.nwg), dim3(256), p.lds, st, ngrid, nao, p.NP, p.kc, p.ldk, ao_grad, ao_grad + plane,
                       ao_grad + 2 * plane, Dp, tau);
    return hipGetLastError();
}

hipError_t launch_xc_points_meta(hipStream_t st, const double *mix8, const double *meta2, long ngrid, const double *rho,
                                 const double *grad, const double *tau, const double *w, double *coef, double *ct, double *partial)
{
    xc::MixWeights m;
    for (int k = 0; k < 8; ++k) m.c[k] = mix8[k];
    const xc::MetaWeights mm = {{meta2[0], meta2[1]}};
    hipLaunchKernelGGL(k_xc_points_meta, dim3((unsigned)meta_points_blocks(ngrid)), dim3(256), 0, st, ngrid, rho, grad, tau, w, coef, ct,
                       partial, m, mm);
    return hipGetLastError();
}

VxcTauPlan vxc_tau_plan(int num_cu, long ngrid, int nao)
{
    VxcTauPlan p;
    p.nblk = (nao + 127) / 128;
    const long npair = (long)p.nblk * (p.nblk + 1) / 2;
    // enough workgroups to fill the chip twice over, >= 256 grid rows each, slabs within 1 GB
    long nsplit = std::max<long>(1, (2L * num_cu + npair - 1) / npair);
    nsplit = std::min<long>(nsplit, (ngrid + 255) / 256);
    nsplit = std::min<long>(nsplit, std::max<long>(1, (long)(1.0e9 / (8.0 * nao * nao))));
    long chunk = (ngrid + nsplit - 1) / nsplit;
    chunk = ((chunk + META_VG - 1) / META_VG) * META_VG;
    p.chunk = chunk;
    p.nslab = (int)((ngrid + chunk - 1) / chunk);
    return p;
}

hipError_t launch_vxc_tau(hipStream_t st, const VxcTauPlan &p, long ngrid, int nao, const double *ao_grad, const double *ct,
                          double *slabs, double *vxc)
{
    const long npair = (long)p.nblk * (p.nblk + 1) / 2;
    if (p.nslab <= 0 || npair > 65535) return hipErrorInvalidValue;
    const size_t plane = (size_t)ngrid * nao;
    hipLaunchKernelGGL(k_vxc_tau, dim3((unsigned)p.nslab, (unsigned)npair), dim3(256), 0, st, ngrid, nao, p.chunk, p.nblk, ao_grad,
                       ao_grad + plane, ao_grad + 2 * plane, ct, slabs);
    const long n = (long)nao * nao;
    hipLaunchKernelGGL(k_vxc_tau_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, p.nslab, slabs, vxc);
    return hipGetLastError();
}

hipError_t launch_meta_add(hipStream_t st, long n, const double *t, double *vxc)
{
    hipLaunchKernelGGL(k_meta_add, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, t, vxc);
    return hipGetLastError();
}

} // namespace qcdft
