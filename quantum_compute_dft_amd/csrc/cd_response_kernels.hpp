// Response J from a factorised ERI for several trial densities at once (DFT_ComputeJKFactorizedResponse).
//
// An excitation solver hands over trial densities  D_k = A B_k^T + B_k A^T  that share their left factor A (the occupied
// orbitals).  With Yt^A_P = A^T L_P (one half transform per call, k_gemm_tn of cd_kernels.hpp)
//     v[k][P] = L_P : D_k = 2 sum_{i,nu} Yt^A_P[i][nu] B_k[nu][i]       k_cdr_dot: reads Yt^A, never L
//     J_k     = sum_P v[k][P] L_P   for up to 8 trials in ONE pass over L   k_cdr_axpy
// where DFT_ComputeJKFactorized streams L twice per trial.  Neither kernel's summation order depends on how many trials
// a launch carries, so a trial's J is bitwise the same alone or in a batch.
#pragma once
#include <hip/hip_runtime.h>

namespace qcdft {

constexpr int CDR_MAXV = 8;   // trials per pass over L: 8 (x2 elements) accumulators per thread

// bt[k][i][nu] = b[k][nu][i]: the right factors in the layout of a Yt block, so k_cdr_dot reads both along nu
__global__ __launch_bounds__(256) void k_cdr_transpose(int nao, int nocc, const double *__restrict__ b,
                                                       double *__restrict__ bt)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x, ne = (long)nao * nocc;
    if (e >= ne) return;
    const int i = (int)(e / nao), nu = (int)(e % nao);
    const size_t k = blockIdx.y;
    bt[k * ne + e] = b[k * ne + (size_t)nu * nocc + i];
}

// v[k][P] = 2 sum_{i,nu} yt[P][i][nu] bt[k][i][nu], one workgroup per vector P, NV trials per element of Yt loaded.
// Wave w takes rows i = w, w + 4, ..., lane l columns nu = l, l + 64, ...; then a fixed tree over the 256 partials.
template <int NV>
__global__ __launch_bounds__(256) void k_cdr_dot(int nao, int nocc, int ldy, int naux, const double *__restrict__ yt,
                                                 const double *__restrict__ bt, double *__restrict__ v)
{
    __shared__ double red[NV][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t P = blockIdx.x, ne = (size_t)nao * nocc;
    double s[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] = 0.0;
    for (int i = wave; i < nocc; i += 4) {
        const double *y = yt + (P * nocc + i) * (size_t)ldy;
        const double *b = bt + (size_t)i * nao;
        for (int nu = lane; nu < nao; nu += 64) {
            const double yv = y[nu];
#pragma unroll
            for (int k = 0; k < NV; ++k) s[k] = fma(yv, b[k * ne + nu], s[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k][tid] = s[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < NV; ++k) red[k][tid] += red[k][tid + w];
        }
        __syncthreads();
    }
    if (tid < NV) v[(size_t)tid * naux + P] = 2.0 * red[tid][0];
}

// part[k][y][e] = sum_{P in slice y} v[k][P] L[P][e] for NV trials: every element of L is loaded once (16 bytes a
// thread with VEC: nao even and L 16-byte aligned) and feeds NV accumulators.  As k_cd_axpy, only elements on or above
// the diagonal of the symmetric L_P are read (a pair that touches the diagonal is read whole); k_sym_from_upper
// fills the rest of each J after the slab sum.
template <int NV, bool VEC>
__global__ __launch_bounds__(256) void k_cdr_axpy(long n2, int n, int naux, int pslice, int nsl,
                                                  const double *__restrict__ L, const double *__restrict__ v,
                                                  double *__restrict__ part)
{
    constexpr int EPT = VEC ? 2 : 1;
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * EPT;
    if (e >= n2) return;
    const int p0 = blockIdx.y * pslice, p1 = min(naux, p0 + pslice);
    const int row = (int)(e / n), col = (int)(e % n);
    double acc[NV][EPT];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int j = 0; j < EPT; ++j) acc[k][j] = 0.0;
    if (col + EPT - 1 >= row) {
#pragma unroll 4
        for (int p = p0; p < p1; ++p) {
            double x[EPT];
            if constexpr (VEC) {
                const double2 t = *reinterpret_cast<const double2 *>(L + (size_t)p * n2 + e);
                x[0] = t.x;
                x[1] = t.y;
            } else {
                x[0] = L[(size_t)p * n2 + e];
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const double vk = v[(size_t)k * naux + p];
#pragma unroll
                for (int j = 0; j < EPT; ++j) acc[k][j] = fma(vk, x[j], acc[k][j]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double *o = part + ((size_t)k * nsl + blockIdx.y) * n2 + e;
        if constexpr (VEC) *reinterpret_cast<double2 *>(o) = make_double2(acc[k][0], acc[k][1]);
        else o[0] = acc[k][0];
    }
}

} // namespace qcdft
