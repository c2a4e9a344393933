// Rank-revealing factorisation of a density matrix on the device: dm = L L^T, L (nao, rank), by pivoted Cholesky.
//
// A caller of the reference's ABI hands over dm and nothing else (DFT_ComputeXC), while the cheaper density step of the
// sweep (xc_occ_kernels.hpp) and the exchange half of DFT_ComputeJKFactorized want a factor of it.  Every closed-shell
// SCF loop produces dm = 2 C_occ C_occ^T (dft.py:181-182, 228): its rank is the number of occupied orbitals, and
// pivoted Cholesky finds that rank and a factor in `rank` steps.  (The factor is not C_occ -- any L with L L^T = dm
// gives the same density on the grid and the same exchange matrix.)
//
// k_pchol: left-looking, ONE workgroup, no cross-workgroup synchronisation of any kind.  Per step k
//   p    = argmax of the residual diagonal d (kept in LDS); ties go to the lowest index: the same bits every run
//   stop   when d_p <= tol * scale, scale = max_i dm_ii (rank = k);  fail when k == max_rank (the loop is bounded by
//          max_rank whatever the input holds, NaN included)
//   col  = (dm[p, :] - L[:, :k] L[p, :k]) / sqrt(d_p);  d -= col^2;  d_p = 0
// and after the last step a residual diagonal entry below -10 tol scale (or NaN) marks an indefinite matrix.
// The factor is kept transposed, Lt (max_rank, nao): a lane per row i then reads Lt[j][i] coalesced over the lanes, and
// the pivot row L[p, :k] -- k strided words -- is staged through LDS once per step.  Rows loop over the lanes when nao
// exceeds the workgroup.  Two barriers per step: behind the waves' argmax candidates and behind the staged pivot row.
// Row p of dm is read where the algorithm says column p: the same numbers for the symmetric matrices that are accepted,
// and contiguous.  Nothing here looks at the other triangle: a non-symmetric dm is caught by the acceptance check the
// caller runs over the whole matrix (k_dm_consistency, cd_kernels.hpp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "dm_factor_launch.hpp"

namespace qcdft {

namespace {

constexpr int DMF_T = 1024;        // lanes of k_pchol at most (16 waves)
constexpr int DMF_W = DMF_T / 64;

struct Cand {
    double v;
    int i;
};

// the larger value, the lower index among equals
__device__ __forceinline__ Cand better(Cand a, Cand b)
{
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}

__device__ __forceinline__ Cand wave_argmax(Cand c)
{
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        Cand o;
        o.v = __shfl_xor(c.v, m, 64);
        o.i = __shfl_xor(c.i, m, 64);
        c = better(c, o);
    }
    return c;
}

__global__ __launch_bounds__(DMF_T) void k_pchol(int nao, int max_rank, double tol, const double *__restrict__ dm,
                                                 double *Lt, double *__restrict__ status)
{
    __shared__ double d[DMF_MAX_NAO];        // residual diagonal
    __shared__ double prow[DMF_MAX_NAO];     // L[p, :k] of the current step
    __shared__ double wv[DMF_W];
    __shared__ int wi[DMF_W];
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = T >> 6;

    Cand mine{-INFINITY, nao};               // NaN never wins a '>' : an all-NaN diagonal leaves the sentinel index
    for (int i = tid; i < nao; i += T) {
        const double v = dm[(size_t)i * nao + i];
        d[i] = v;
        if (v > mine.v) mine = Cand{v, i};
    }
    double scale = 0.0, last = 0.0;
    int rank = 0, reason = DMF_OK;
    for (int k = 0;; ++k) {
        const Cand w = wave_argmax(mine);
        if (lane == 0) { wv[wave] = w.v; wi[wave] = w.i; }
        __syncthreads();
        Cand g{wv[0], wi[0]};
        for (int q = 1; q < nw; ++q) g = better(g, Cand{wv[q], wi[q]});
        // everything below is decided from g alone: the same in every lane
        if (k == 0) {
            scale = g.v;
            if (!(scale > 0.0) || !(scale < INFINITY)) { reason = DMF_NOT_PSD; break; }   // zero matrix, negative or non-finite diagonal
        }
        last = g.v;
        rank = k;
        if (g.v <= tol * scale) break;
        if (k == max_rank) { reason = DMF_RANK_EXCEEDED; break; }
        const int p = g.i;
        if (p < 0 || p >= nao) { reason = DMF_NOT_PSD; break; }
        for (int j = tid; j < k; j += T) prow[j] = Lt[(size_t)j * nao + p];
        __syncthreads();
        const double sq = sqrt(g.v);
        const double *__restrict__ dmp = dm + (size_t)p * nao;
        double *out = Lt + (size_t)k * nao;
        mine = Cand{-INFINITY, nao};
        auto finish = [&](int i, double acc) {
            const double c = (dmp[i] - acc) / sq;
            out[i] = c;
            const double di = i == p ? 0.0 : d[i] - c * c;
            d[i] = di;
            if (di > mine.v) mine = Cand{di, i};
        };
        // One CU streams Lt from L2 at ~57 GB/s whatever the loop looks like (eight loads in flight per lane and two rows
        // side by side measured the same as this form: 5.1 against 5.0 ms at nao 1150, rank 250): the cost is
        // nao rank^2 / 2 words through one CU, what keeping the factorisation in one workgroup means.
        for (int i = tid; i < nao; i += T) {
            double acc = 0.0;
#pragma unroll 4
            for (int j = 0; j < k; ++j) acc += Lt[(size_t)j * nao + i] * prow[j];
            finish(i, acc);
        }
    }
    if (reason == DMF_OK) {
        // each lane re-reads the entries it wrote itself
        const double floor_ = -10.0 * tol * scale;
        int bad = 0;
        for (int i = tid; i < nao; i += T) bad |= !(d[i] >= floor_);
        if (__syncthreads_or(bad)) reason = DMF_NOT_PSD;
        if (rank == 0) reason = DMF_NOT_PSD;
    }
    if (tid == 0) {
        status[0] = (double)rank;   // steps taken (the caller turns a failure into rank 0)
        status[1] = scale > 0.0 ? last / scale : 0.0;
        status[2] = (double)reason;
        status[3] = scale;
    }
}

// out (nao, rank) = Lt (rank, nao)^T through 32 x 32 LDS tiles: both sides coalesced
__global__ __launch_bounds__(256) void k_pchol_pack(int nao, int rank, const double *__restrict__ Lt, double *__restrict__ out)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, i = i0 + tx;
        tile[r][tx] = (k < rank && i < nao) ? Lt[(size_t)k * nao + i] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, k = k0 + tx;
        if (i < nao && k < rank) out[(size_t)i * rank + k] = tile[tx][r];
    }
}

__global__ __launch_bounds__(256) void k_dm_nonfinite(long n2, const double *__restrict__ dm, int *__restrict__ flag)
{
    int bad = 0;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n2; e += (long)gridDim.x * 256) bad |= !(fabs(dm[e]) < INFINITY);
    if (bad) atomicOr(flag, 1);
}

} // namespace

hipError_t launch_dm_factor(hipStream_t st, int nao, int max_rank, double tol, const double *dm, double *Lt, double *status)
{
    if (nao < DMF_MIN_NAO || nao > DMF_MAX_NAO || max_rank < 1 || max_rank > nao) return hipErrorInvalidValue;
    const int T = nao >= DMF_T ? DMF_T : ((nao + 63) / 64) * 64;
    hipLaunchKernelGGL(k_pchol, dim3(1), dim3((unsigned)T), 0, st, nao, max_rank, tol, dm, Lt, status);
    return hipGetLastError();
}

hipError_t launch_dm_factor_pack(hipStream_t st, int nao, int rank, const double *Lt, double *out)
{
    if (nao < 1 || rank < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pchol_pack, dim3((unsigned)((nao + 31) / 32), (unsigned)((rank + 31) / 32)), dim3(256), 0, st, nao, rank, Lt, out);
    return hipGetLastError();
}

hipError_t launch_dm_nonfinite(hipStream_t st, int nao, const double *dm, int *flag)
{
    const long n2 = (long)nao * nao;
    const unsigned nb = (unsigned)((n2 + 255) / 256 < 4096 ? (n2 + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_dm_nonfinite, dim3(nb), dim3(256), 0, st, n2, dm, flag);
    return hipGetLastError();
}

} // namespace qcdft
