// Host interface of the density-matrix factorisation kernels (dm_factor.hip): dm = L L^T by pivoted Cholesky in one
// workgroup, and the transpose of the factor into the (nao, rank) layout the occupied-orbital entries read.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace qcdft {

constexpr int DMF_MIN_NAO = 2, DMF_MAX_NAO = 8192;   // outside: "not factorable" (reason 4)
constexpr int DMF_STATUS_DOUBLES = 4;                // rank, last residual maximum / scale, reason, scale
// reasons (DFT_FactorDensity, info4[2])
constexpr int DMF_OK = 0, DMF_RANK_EXCEEDED = 1, DMF_NOT_PSD = 2, DMF_INCONSISTENT = 3, DMF_SIZE = 4;

// Lt (max_rank, nao): the factor transposed, row k = column k of L; status: DMF_STATUS_DOUBLES doubles.
// 2 <= nao <= DMF_MAX_NAO and 1 <= max_rank <= nao are the caller's to check.
hipError_t launch_dm_factor(hipStream_t st, int nao, int max_rank, double tol, const double *dm, double *Lt, double *status);

// out (nao, rank) C-order = Lt^T
hipError_t launch_dm_factor_pack(hipStream_t st, int nao, int rank, const double *Lt, double *out);

// *flag |= 1 when dm holds a NaN or an infinity (the comparison of k_dm_consistency is false for both)
hipError_t launch_dm_nonfinite(hipStream_t st, int nao, const double *dm, int *flag);

} // namespace qcdft
