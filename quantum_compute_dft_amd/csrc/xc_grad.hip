// XC part of the analytic nuclear gradient (DFT_EvalAOHess / DFT_ComputeXCGradient, dft_api.hip).
//
// G[mu, x] = dExc / d(centre of AO mu)_x at fixed grid points and weights.  With a0 = w vrho and a_k = 2 w vsigma grad_k rho
// the derivatives of the energy at a point, moving the centre of column mu by t changes phi_mu by -t d_x phi_mu and
// d_k phi_mu by -t d_xk phi_mu, so
//
//     G[mu, x] = -2 sum_g [ d_x phi_mu (a0 X + sum_k a_k Y_k)[g, mu] + (sum_k a_k d_xk phi_mu) X[g, mu] ],
//     X = AO D,  Y_k = (d_k AO) D                                            (D symmetric).
//
// The sweep hands over c0..c3 in the convention of the solver type (k_xc_points): c0 = a0, c_k = 2 a_k for the one-sided
// types (GGA, mixes; LDA: c0 = a0), c0 = a0 / 2, c_k = a_k for B3LYP (its M + M^T).  In both
//
//     G[mu, x] = -fac sum_g [ d_x phi_mu Z[g, mu] + (sum_k c_k d_xk phi_mu) X[g, mu] ],   Z = Q D,  Q = 2 c0 AO + sum_k c_k d_k AO,
//
// with fac = 1 (one-sided types) or 2 (B3LYP).  An LDA-class solver has Z = 2 c0 X and needs one product only.
//
// k_xc_grad: a workgroup (4 waves) owns tiles of 16 grid rows.  The AO rows and the Q rows of a tile are staged once in
// LDS (all nao columns while nao <= XCG_KC_MAX; wider bases go through K chunks and restage per round of column tiles);
// wave w takes the column tiles w, w + 4, ... and forms X and Z of each on v_mfma_f64_16x16x4 with the B operand (D,
// zero-padded to NP = 16 ceil(nao / 16)) straight from L2.  The epilogue reads the three gradient and six Hessian planes
// at the positions of the result layout -- each plane element once -- and adds into a per-workgroup (nao, 3) in LDS,
// which leaves as one slab; k_xc_grad_reduce sums the slabs in a fixed order, so a call is bitwise reproducible.
// The open-shell gradient (DFT_ComputeXCGradientSpin) is the same formula once per spin with (D_s, c_s).  The kernel is one
// template over the number of (c, D) pairs, k_xc_grad<GGA, NS>: NS = 1 is the closed shell, NS = 2 does both spins in one
// pass over the planes (launch_xc_grad_spin_fused).  launch_xc_grad_spin is the plain form that one is tested against:
// k_xc_grad<GGA, 1> twice into two slab sets and one reduce over both, alpha's slabs first.  One plan function sizes all
// of them (xc_grad_plan, by the number of pairs per launch) and one launch core sets them off (launch_xc_grad_slabs).
// Rows past the grid and columns past nao are staged as zeros and masked in the epilogue: no out-of-range read.
//
// k_eval_ao_hess: the six second-derivative planes in k_eval_ao's conventions (same harmonics, column order and
// AO_EXP_CUT), a kernel of its own.  Write-bound: a workgroup evaluates 8 points x one column block (<= AO_CW columns)
// into LDS and the rows of every plane leave whole.
#include "xc_grad_launch.hpp"
#include "device_util.hpp"
#include <algorithm>

namespace qcdft {

namespace {

// phi = R(r^2) S(x, y, z):  d_ij phi = R0 S_ij + R1 (x_i S_j + x_j S_i + delta_ij S) + R2 x_i x_j S,
// R1 = sum -2 a c e, R2 = sum 4 a^2 c e (dR0/dx = R1 x, dR1/dx = R2 x).
__device__ __forceinline__ void hess_put(double *tile, int psz, int idx, double S, double Sx, double Sy, double Sz,
                                         double Sxx, double Sxy, double Sxz, double Syy, double Syz, double Szz,
                                         double R0, double R1, double R2, double x, double y, double z)
{
    const double t1 = R1 * S, t2 = R2 * S;
    tile[idx] = R0 * Sxx + 2.0 * R1 * x * Sx + t1 + t2 * x * x;
    tile[psz + idx] = R0 * Sxy + R1 * (x * Sy + y * Sx) + t2 * x * y;
    tile[2 * psz + idx] = R0 * Sxz + R1 * (x * Sz + z * Sx) + t2 * x * z;
    tile[3 * psz + idx] = R0 * Syy + 2.0 * R1 * y * Sy + t1 + t2 * y * y;
    tile[4 * psz + idx] = R0 * Syz + R1 * (y * Sz + z * Sy) + t2 * y * z;
    tile[5 * psz + idx] = R0 * Szz + 2.0 * R1 * z * Sz + t1 + t2 * z * z;
}

} // namespace

// blockIdx.x = tile * nchunk + column block.  Dynamic LDS: 6 * AOH_PT * ldt doubles (ldt odd, >= the widest block).
__global__ __launch_bounds__(256) void k_eval_ao_hess(long ngrid, int nao, int nchunk, int ldt,
                                                      const AoShell *__restrict__ sh, const double *__restrict__ pexp,
                                                      const double *__restrict__ pcoef,
                                                      const AoChunk *__restrict__ chunks,
                                                      const double *__restrict__ coords, double *__restrict__ hess)
{
    extern __shared__ double tile[];
    constexpr int PT = AOH_PT, NSLOT = 256 / PT;
    const int psz = PT * ldt;
    const int tid = threadIdx.x, pt = tid % PT, slot = tid / PT;
    const long tl = blockIdx.x / nchunk;
    const AoChunk ch = chunks[blockIdx.x % nchunk];
    const long g0 = tl * PT;
    const long gp = min(g0 + pt, ngrid - 1);   // points past the grid repeat the last one; their rows are not stored
    const double px = coords[3 * gp], py = coords[3 * gp + 1], pz = coords[3 * gp + 2];

    for (int k = ch.shell_lo + slot; k < ch.shell_hi; k += NSLOT) {
        const AoShell q = sh[k];
        const double x = px - q.x, y = py - q.y, z = pz - q.z;
        const double r2 = x * x + y * y + z * z;
        double R0 = 0.0, R1 = 0.0, R2 = 0.0;
        for (int p = 0; p < q.nprim; ++p) {
            const double a = pexp[q.off + p];
            const double t = a * r2;
            const double e = t < AO_EXP_CUT ? pcoef[q.off + p] * exp(-t) : 0.0;
            R0 += e;
            R1 -= 2.0 * a * e;
            R2 += 4.0 * a * a * e;
        }
        const int i0 = pt * ldt + (q.ao - ch.col_lo);
        if (q.l == 0) {
            constexpr double c = 0.282094791773878143;
            hess_put(tile, psz, i0, c, 0, 0, 0, 0, 0, 0, 0, 0, 0, R0, R1, R2, x, y, z);
        } else if (q.l == 1) {
            constexpr double c = 0.488602511902919921;
            hess_put(tile, psz, i0 + 0, c * x, c, 0, 0, 0, 0, 0, 0, 0, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 1, c * y, 0, c, 0, 0, 0, 0, 0, 0, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 2, c * z, 0, 0, c, 0, 0, 0, 0, 0, 0, R0, R1, R2, x, y, z);
        } else if (q.l == 2) {
            constexpr double c = 1.092548430592079070, d = 0.315391565252520002, e = 0.546274215296039535;
            hess_put(tile, psz, i0 + 0, c * x * y, c * y, c * x, 0, 0, c, 0, 0, 0, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 1, c * y * z, 0, c * z, c * y, 0, 0, 0, 0, c, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 2, d * (2 * z * z - x * x - y * y), -2 * d * x, -2 * d * y, 4 * d * z, -2 * d, 0, 0,
                     -2 * d, 0, 4 * d, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 3, c * x * z, c * z, 0, c * x, 0, 0, c, 0, 0, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 4, e * (x * x - y * y), 2 * e * x, -2 * e * y, 0, 2 * e, 0, 0, -2 * e, 0, 0, R0, R1,
                     R2, x, y, z);
        } else {
            constexpr double f3 = 0.590043589926643510, f2 = 2.890611442640554055, f1 = 0.457045799464465739,
                             f0 = 0.373176332590115391, f2b = 1.445305721320277020;
            const double xx = x * x, yy = y * y, zz = z * z;
            hess_put(tile, psz, i0 + 0, f3 * y * (3 * xx - yy), f3 * 6 * x * y, f3 * (3 * xx - 3 * yy), 0,
                     6 * f3 * y, 6 * f3 * x, 0, -6 * f3 * y, 0, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 1, f2 * x * y * z, f2 * y * z, f2 * x * z, f2 * x * y,
                     0, f2 * z, f2 * y, 0, f2 * x, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 2, f1 * y * (4 * zz - xx - yy), -2 * f1 * x * y, f1 * (4 * zz - xx - 3 * yy), 8 * f1 * y * z,
                     -2 * f1 * y, -2 * f1 * x, 0, -6 * f1 * y, 8 * f1 * z, 8 * f1 * y, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 3, f0 * z * (2 * zz - 3 * xx - 3 * yy), -6 * f0 * x * z, -6 * f0 * y * z,
                     f0 * (6 * zz - 3 * xx - 3 * yy),
                     -6 * f0 * z, 0, -6 * f0 * x, -6 * f0 * z, -6 * f0 * y, 12 * f0 * z, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 4, f1 * x * (4 * zz - xx - yy), f1 * (4 * zz - 3 * xx - yy), -2 * f1 * x * y, 8 * f1 * x * z,
                     -6 * f1 * x, -2 * f1 * y, 8 * f1 * z, -2 * f1 * x, 0, 8 * f1 * x, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 5, f2b * z * (xx - yy), 2 * f2b * x * z, -2 * f2b * y * z, f2b * (xx - yy),
                     2 * f2b * z, 0, 2 * f2b * x, -2 * f2b * z, -2 * f2b * y, 0, R0, R1, R2, x, y, z);
            hess_put(tile, psz, i0 + 6, f3 * x * (xx - 3 * yy), f3 * (3 * xx - 3 * yy), -6 * f3 * x * y, 0,
                     6 * f3 * x, -6 * f3 * y, 0, -6 * f3 * x, 0, 0, R0, R1, R2, x, y, z);
        }
    }
    __syncthreads();
    // whole rows: consecutive threads write consecutive columns of one row of one plane
    const size_t plane = (size_t)ngrid * nao;
    const int nelem = PT * ch.ncol;
    for (int idx = tid; idx < nelem; idx += 256) {
        const int r = idx / ch.ncol, c = idx - r * ch.ncol;
        const long g = g0 + r;
        if (g >= ngrid) continue;
        const size_t o = (size_t)g * nao + ch.col_lo + c;
        const double *t0 = tile + r * ldt + c;
#pragma unroll
        for (int p = 0; p < 6; ++p) hess[p * plane + o] = t0[p * psz];
    }
}

// One (coef, D) pair (NS = 1: the closed shell, or one spin of an open-shell state) or both spins' pairs in one pass over the
// planes (NS = 2): the AO rows of a tile are staged once, beside the Q rows of every spin; X_s, Z_s of a column tile are formed
// together, and the epilogue reads each plane element once for
//     d_x phi sum_s Z_s + sum_k d_xk phi sum_s c_sk X_s.
// Two spins keep three 16-row tiles, so their K chunk is capped lower (XCGS_KC_MAX).  coef_b and Dp_b are not read when NS = 1.
// Dynamic LDS: As[16 * ldk], (GGA) Qs[NS][16 * ldk], Gs[3 * NP], cs[NS][4 * 16].  kc: K chunk, a multiple of 16; ldk = kc | 1.
template <bool GGA, int NS>
__global__ __launch_bounds__(256) void k_xc_grad(long ngrid, int nao, int NP, int kc, int ldk, double fac,
                                                 const double *__restrict__ ao, const double *__restrict__ gx,
                                                 const double *__restrict__ gy, const double *__restrict__ gz,
                                                 const double *__restrict__ hess, const double *__restrict__ coef_a,
                                                 const double *__restrict__ coef_b, const double *__restrict__ Dp_a,
                                                 const double *__restrict__ Dp_b, double *__restrict__ slabs)
{
    static_assert(NS == 1 || NS == 2, "one (coef, D) pair or two");
    extern __shared__ double lds[];
    const int qsz = XCG_ROWS * ldk;   // one staged tile
    double *As = lds;
    double *Qs = As + qsz;            // spin s at Qs + s * qsz (GGA only)
    double *Gs = Qs + (GGA ? NS * qsz : 0);
    double *cs = Gs + 3 * NP;         // c0..c3 of the 16 rows, spin s at cs + 64 s
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const size_t ng = (size_t)ngrid, plane = ng * nao;
    const int nct = NP / 16, nround = (nct + 3) / 4, nchunk = (NP + kc - 1) / kc;
    const long ntile = (ngrid + XCG_ROWS - 1) / XCG_ROWS;

    for (int i = tid; i < 3 * NP; i += 256) Gs[i] = 0.0;

    for (long tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const long g0 = tl * XCG_ROWS;
        __syncthreads();   // the previous tile's readers of cs and of the staged rows are done
        if (tid < 64 * NS) {
            const int k = (tid >> 4) & 3, r = tid & 15;
            const long g = g0 + r;
            const double *coef = (NS == 2 && tid >= 64) ? coef_b : coef_a;
            cs[tid] = (g < ngrid && (GGA || k == 0)) ? coef[k * ng + g] : 0.0;
        }
        __syncthreads();
        for (int rd = 0; rd < nround; ++rd) {
            const int j = rd * 4 + wave;
            const bool active = j < nct;   // wave-uniform
            d4 accX[NS], accZ[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) accX[s] = accZ[s] = (d4){0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < nchunk; ++c) {
                const int k0 = c * kc, kw = min(kc, NP - k0);
                if (nchunk > 1 || rd == 0) {   // block-uniform: one staging per tile while the whole row fits
                    if (nchunk > 1 || rd > 0) __syncthreads();
                    for (int idx = tid; idx < XCG_ROWS * kw; idx += 256) {
                        const int r = idx / kw, k = idx - r * kw;
                        const long g = g0 + r;
                        const int col = k0 + k;
                        double a = 0.0, q[NS] = {};
                        if (g < ngrid && col < nao) {
                            const size_t o = (size_t)g * nao + col;
                            a = ao[o];
                            if (GGA) {
                                const double vx = gx[o], vy = gy[o], vz = gz[o];
#pragma unroll
                                for (int s = 0; s < NS; ++s) {
                                    const double *c4 = cs + 64 * s + r;
                                    q[s] = 2.0 * c4[0] * a + c4[16] * vx + c4[32] * vy + c4[48] * vz;
                                }
                            }
                        }
                        As[r * ldk + k] = a;
                        if (GGA) {
#pragma unroll
                            for (int s = 0; s < NS; ++s) Qs[s * qsz + r * ldk + k] = q[s];
                        }
                    }
                    __syncthreads();
                }
                if (active) {
                    const double *arow = As + li * ldk + lk, *qrow = Qs + li * ldk + lk;
                    const size_t bo = (size_t)(k0 + lk) * NP + 16 * j + li;
                    const double *bcol[NS];
                    bcol[0] = Dp_a + bo;
                    if constexpr (NS == 2) bcol[1] = Dp_b + bo;
                    for (int ks = 0; ks < kw; ks += 4) {
                        const double a = arow[ks];
                        double b[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) b[s] = bcol[s][(size_t)ks * NP];
#pragma unroll
                        for (int s = 0; s < NS; ++s) accX[s] = mfma_f64(a, b[s], accX[s]);
                        if (GGA) {
#pragma unroll
                            for (int s = 0; s < NS; ++s) accZ[s] = mfma_f64(qrow[s * qsz + ks], b[s], accZ[s]);
                        }
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
                        const double *c4 = cs + row;
                        double Z;
                        if constexpr (NS == 1) Z = GGA ? accZ[0][r] : 2.0 * c4[0] * accX[0][r];
                        else Z = GGA ? accZ[0][r] + accZ[1][r] : 2.0 * (c4[0] * accX[0][r] + c4[64] * accX[1][r]);
                        sx += gx[o] * Z;
                        sy += gy[o] * Z;
                        sz += gz[o] * Z;
                        if (GGA) {
                            const double hxx = hess[o], hxy = hess[plane + o], hxz = hess[2 * plane + o],
                                         hyy = hess[3 * plane + o], hyz = hess[4 * plane + o], hzz = hess[5 * plane + o];
                            if constexpr (NS == 1) {   // the closed-shell order of operations: the sum over k first, then X
                                const double c1 = c4[16], c2 = c4[32], c3 = c4[48], X = accX[0][r];
                                sx += (c1 * hxx + c2 * hxy + c3 * hxz) * X;
                                sy += (c1 * hxy + c2 * hyy + c3 * hyz) * X;
                                sz += (c1 * hxz + c2 * hyz + c3 * hzz) * X;
                            } else {
                                const double Xa = accX[0][r], Xb = accX[1][r];
                                const double w1 = c4[16] * Xa + c4[80] * Xb, w2 = c4[32] * Xa + c4[96] * Xb,
                                             w3 = c4[48] * Xa + c4[112] * Xb;
                                sx += w1 * hxx + w2 * hxy + w3 * hxz;
                                sy += w1 * hxy + w2 * hyy + w3 * hyz;
                                sz += w1 * hxz + w2 * hyz + w3 * hzz;
                            }
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
    for (int i = tid; i < 3 * nao; i += 256) slab[i] = -fac * Gs[i];
}

// out[i] = sum of the slabs in slab order, i < n
__global__ __launch_bounds__(256) void k_xc_grad_reduce(int n, int nslab, const double *__restrict__ slabs,
                                                        double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < nslab; ++k) s += slabs[(size_t)k * n + i];
    out[i] = s;
}

hipError_t launch_eval_ao_hess(hipStream_t st, long ngrid, int nao, int nchunk, int maxcol, const AoShell *sh,
                               const double *pexp, const double *pcoef, const AoChunk *chunks, const double *coords,
                               double *hess)
{
    const int ldt = maxcol | 1;
    const size_t lds = sizeof(double) * 6 * AOH_PT * ldt;   // <= 6 * 8 * 127 * 8 = 48768 bytes
    const long ntile = (ngrid + AOH_PT - 1) / AOH_PT;
    if (ntile * nchunk > 0x7FFFFFFFL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_eval_ao_hess, dim3((unsigned)(ntile * nchunk)), dim3(256), lds, st, ngrid, nao, nchunk, ldt, sh, pexp,
                       pcoef, chunks, coords, hess);
    return hipGetLastError();
}

XcGradPlan xc_grad_plan(int num_cu, bool gga, int nspin, long ngrid, int nao)
{
    XcGradPlan p;
    p.NP = ((nao + 15) / 16) * 16;
    p.kc = std::min(p.NP, nspin == 2 ? XCGS_KC_MAX : XCG_KC_MAX);
    p.ldk = p.kc | 1;
    p.lds = sizeof(double) * ((size_t)(gga ? 1 + nspin : 1) * XCG_ROWS * p.ldk + 3 * (size_t)p.NP + 64 * (size_t)nspin);
    const long ntile = (ngrid + XCG_ROWS - 1) / XCG_ROWS;
    const long per_cu = std::max<long>(1, std::min<long>(8, (160 * 1024) / (long)(p.lds + 512)));
    p.nwg = (int)std::min<long>(ntile, per_cu * num_cu);
    return p;
}

namespace {

// k_xc_grad<gga, NS> alone: one slab of (nao, 3) per workgroup into `slabs`.  `p`: the plan for NS spins.
template <int NS>
hipError_t launch_xc_grad_slabs(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                                const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                                const double *Dp_a, const double *Dp_b, double *slabs)
{
    if (p.lds > 160 * 1024) return hipErrorInvalidValue;
    const size_t plane = (size_t)ngrid * nao;
    const double *gx = ao_grad, *gy = ao_grad + plane, *gz = ao_grad + 2 * plane;
    auto launch = [&](auto kern, size_t &allowed) -> hipError_t {
        if (p.lds > allowed) {   // per instantiation: dynamic LDS above the default needs the attribute once
            const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
            if (e != hipSuccess) return e;
            allowed = p.lds;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)p.nwg), dim3(256), p.lds, st, ngrid, nao, p.NP, p.kc, p.ldk, fac, ao, gx, gy, gz,
                           hess, coef_a, coef_b, Dp_a, Dp_b, slabs);
        return hipGetLastError();
    };
    static size_t allowed_gga = 48 * 1024, allowed_lda = 48 * 1024;   // of this NS
    return gga ? launch(k_xc_grad<true, NS>, allowed_gga) : launch(k_xc_grad<false, NS>, allowed_lda);
}

hipError_t launch_xc_grad_reduce(hipStream_t st, int nao, int nslab, const double *slabs, double *out)
{
    const int n = 3 * nao;
    hipLaunchKernelGGL(k_xc_grad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, nslab, slabs, out);
    return hipGetLastError();
}

} // namespace

hipError_t launch_xc_grad_gga_slabs(hipStream_t st, const XcGradPlan &p, double fac, long ngrid, int nao, const double *ao,
                                    const double *ao_grad, const double *hess, const double *coef, const double *Dp, double *slabs)
{
    return launch_xc_grad_slabs<1>(st, p, true, fac, ngrid, nao, ao, ao_grad, hess, coef, nullptr, Dp, nullptr, slabs);
}

hipError_t launch_xc_grad_sum(hipStream_t st, int nao, int nslab, const double *slabs, double *out)
{
    return launch_xc_grad_reduce(st, nao, nslab, slabs, out);
}

hipError_t launch_xc_grad(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                          const double *ao_grad, const double *hess, const double *coef, const double *Dp, double *slabs,
                          double *out)
{
    const hipError_t e = launch_xc_grad_slabs<1>(st, p, gga, fac, ngrid, nao, ao, ao_grad, hess, coef, nullptr, Dp, nullptr, slabs);
    if (e != hipSuccess) return e;
    return launch_xc_grad_reduce(st, nao, p.nwg, slabs, out);
}

hipError_t launch_xc_grad_spin_fused(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                                     const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                                     const double *Dp_a, const double *Dp_b, double *slabs, double *out)
{
    const hipError_t e = launch_xc_grad_slabs<2>(st, p, gga, fac, ngrid, nao, ao, ao_grad, hess, coef_a, coef_b, Dp_a, Dp_b, slabs);
    if (e != hipSuccess) return e;
    return launch_xc_grad_reduce(st, nao, p.nwg, slabs, out);
}

hipError_t launch_xc_grad_spin(hipStream_t st, const XcGradPlan &p, bool gga, double fac, long ngrid, int nao, const double *ao,
                               const double *ao_grad, const double *hess, const double *coef_a, const double *coef_b,
                               const double *Dp_a, const double *Dp_b, double *slabs, double *out)
{
    hipError_t e = launch_xc_grad_slabs<1>(st, p, gga, fac, ngrid, nao, ao, ao_grad, hess, coef_a, nullptr, Dp_a, nullptr, slabs);
    if (e != hipSuccess) return e;
    e = launch_xc_grad_slabs<1>(st, p, gga, fac, ngrid, nao, ao, ao_grad, hess, coef_b, nullptr, Dp_b, nullptr,
                                slabs + (size_t)p.nwg * 3 * nao);
    if (e != hipSuccess) return e;
    return launch_xc_grad_reduce(st, nao, 2 * p.nwg, slabs, out);
}

} // namespace qcdft
