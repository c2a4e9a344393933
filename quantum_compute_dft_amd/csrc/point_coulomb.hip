// One-electron Coulomb integrals at points, A[c, mu, nu] = int phi_mu(r) phi_nu(r) / |r - R_c| dr, contracted on the
// device without ever being stored:
//   matrix    M[mu, nu] = sum_c w_c A[c, mu, nu]          (external point charges: V_ext = -M)
//   contract  u[c]      = sum_{mu nu} D[mu, nu] A[c, mu, nu]   (electrostatic potential of a density)
//   field     G[c, k]   = d u[c] / d R_c,k, k = x, y, z        (electric field of a density, forces on point charges)
// Device counterpart of integrals.c::qc_point_matrix / qc_point_contract (same McMurchie-Davidson formulation as the
// nuclear attraction of qc_int1e: same Boys function, same recurrences, same 1e-18 cut on primitive pairs); s-f shells.
//
// Per primitive pair (exponent sum p, centre P, total angular momentum L = la + lb <= 6) and point c
//     A^cart_ab(c) = (2 pi / p) cc sum_tuv E_t^x E_u^y E_v^z R_tuv(p, P - R_c)
// and the (L+1)(L+2)(L+3)/6 Hermite integrals R_tuv are the only thing that depends on the point.  Both hot kernels
// run one point per lane and keep the R table of their lane in REGISTERS: one instantiation per L, every index a
// compile-time constant (a lane-private table indexed at run time would live in scratch memory), the recurrence in
// place (level n overwrites level n + 1 from the highest order down).  What is left is linear in R:
//   contract  k_pc_lambda  (one workgroup per shell pair A >= B) turns D into Hermite densities Lambda_tuv per
//             primitive pair: D[A,B] + D[B,A]^T, solid harmonics -> Cartesians, contraction with E, prefactor;
//             k_pc_contract<L>  u[c] += sum_pairs sum_tuv Lambda_tuv R_tuv, primitive pairs staged through LDS.
//   field     the same k_pc_lambda; k_pc_field<L>  G[c] -= sum_pairs sum_tuv Lambda_tuv (R_t+1,u,v, R_t,u+1,v, R_t,u,v+1)
//             with the table of order L + 1.
//   matrix    k_pc_wsum<L>  (primitive pair x chunk of points) W_tuv = sum_c w_c R_tuv: per-lane sums, a butterfly over
//             the wave, the four waves added in order -- no atomics, the same bits in every run; k_pc_matrix (one
//             workgroup per shell pair) adds the chunks in order, contracts with E, sums the primitive pairs, rotates
//             to solid harmonics and writes the block and its mirror image (a diagonal block: its lower triangle
//             and the mirror of that, so M == M^T bit for bit).
// The primitive pairs are laid out on the host when the handle is opened.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/dft_solver.h"
#include "md_device.hpp"   // boys_fixed, hermite_E, c_cx / c_cy / c_cz, c_sph, fill_tables

namespace {

constexpr int PC_T = 256;      // lanes of the hot kernels: one point each
constexpr int PC_TS = 128;     // lanes of the per-shell-pair kernels
constexpr int PC_TILE = 16;    // primitive pairs staged per LDS tile of k_pc_contract
constexpr int PC_MAXCHUNK = 64;

__host__ __device__ constexpr int ntuv(int L) { return (L + 1) * (L + 2) * (L + 3) / 6; }
// position of (t, u, v), t + u + v <= L, in the order t = 0..L, u = 0..L-t, v = 0..L-t-u
__host__ __device__ constexpr int tuv_index(int L, int t, int u, int v)
{
    return ntuv(L) - ntuv(L - t) + u * (L - t + 1) - u * (u - 1) / 2 + v;
}

template <int I, int N, class F> __device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// R_tuv(p, PC) of order 0 for t + u + v <= L (integrals.c::hermite_R, same recurrence and branch order), in place:
// after step n the table holds auxiliary level n for the orders <= L - n.  An order-s entry reads orders s - 1 and
// s - 2 of the level above, so a level is rewritten from the highest order down.
template <int L> __device__ __forceinline__ void hermite_R_regs(double p, double X, double Y, double Z, double (&R)[ntuv(L)])
{
    double F[L + 1];
    boys_fixed<L>(p * (X * X + Y * Y + Z * Z), F);
    double f = 1.0;
#pragma unroll
    for (int n = 0; n <= L; ++n) { F[n] *= f; f *= -2.0 * p; }
    R[0] = F[L];
    static_for<0, L>([&](auto n_) {
        constexpr int n = L - 1 - decltype(n_)::value;
        static_for<0, L - n>([&](auto s_) {
            constexpr int s = L - n - decltype(s_)::value;
            static_for<0, s + 1>([&](auto t_) {
                constexpr int t = decltype(t_)::value;
                static_for<0, s - t + 1>([&](auto u_) {
                    constexpr int u = decltype(u_)::value, v = s - t - u;
                    double val;
                    if constexpr (t > 0) {
                        val = X * R[tuv_index(L, t - 1, u, v)];
                        if constexpr (t > 1) val += (t - 1) * R[tuv_index(L, t - 2, u, v)];
                    } else if constexpr (u > 0) {
                        val = Y * R[tuv_index(L, t, u - 1, v)];
                        if constexpr (u > 1) val += (u - 1) * R[tuv_index(L, t, u - 2, v)];
                    } else {
                        val = Z * R[tuv_index(L, t, u, v - 1)];
                        if constexpr (v > 1) val += (v - 1) * R[tuv_index(L, t, u, v - 2)];
                    }
                    R[tuv_index(L, t, u, v)] = val;
                });
            });
        });
        R[0] = F[n];
    });
}

// ---- contract ------------------------------------------------------------------------------------------------------
// One workgroup per shell pair A >= B: Lambda_tuv of its primitive pairs from the density matrix.
__global__ __launch_bounds__(PC_TS) void k_pc_lambda(int nao, const double *__restrict__ xyz, const int *__restrict__ ls,
                                                     const int *__restrict__ ao0, const int *__restrict__ pA,
                                                     const int *__restrict__ pB, const int *__restrict__ pp_begin,
                                                     const double *__restrict__ pp_ab, const double *__restrict__ pp_cc,
                                                     const long long *__restrict__ tuvoff, const double *__restrict__ D,
                                                     double *__restrict__ lam)
{
    __shared__ double s_D[7 * 7], s_half[EC_MAXC * 7], s_C[EC_MAXC * EC_MAXC], s_E[3 * EC_ED];
    const int tid = threadIdx.x, kab = blockIdx.x;
    const int A = pA[kab], B = pB[kab], la = ls[A], lb = ls[B];
    const int nsa = 2 * la + 1, nsb = 2 * lb + 1, nca = ncart(la), ncb = ncart(lb);
    // A is symmetric in (mu, nu): an off-diagonal shell pair stands for both triangles of D
    for (int e = tid; e < nsa * nsb; e += PC_TS) {
        const int i = e / nsb, j = e - i * nsb;
        const size_t gi = ao0[A] + i, gj = ao0[B] + j;
        s_D[e] = A == B ? D[gi * nao + gj] : D[gi * nao + gj] + D[gj * nao + gi];
    }
    __syncthreads();
    for (int e = tid; e < nca * nsb; e += PC_TS) { // solid harmonics -> Cartesians, first index
        const int ca = e / nsb, mb = e - ca * nsb;
        double s = 0.0;
        for (int ma = 0; ma < nsa; ++ma) s += c_sph[la][ma][ca] * s_D[ma * nsb + mb];
        s_half[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < nca * ncb; e += PC_TS) { // second index
        const int ca = e / ncb, cb = e - ca * ncb;
        double s = 0.0;
        for (int mb = 0; mb < nsb; ++mb) s += c_sph[lb][mb][cb] * s_half[ca * nsb + mb];
        s_C[e] = s;
    }
    const int L = la + lb, NT = ntuv(L);
    const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
    for (int pp = pp_begin[kab]; pp < pp_begin[kab + 1]; ++pp) {
        const double a = pp_ab[2 * pp], b = pp_ab[2 * pp + 1];
        __syncthreads(); // s_C complete; the previous primitive pair is done with s_E
        if (tid < 3) hermite_E(la, lb, a, b, RA[tid] - RB[tid], s_E + tid * EC_ED);
        __syncthreads();
        const double pref = 2.0 * M_PI / (a + b) * pp_cc[pp];
        for (int i = tid; i < NT; i += PC_TS) {
            int t = 0, r = i; // i -> (t, u, v) in the order of tuv_index
            while (r >= (L - t + 1) * (L - t + 2) / 2) { r -= (L - t + 1) * (L - t + 2) / 2; ++t; }
            int u = 0;
            while (r >= L - t - u + 1) { r -= L - t - u + 1; ++u; }
            const int v = r;
            double s = 0.0;
            for (int ca = 0; ca < nca; ++ca)
                for (int cb = 0; cb < ncb; ++cb) // E[i][j][t] is zero for t > i + j
                    s += s_C[ca * ncb + cb] * s_E[(c_cx[la][ca] * 4 + c_cx[lb][cb]) * 7 + t] *
                         s_E[EC_ED + (c_cy[la][ca] * 4 + c_cy[lb][cb]) * 7 + u] * s_E[2 * EC_ED + (c_cz[la][ca] * 4 + c_cz[lb][cb]) * 7 + v];
            lam[tuvoff[pp] + i] = pref * s;
        }
    }
}

// One point per lane; the primitive pairs of class L (list) in tiles through LDS.  `out` was cleared by the caller and
// the classes' launches follow each other on one stream: a point's value is the sum of its classes in a fixed order.
template <int L>
__global__ __launch_bounds__(PC_T) void k_pc_contract(long long npts, const double *__restrict__ pts, int npp,
                                                      const int *__restrict__ list, const double *__restrict__ geom,
                                                      const long long *__restrict__ tuvoff, const double *__restrict__ lam,
                                                      double *__restrict__ out)
{
    constexpr int NT = ntuv(L);
    __shared__ double s_lam[PC_TILE * NT], s_g[PC_TILE * 4];
    const int tid = threadIdx.x;
    const long long c = (long long)blockIdx.x * PC_T + tid;
    const bool live = c < npts;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (live) { cx = pts[3 * c]; cy = pts[3 * c + 1]; cz = pts[3 * c + 2]; }
    double acc = 0.0;
    for (int base = 0; base < npp; base += PC_TILE) {
        const int nt = min(PC_TILE, npp - base);
        __syncthreads();
        for (int e = tid; e < nt * NT; e += PC_T) {
            const int k = e / NT, i = e - k * NT;
            s_lam[e] = lam[tuvoff[list[base + k]] + i];
        }
        for (int e = tid; e < nt * 4; e += PC_T) s_g[e] = geom[4 * (size_t)list[base + (e >> 2)] + (e & 3)];
        __syncthreads();
        if (live)
            for (int k = 0; k < nt; ++k) {
                double R[NT];
                hermite_R_regs<L>(s_g[4 * k], s_g[4 * k + 1] - cx, s_g[4 * k + 2] - cy, s_g[4 * k + 3] - cz, R);
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < NT; ++i) s += s_lam[k * NT + i] * R[i];
                acc += s;
            }
    }
    if (live) out[c] += acc;
}

// ---- field ---------------------------------------------------------------------------------------------------------
// The gradient of the contraction with respect to the point, G[c][k] = d u[c] / d R_c,k.  The basis does not move with the
// point, so only R depends on it and d R_tuv(p, P - C) / d C_x = -R_{t+1,u,v}: the Lambda of k_pc_lambda unchanged against
// a table one order higher, G_x = -sum_pairs sum_tuv Lambda_tuv R_{t+1,u,v} (y: u + 1, z: v + 1).  Same shape as
// k_pc_contract<L>: one point per lane, the class's primitive pairs in tiles through LDS, the table of order L + 1 in
// registers, every index a compile-time constant.  `out` (npts, 3) was cleared by the caller.
template <int L>
__global__ __launch_bounds__(PC_T) void k_pc_field(long long npts, const double *__restrict__ pts, int npp,
                                                   const int *__restrict__ list, const double *__restrict__ geom,
                                                   const long long *__restrict__ tuvoff, const double *__restrict__ lam,
                                                   double *__restrict__ out)
{
    constexpr int NT = ntuv(L);
    __shared__ double s_lam[PC_TILE * NT], s_g[PC_TILE * 4];
    const int tid = threadIdx.x;
    const long long c = (long long)blockIdx.x * PC_T + tid;
    const bool live = c < npts;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (live) { cx = pts[3 * c]; cy = pts[3 * c + 1]; cz = pts[3 * c + 2]; }
    double gx = 0.0, gy = 0.0, gz = 0.0;
    for (int base = 0; base < npp; base += PC_TILE) {
        const int nt = min(PC_TILE, npp - base);
        __syncthreads();
        for (int e = tid; e < nt * NT; e += PC_T) {
            const int k = e / NT, i = e - k * NT;
            s_lam[e] = lam[tuvoff[list[base + k]] + i];
        }
        for (int e = tid; e < nt * 4; e += PC_T) s_g[e] = geom[4 * (size_t)list[base + (e >> 2)] + (e & 3)];
        __syncthreads();
        if (live)
            for (int k = 0; k < nt; ++k) {
                double R[ntuv(L + 1)];
                hermite_R_regs<L + 1>(s_g[4 * k], s_g[4 * k + 1] - cx, s_g[4 * k + 2] - cy, s_g[4 * k + 3] - cz, R);
                double sx = 0.0, sy = 0.0, sz = 0.0;
                static_for<0, L + 1>([&](auto t_) {
                    constexpr int t = decltype(t_)::value;
                    static_for<0, L - t + 1>([&](auto u_) {
                        constexpr int u = decltype(u_)::value;
                        static_for<0, L - t - u + 1>([&](auto v_) {
                            constexpr int v = decltype(v_)::value;
                            const double l = s_lam[k * NT + tuv_index(L, t, u, v)];
                            sx += l * R[tuv_index(L + 1, t + 1, u, v)];
                            sy += l * R[tuv_index(L + 1, t, u + 1, v)];
                            sz += l * R[tuv_index(L + 1, t, u, v + 1)];
                        });
                    });
                });
                gx -= sx; gy -= sy; gz -= sz;
            }
    }
    if (live) {
        out[3 * c] += gx;
        out[3 * c + 1] += gy;
        out[3 * c + 2] += gz;
    }
}

// ---- matrix --------------------------------------------------------------------------------------------------------
// Workgroup (x, y): primitive pair list[x] of class L, points y * 256 + lane + k * nchunk * 256.  Writes the NT sums
// of its chunk to ws[tuvoff[pp] * nchunk + y * NT ..].
template <int L>
__global__ __launch_bounds__(PC_T) void k_pc_wsum(long long npts, const double *__restrict__ pts, const double *__restrict__ w,
                                                  const int *__restrict__ list, const double *__restrict__ geom,
                                                  const long long *__restrict__ tuvoff, int nchunk, double *__restrict__ ws)
{
    constexpr int NT = ntuv(L);
    __shared__ double s_part[(PC_T / 64) * NT];
    const int tid = threadIdx.x, pp = list[blockIdx.x], chunk = blockIdx.y;
    const double p = geom[4 * (size_t)pp], Px = geom[4 * (size_t)pp + 1], Py = geom[4 * (size_t)pp + 2], Pz = geom[4 * (size_t)pp + 3];
    double acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = 0.0;
    for (long long c = (long long)chunk * PC_T + tid; c < npts; c += (long long)nchunk * PC_T) {
        double R[NT];
        hermite_R_regs<L>(p, Px - pts[3 * c], Py - pts[3 * c + 1], Pz - pts[3 * c + 2], R);
        const double wc = w[c];
#pragma unroll
        for (int i = 0; i < NT; ++i) acc[i] += wc * R[i];
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        double v = acc[i];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) s_part[wave * NT + i] = v;
    }
    __syncthreads();
    double *dst = ws + (size_t)tuvoff[pp] * nchunk + (size_t)chunk * NT;
    for (int i = tid; i < NT; i += PC_T) dst[i] = ((s_part[i] + s_part[NT + i]) + s_part[2 * NT + i]) + s_part[3 * NT + i];
}

// One workgroup per shell pair A >= B: chunks added in order, E contraction, primitive pairs summed, rotation, store.
__global__ __launch_bounds__(PC_TS) void k_pc_matrix(int nao, const double *__restrict__ xyz, const int *__restrict__ ls,
                                                     const int *__restrict__ ao0, const int *__restrict__ pA,
                                                     const int *__restrict__ pB, const int *__restrict__ pp_begin,
                                                     const double *__restrict__ pp_ab, const double *__restrict__ pp_cc,
                                                     const long long *__restrict__ tuvoff, int nchunk,
                                                     const double *__restrict__ ws, double *__restrict__ out)
{
    __shared__ double s_W[ntuv(6)], s_E[3 * EC_ED], s_cart[EC_MAXC * EC_MAXC], s_half[7 * EC_MAXC];
    const int tid = threadIdx.x, kab = blockIdx.x;
    const int A = pA[kab], B = pB[kab], la = ls[A], lb = ls[B];
    const int nsa = 2 * la + 1, nsb = 2 * lb + 1, nca = ncart(la), ncb = ncart(lb), nab = nca * ncb;
    const int L = la + lb, NT = ntuv(L);
    const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
    int x1 = 0, x2 = 0, y1 = 0, y2 = 0, z1 = 0, z2 = 0;
    if (tid < nab) { // this lane's Cartesian component pair (nab <= 100)
        const int ca = tid / ncb, cb = tid - ca * ncb;
        x1 = c_cx[la][ca]; x2 = c_cx[lb][cb]; y1 = c_cy[la][ca]; y2 = c_cy[lb][cb]; z1 = c_cz[la][ca]; z2 = c_cz[lb][cb];
    }
    double acc = 0.0;
    for (int pp = pp_begin[kab]; pp < pp_begin[kab + 1]; ++pp) {
        const double a = pp_ab[2 * pp], b = pp_ab[2 * pp + 1];
        __syncthreads(); // the previous primitive pair is done with s_W and s_E
        if (tid < 3) hermite_E(la, lb, a, b, RA[tid] - RB[tid], s_E + tid * EC_ED);
        const double *src = ws + (size_t)tuvoff[pp] * nchunk;
        for (int i = tid; i < NT; i += PC_TS) {
            double s = src[i];
            for (int ch = 1; ch < nchunk; ++ch) s += src[(size_t)ch * NT + i];
            s_W[i] = s;
        }
        __syncthreads();
        if (tid < nab) {
            double s = 0.0;
            for (int t = 0; t <= x1 + x2; ++t) {
                const double e1 = s_E[(x1 * 4 + x2) * 7 + t];
                for (int u = 0; u <= y1 + y2; ++u) {
                    const double e2 = e1 * s_E[EC_ED + (y1 * 4 + y2) * 7 + u];
                    for (int v = 0; v <= z1 + z2; ++v) s += e2 * s_E[2 * EC_ED + (z1 * 4 + z2) * 7 + v] * s_W[tuv_index(L, t, u, v)];
                }
            }
            acc += 2.0 * M_PI / (a + b) * pp_cc[pp] * s;
        }
    }
    if (tid < nab) s_cart[tid] = acc;
    __syncthreads();
    for (int e = tid; e < nsa * ncb; e += PC_TS) { // Cartesians -> solid harmonics, first index
        const int ma = e / ncb, cb = e - ma * ncb;
        double s = 0.0;
        for (int ca = 0; ca < nca; ++ca) s += c_sph[la][ma][ca] * s_cart[ca * ncb + cb];
        s_half[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < nsa * nsb; e += PC_TS) { // second index, the block and its mirror image
        const int ma = e / nsb, mb = e - ma * nsb;
        if (A == B && mb > ma) continue; // diagonal block: written from its lower triangle
        double s = 0.0;
        for (int cb = 0; cb < ncb; ++cb) s += c_sph[lb][mb][cb] * s_half[ma * ncb + cb];
        const size_t i = ao0[A] + ma, j = ao0[B] + mb;
        out[i * nao + j] = s;
        out[j * nao + i] = s;
    }
}

struct PcDev {
    int device = 0, nshell = 0, nao = 0, npairs = 0, npp = 0, nchunk_max = 1;
    long long total_tuv = 0;
    double *xyz = nullptr, *pp_ab = nullptr, *pp_cc = nullptr, *geom = nullptr, *ws = nullptr, *lam = nullptr;
    int *ls = nullptr, *ao0 = nullptr, *pA = nullptr, *pB = nullptr, *pp_begin = nullptr, *cls_list = nullptr;
    long long *tuvoff = nullptr;
    int cls_off[8] = {0};   // class L -> [cls_off[L], cls_off[L + 1]) of cls_list
    hipStream_t stream = nullptr;
    char err[256] = {0};
};

struct PcGuard { // every entry runs on the device that was current at Open
    int prev = -1;
    bool switched = false;
    explicit PcGuard(const PcDev *c)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
    }
    ~PcGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

template <class T> bool upload(T *&dst, const std::vector<T> &src)
{
    if (hipMalloc((void **)&dst, sizeof(T) * std::max<size_t>(src.size(), 1)) != hipSuccess) return false;
    return src.empty() || hipMemcpy(dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice) == hipSuccess;
}

int fail(PcDev *c, const char *what, hipError_t e)
{
    snprintf(c->err, sizeof c->err, "%s: %s", what, hipGetErrorString(e));
    return -1;
}

int check_launches(PcDev *c, const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(c, what, e);
}

} // namespace

extern "C" {

void *DFT_PointCoulombOpen(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off, const int *ao0,
                           const double *ex, const double *cf, int nao, int nprim_total)
{
    if (nshell <= 0 || nao <= 0 || !xyz || !ls || !nprim || !off || !ao0 || !ex || !cf) return nullptr;
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > 3 || nprim[s] < 0 || off[s] < 0 || off[s] + nprim[s] > nprim_total || ao0[s] < 0 || ao0[s] + 2 * ls[s] + 1 > nao) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    PcDev *c = new (std::nothrow) PcDev();
    if (!c) return nullptr;
    c->device = dev; c->nshell = nshell; c->nao = nao; c->npairs = nshell * (nshell + 1) / 2;
    std::vector<int> pA, pB, begin, cls[7];
    std::vector<double> ab, cc, geom;
    std::vector<long long> tuvoff;
    for (int A = 0; A < nshell; ++A)
        for (int B = 0; B <= A; ++B) {
            pA.push_back(A); pB.push_back(B); begin.push_back((int)cc.size());
            const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
            const double R2 = (RA[0] - RB[0]) * (RA[0] - RB[0]) + (RA[1] - RB[1]) * (RA[1] - RB[1]) + (RA[2] - RB[2]) * (RA[2] - RB[2]);
            const int L = ls[A] + ls[B];
            for (int ia = 0; ia < nprim[A]; ++ia)
                for (int ib = 0; ib < nprim[B]; ++ib) {
                    const double a = ex[off[A] + ia], b = ex[off[B] + ib], k = cf[off[A] + ia] * cf[off[B] + ib], p = a + b;
                    if (fabs(k) * exp(-a * b / p * R2) < 1e-18) continue; // as integrals.c and eri_cols.hip drop them
                    cls[L].push_back((int)cc.size());
                    ab.push_back(a); ab.push_back(b); cc.push_back(k);
                    geom.push_back(p);
                    for (int d = 0; d < 3; ++d) geom.push_back((a * RA[d] + b * RB[d]) / p);
                    tuvoff.push_back(c->total_tuv);
                    c->total_tuv += ntuv(L);
                }
        }
    begin.push_back((int)cc.size());
    c->npp = (int)cc.size();
    std::vector<int> list;
    for (int L = 0; L < 7; ++L) {
        c->cls_off[L] = (int)list.size();
        list.insert(list.end(), cls[L].begin(), cls[L].end());
    }
    c->cls_off[7] = (int)list.size();
    // chunks of points per primitive pair in the matrix call: enough workgroups for a few thousand in flight when the
    // pairs alone do not supply them, and a bounded workspace
    c->nchunk_max = std::min(PC_MAXCHUNK, std::max(1, (16384 + std::max(c->npp, 1) - 1) / std::max(c->npp, 1)));
    fill_tables();
    const std::vector<double> vxyz(xyz, xyz + 3 * (size_t)nshell);
    const std::vector<int> vls(ls, ls + nshell), vao(ao0, ao0 + nshell);
    const bool ok = upload(c->xyz, vxyz) && upload(c->ls, vls) && upload(c->ao0, vao) && upload(c->pA, pA) && upload(c->pB, pB) &&
                    upload(c->pp_begin, begin) && upload(c->pp_ab, ab) && upload(c->pp_cc, cc) && upload(c->geom, geom) &&
                    upload(c->tuvoff, tuvoff) && upload(c->cls_list, list) &&
                    hipMalloc((void **)&c->lam, sizeof(double) * std::max<size_t>((size_t)c->total_tuv, 1)) == hipSuccess &&
                    hipMalloc((void **)&c->ws, sizeof(double) * std::max<size_t>((size_t)c->total_tuv * c->nchunk_max, 1)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        DFT_PointCoulombClose(c);
        return nullptr;
    }
    return c;
}

void DFT_PointCoulombClose(void *h)
{
    PcDev *c = (PcDev *)h;
    if (!c) return;
    PcGuard g(c);
    void *bufs[] = {c->xyz, c->pp_ab, c->pp_cc, c->geom, c->ws, c->lam, c->ls, c->ao0, c->pA, c->pB, c->pp_begin, c->cls_list, c->tuvoff};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete c;
}

int DFT_PointCoulombSetStream(void *h, unsigned long long hip_stream)
{
    PcDev *c = (PcDev *)h;
    if (!c) return -1;
    c->stream = (hipStream_t)hip_stream;
    return 0;
}

const char *DFT_PointCoulombLastError(void *h) { return h ? ((PcDev *)h)->err : "null handle"; }

int DFT_PointCoulombMatrix(void *h, long long npts, unsigned long long d_points_xyz, unsigned long long d_weights, unsigned long long d_out)
{
    PcDev *c = (PcDev *)h;
    if (!c) return -1;
    c->err[0] = 0;
    if (npts < 0 || !d_out || (npts > 0 && (!d_points_xyz || !d_weights))) {
        snprintf(c->err, sizeof c->err, "DFT_PointCoulombMatrix: null pointer or negative point count");
        return -1;
    }
    PcGuard g(c);
    double *out = (double *)d_out;
    if (npts == 0) {
        const hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * (size_t)c->nao * c->nao, c->stream);
        return e == hipSuccess ? 0 : fail(c, "clearing the matrix", e);
    }
    const double *pts = (const double *)d_points_xyz, *w = (const double *)d_weights;
    const int nchunk = (int)std::min<long long>(c->nchunk_max, (npts + PC_T - 1) / PC_T);
#define PC_WSUM(LL)                                                                                                         \
    if (c->cls_off[LL + 1] > c->cls_off[LL])                                                                                \
        hipLaunchKernelGGL(k_pc_wsum<LL>, dim3((unsigned)(c->cls_off[LL + 1] - c->cls_off[LL]), (unsigned)nchunk), dim3(PC_T), 0, \
                           c->stream, npts, pts, w, c->cls_list + c->cls_off[LL], c->geom, c->tuvoff, nchunk, c->ws)
    PC_WSUM(0); PC_WSUM(1); PC_WSUM(2); PC_WSUM(3); PC_WSUM(4); PC_WSUM(5); PC_WSUM(6);
#undef PC_WSUM
    hipLaunchKernelGGL(k_pc_matrix, dim3((unsigned)c->npairs), dim3(PC_TS), 0, c->stream, c->nao, c->xyz, c->ls, c->ao0, c->pA, c->pB,
                       c->pp_begin, c->pp_ab, c->pp_cc, c->tuvoff, nchunk, c->ws, out);
    return check_launches(c, "DFT_PointCoulombMatrix launch failed");
}

int DFT_PointCoulombContract(void *h, long long npts, unsigned long long d_points_xyz, unsigned long long d_dm, unsigned long long d_out)
{
    PcDev *c = (PcDev *)h;
    if (!c) return -1;
    c->err[0] = 0;
    if (npts < 0 || (npts > 0 && (!d_points_xyz || !d_dm || !d_out))) {
        snprintf(c->err, sizeof c->err, "DFT_PointCoulombContract: null pointer or negative point count");
        return -1;
    }
    if (npts == 0) return 0;
    const long long nblk = (npts + PC_T - 1) / PC_T;
    if (nblk > INT_MAX) {
        snprintf(c->err, sizeof c->err, "DFT_PointCoulombContract: more than %lld points in one call", (long long)INT_MAX * PC_T);
        return -1;
    }
    PcGuard g(c);
    const double *pts = (const double *)d_points_xyz;
    double *out = (double *)d_out;
    hipLaunchKernelGGL(k_pc_lambda, dim3((unsigned)c->npairs), dim3(PC_TS), 0, c->stream, c->nao, c->xyz, c->ls, c->ao0, c->pA, c->pB,
                       c->pp_begin, c->pp_ab, c->pp_cc, c->tuvoff, (const double *)d_dm, c->lam);
    const hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * (size_t)npts, c->stream);
    if (e != hipSuccess) return fail(c, "clearing the output", e);
#define PC_CONTRACT(LL)                                                                                                     \
    if (c->cls_off[LL + 1] > c->cls_off[LL])                                                                                \
        hipLaunchKernelGGL(k_pc_contract<LL>, dim3((unsigned)nblk), dim3(PC_T), 0, c->stream, npts, pts,                    \
                           c->cls_off[LL + 1] - c->cls_off[LL], c->cls_list + c->cls_off[LL], c->geom, c->tuvoff, c->lam, out)
    PC_CONTRACT(0); PC_CONTRACT(1); PC_CONTRACT(2); PC_CONTRACT(3); PC_CONTRACT(4); PC_CONTRACT(5); PC_CONTRACT(6);
#undef PC_CONTRACT
    return check_launches(c, "DFT_PointCoulombContract launch failed");
}

int DFT_PointCoulombField(void *h, long long npts, unsigned long long d_points_xyz, unsigned long long d_dm, unsigned long long d_out)
{
    PcDev *c = (PcDev *)h;
    if (!c) return -1;
    c->err[0] = 0;
    if (npts < 0 || (npts > 0 && (!d_points_xyz || !d_dm || !d_out))) {
        snprintf(c->err, sizeof c->err, "DFT_PointCoulombField: null pointer or negative point count");
        return -1;
    }
    if (npts == 0) return 0;
    const long long nblk = (npts + PC_T - 1) / PC_T;
    if (nblk > INT_MAX) {
        snprintf(c->err, sizeof c->err, "DFT_PointCoulombField: more than %lld points in one call", (long long)INT_MAX * PC_T);
        return -1;
    }
    PcGuard g(c);
    const double *pts = (const double *)d_points_xyz;
    double *out = (double *)d_out;
    hipLaunchKernelGGL(k_pc_lambda, dim3((unsigned)c->npairs), dim3(PC_TS), 0, c->stream, c->nao, c->xyz, c->ls, c->ao0, c->pA, c->pB,
                       c->pp_begin, c->pp_ab, c->pp_cc, c->tuvoff, (const double *)d_dm, c->lam);
    const hipError_t e = hipMemsetAsync(out, 0, sizeof(double) * 3 * (size_t)npts, c->stream);
    if (e != hipSuccess) return fail(c, "clearing the output", e);
#define PC_FIELD(LL)                                                                                                        \
    if (c->cls_off[LL + 1] > c->cls_off[LL])                                                                                \
        hipLaunchKernelGGL(k_pc_field<LL>, dim3((unsigned)nblk), dim3(PC_T), 0, c->stream, npts, pts,                       \
                           c->cls_off[LL + 1] - c->cls_off[LL], c->cls_list + c->cls_off[LL], c->geom, c->tuvoff, c->lam, out)
    PC_FIELD(0); PC_FIELD(1); PC_FIELD(2); PC_FIELD(3); PC_FIELD(4); PC_FIELD(5); PC_FIELD(6);
#undef PC_FIELD
    return check_launches(c, "DFT_PointCoulombField launch failed");
}

} // extern "C"
