// The two-electron term of the nuclear gradient on the device: per shell A the derivative of
//     1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum D_ac D_bd (ab|cd)
// by the centre of A.  Device counterpart of integrals.c::grad_quartet / qc_grad2e: the same McMurchie-Davidson
// formulation (Boys function, Hermite E recurrence, downward R recurrence by auxiliary level as in eri_cols.hip), the
// same primitive-pair cut, every ordered bra pair (A, B) with every ket pair C >= D, derivative by A only, the density
// quartet 2 f D_ab D_cd - c_hf (D_ac D_bd [+ D_ad D_bc]) contracted as the derivative quartet is made.  s, p, d, f.
//
// One workgroup (256 threads; one wave for s and p on the bra) per (ordered bra pair, slice of the ket-pair list, chunk
// of the bra's Cartesian component pairs); launches are grouped by the bra's (la, lb), so a launch has one LDS layout (sized for the largest ket class of
// the molecule).  Per ket pair of its slice a workgroup
//   gathers the density quartet from dm (spherical), rotates the ket indices to Cartesian components in place and the
//     bra indices for its chunk:  Gc[kb][kc]                                       (a quartet that is exactly zero is skipped)
//   per ket primitive pair   E^cd, then the density folded into the ket's Hermite expansion
//                                P[kb][tau] = sum_kc Gc[kb][kc] (-1)^|tau| E_x E_y E_z      (independent of the bra primitives)
//   per bra primitive pair   E^ab of the RAISED first shell (i <= la + 1), R_tuv, then
//                                H[kb][tuv] = sum_tau P[kb][tau] R[tuv + tau]   over the box of kb's Hermite orders, one raised
//                            and the three short sums  sum_tuv pref dE_t E_u E_v H[kb][tuv]  with
//                                dE_t = 2a E[i+1][j][t] - i E[i-1][j][t]  in the differentiated direction.
// A thread owns one (component pair, direction) sum for the whole workgroup's life; at the end the workgroup adds them in
// component order and writes three doubles to part[(A, B)][slice][chunk].  A second kernel adds the partial sums of a
// shell in a fixed order: no floating-point atomics anywhere, the same call twice gives the same bits.
// DFT_Grad2eSpin (an open-shell state) is the same pass with the spin density M = D_a - D_b beside D in the exchange part of
// the gather, -c_hf (D_ac D_bd + M_ac M_bd [+ D_ad D_bc + M_ad M_bc]): the SPIN instantiations of the kernel.
// Not here: Schwarz or density screening (the host has none either, the two agree to rounding).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/dft_solver.h"
#include "md_device.hpp"   // boys, hermite_E, hermite_E_dim, c_cx / c_cy / c_cz, c_sph, fill_tables

namespace {

constexpr int G2_T = 256;
constexpr int G2_EI = 5, G2_EJ = 4, G2_ET = 8;      // E of the raised bra: i <= 4, j <= 3, t <= 7
constexpr int G2_ED = G2_EI * G2_EJ * G2_ET;
constexpr int G2_KBC = 32;                          // bra component pairs per chunk, at most
constexpr int G2_MAXCH = 4;                         // chunks of the largest bra (f f: 100 component pairs)
constexpr int G2_NTAU = 84;                         // (tau, nu, phi) with tau + nu + phi <= 6

// the Hermite orders of a ket, sorted by total order: the first (n + 1)(n + 2)(n + 3) / 6 serve a ket with lc + ld = n
__constant__ int c_tau[G2_NTAU];                    // tau | nu << 4 | phi << 8

__host__ __device__ inline int g2_ncart(int l) { return (l + 1) * (l + 2) / 2; }
__host__ __device__ inline int g2_ntau(int n) { return (n + 1) * (n + 2) * (n + 3) / 6; }

// LDS layout in doubles, by the launch's bra class and the molecule's largest ket shell
struct G2Layout {
    int rreg, gc, p, h, eab, ecd, f, red, ints, total;
};
__host__ __device__ inline G2Layout g2_layout(int la, int lb, int lmaxk, int kbc, int hbox)
{
    const int ncm = g2_ncart(lmaxk), rd = la + lb + 1 + 2 * lmaxk + 1;
    const int gq = (2 * la + 1) * (2 * lb + 1) * ncm * ncm;        // the half-rotated density quartet aliases the R tables
    G2Layout y;
    int o = 0;
    y.rreg = o; o += 2 * rd * rd * rd > gq ? 2 * rd * rd * rd : gq;
    y.gc = o; o += kbc * ncm * ncm;
    y.p = o; o += kbc * g2_ntau(2 * lmaxk);
    y.h = o; o += kbc * hbox;
    y.eab = o; o += 3 * G2_ED;
    y.ecd = o; o += 3 * EC_ED;
    y.f = o; o += 16;
    y.red = o; o += 3 * G2_KBC;
    y.ints = o; o += (G2_NTAU + ncm * ncm + G2_KBC + 1) / 2 + 1; // otau, kofs, bdim as ints
    y.total = o;
    return y;
}

struct Grad2eDev {
    int nshell = 0, nao = 0, nket = 0, nslice = 1, lmax = 0;
    double *xyz = nullptr, *ex = nullptr, *cf = nullptr, *part = nullptr;
    int *ls = nullptr, *nprim = nullptr, *off = nullptr, *ao0 = nullptr, *kC = nullptr, *kD = nullptr;
    int *cls_pairs = nullptr;        // ordered bra pairs A * nshell + B grouped by (la, lb) class
    int cls_off[17] = {0};
    size_t part_doubles = 0;
    hipStream_t stream = nullptr;
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork = nullptr, join[4] = {nullptr, nullptr, nullptr, nullptr};
    char err[256] = {0};
};

// T threads: 256, or 64 for s and p on the bra (at most 9 component pairs: a wave has the whole chunk, its barriers cost
// nothing and four times as many workgroups share a CU -- the contracted shells, whose primitive quartets are the bulk of
// the work, are of this kind).  Every sum is taken by one thread in a fixed order: the result does not depend on T.
//
// SPIN: the open-shell quartet (DFT_Grad2eSpin).  With D = D_a + D_b (`dm`) and M = D_a - D_b (`ms`) the exchange part of
// the gather is D_ac D_bd + M_ac M_bd [+ D_ad D_bc + M_ad M_bc]; everything behind the gather is the same code.  `ms` is the
// last parameter and is not read without SPIN, so the SPIN = false instantiations are instruction for instruction the
// kernels that had no such parameter (same registers, same LDS; the build's resource report shows it).
template <int T, bool SPIN>
__global__ __launch_bounds__(T) void k_grad2e(int nao, int nshell, const double *__restrict__ xyz, const int *__restrict__ ls,
                                                 const int *__restrict__ nprim, const int *__restrict__ off,
                                                 const int *__restrict__ ao0, const double *__restrict__ ex,
                                                 const double *__restrict__ cf, const double *__restrict__ dm, double c_hf,
                                                 const int *__restrict__ pairs, const int *__restrict__ kC,
                                                 const int *__restrict__ kD, int nket, int nslice, int nch, int kbc, int lmaxk,
                                                 int hbox, double *__restrict__ part, const double *__restrict__ ms)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int ch = blockIdx.x % nch, slice = (blockIdx.x / nch) % nslice, AB = pairs[blockIdx.x / (nch * nslice)];
    const int A = AB / nshell, B = AB - A * nshell;
    const int la = ls[A], lb = ls[B], nca = ncart(la), ncb = ncart(lb), nsa = 2 * la + 1, nsb = 2 * lb + 1;
    const int kb0 = ch * kbc, nk = min(kbc, nca * ncb - kb0);     // this chunk's bra component pairs
    const G2Layout y = g2_layout(la, lb, lmaxk, kbc, hbox);
    double *Rreg = lds + y.rreg, *Gq = Rreg, *Gc = lds + y.gc, *P = lds + y.p, *H = lds + y.h, *Eab = lds + y.eab, *Ecd = lds + y.ecd,
           *F = lds + y.f, *red = lds + y.red;
    int *otau = reinterpret_cast<int *>(lds + y.ints), *kofs = otau + G2_NTAU, *bdim = kofs + ncart(lmaxk) * ncart(lmaxk);

    // this thread's sum: component pair kb0 + tid / 3, direction tid % 3
    const bool own = tid < 3 * nk;
    const int okb = own ? kb0 + tid / 3 : 0, ox = tid % 3;
    const int oia = okb / ncb, oib = okb - oia * ncb;
    const int i0 = c_cx[la][oia], i1 = c_cy[la][oia], i2 = c_cz[la][oia], j0 = c_cx[lb][oib], j1 = c_cy[lb][oib], j2 = c_cz[lb][oib];
    const int ix = ox == 0 ? i0 : ox == 1 ? i1 : i2, jx = ox == 0 ? j0 : ox == 1 ? j1 : j2;
    double acc = 0.0;

    for (int k = tid; k < nk; k += T) {
        const int kb = kb0 + k, ia = kb / ncb, ib = kb - ia * ncb;
        bdim[k] = (c_cx[la][ia] + c_cx[lb][ib]) | (c_cy[la][ia] + c_cy[lb][ib]) << 4 | (c_cz[la][ia] + c_cz[lb][ib]) << 8;
    }

    const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
    const double Rab2 = (RA[0] - RB[0]) * (RA[0] - RB[0]) + (RA[1] - RB[1]) * (RA[1] - RB[1]) + (RA[2] - RB[2]) * (RA[2] - RB[2]);
    const double two_pi_52 = 34.986836655249725; // 2 pi^(5/2)
    const int npa = nprim[A], npb = nprim[B];
    const size_t n = (size_t)nao;

    for (int kcd = slice; kcd < nket; kcd += nslice) {
        const int C = kC[kcd], D = kD[kcd];
        const int lc = ls[C], ld = ls[D], ncc = ncart(lc), ncd = ncart(ld), nsc = 2 * lc + 1, nsd = 2 * ld + 1, nkc = ncc * ncd;
        const int Lcd = lc + ld, L = la + lb + 1 + Lcd, RD = L + 1, RD3 = RD * RD * RD, ntau = g2_ntau(Lcd);
        const double *RC = xyz + 3 * C, *RDc = xyz + 3 * D;
        const double Rcd2 = (RC[0] - RDc[0]) * (RC[0] - RDc[0]) + (RC[1] - RDc[1]) * (RC[1] - RDc[1]) + (RC[2] - RDc[2]) * (RC[2] - RDc[2]);

        __syncthreads(); // the previous ket pair is over: every region is free
        // the density quartet, spherical, at the strides of the ket's Cartesian block: Gq[ma][mb][cc][cd]
        const double f = C == D ? 1.0 : 2.0;
        int nz = 0;
        for (int e = tid; e < nsa * nsb * nsc * nsd; e += T) {
            const int md = e % nsd, mc = (e / nsd) % nsc, mb = (e / (nsd * nsc)) % nsb, ma = e / (nsd * nsc * nsb);
            const size_t i = ao0[A] + ma, j = ao0[B] + mb, k = ao0[C] + mc, l = ao0[D] + md;
            double v = 2.0 * f * dm[i * n + j] * dm[k * n + l];
            if (c_hf != 0.0) {
                if (SPIN)
                    v -= c_hf * (C == D ? dm[i * n + k] * dm[j * n + l] + ms[i * n + k] * ms[j * n + l]
                                        : dm[i * n + k] * dm[j * n + l] + ms[i * n + k] * ms[j * n + l] + dm[i * n + l] * dm[j * n + k] +
                                              ms[i * n + l] * ms[j * n + k]);
                else
                    v -= c_hf * (C == D ? dm[i * n + k] * dm[j * n + l] : dm[i * n + k] * dm[j * n + l] + dm[i * n + l] * dm[j * n + k]);
            }
            Gq[((ma * nsb + mb) * ncc + mc) * ncd + md] = v;
            nz |= v != 0.0;
        }
        for (int k = tid; k < nkc; k += T) { // where a ket component pair's E rows start, per direction
            const int ic = k / ncd, id = k - ic * ncd;
            kofs[k] = ((c_cx[lc][ic] * 4 + c_cx[ld][id]) * 7) | ((c_cy[lc][ic] * 4 + c_cy[ld][id]) * 7) << 7 | ((c_cz[lc][ic] * 4 + c_cz[ld][id]) * 7) << 14;
        }
        for (int k = tid; k < ntau; k += T) {
            const int t = c_tau[k];
            otau[k] = ((t & 15) * RD + ((t >> 4) & 15)) * RD + (t >> 8);
        }
        if (!__syncthreads_or(nz)) continue; // exactly zero: skipped, as on the host
        // spherical -> Cartesian components of a density (c_sph transposed), index d, then c: a thread owns the entries it rewrites
        for (int r = tid; r < nsa * nsb * nsc; r += T) {
            double *base = Gq + ((r / nsc) * ncc + r % nsc) * ncd;
            double in[7];
#pragma unroll
            for (int m = 0; m < 7; ++m) in[m] = m < nsd ? base[m] : 0.0;
            for (int c = 0; c < ncd; ++c) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) s += c_sph[ld][m][c] * in[m]; // rows past nsd are zero
                base[c] = s;
            }
        }
        __syncthreads();
        for (int r = tid; r < nsa * nsb * ncd; r += T) {
            double *base = Gq + (r / ncd) * nkc + r % ncd;
            double in[7];
#pragma unroll
            for (int m = 0; m < 7; ++m) in[m] = m < nsc ? base[m * ncd] : 0.0;
            for (int c = 0; c < ncc; ++c) {
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) s += c_sph[lc][m][c] * in[m];
                base[c * ncd] = s;
            }
        }
        __syncthreads();
        // the bra indices, for this chunk's component pairs
        for (int m = tid; m < nk * nkc; m += T) {
            const int kbl = m / nkc, kc = m - kbl * nkc, kb = kb0 + kbl, ca = kb / ncb, cb = kb - ca * ncb;
            double s = 0.0;
            for (int ma = 0; ma < nsa; ++ma) {
                const double ta = c_sph[la][ma][ca];
                if (ta == 0.0) continue;
                for (int mb = 0; mb < nsb; ++mb) s += ta * c_sph[lb][mb][cb] * Gq[(ma * nsb + mb) * nkc + kc];
            }
            Gc[m] = s;
        }
        // (the next barrier is the first one of the primitive loop: Gq is dead behind it, the R tables take its place)

        for (int pc = 0; pc < nprim[C]; ++pc)
            for (int pd = 0; pd < nprim[D]; ++pd) {
                const double ec = ex[off[C] + pc], ed = ex[off[D] + pd], ccd = cf[off[C] + pc] * cf[off[D] + pd];
                if (fabs(ccd) * exp(-ec * ed / (ec + ed) * Rcd2) < 1e-18) continue; // uniform
                const double q = ec + ed;
                const double Q[3] = {(ec * RC[0] + ed * RDc[0]) / q, (ec * RC[1] + ed * RDc[1]) / q, (ec * RC[2] + ed * RDc[2]) / q};
                __syncthreads(); // Gc complete; the previous primitive pair's P and Ecd are free
                if (tid < 3) hermite_E(lc, ld, ec, ed, RC[tid] - RDc[tid], Ecd + tid * EC_ED);
                __syncthreads();
                for (int m = tid; m < nk * ntau; m += T) {
                    const int kbl = m / ntau, ti = m - kbl * ntau, t = c_tau[ti];
                    const double *ex_ = Ecd + (t & 15), *ey_ = Ecd + EC_ED + ((t >> 4) & 15), *ez_ = Ecd + 2 * EC_ED + (t >> 8);
                    const double *g = Gc + kbl * nkc;
                    double s = 0.0;
                    for (int kc = 0; kc < nkc; ++kc) {
                        const int o = kofs[kc];
                        s += g[kc] * (ex_[o & 127] * ey_[(o >> 7) & 127] * ez_[o >> 14]);
                    }
                    P[kbl * ntau + ti] = (((t & 15) + ((t >> 4) & 15) + (t >> 8)) & 1) ? -s : s;
                }
                for (int pab = 0; pab < npa * npb; ++pab) {
                    const int pa = pab / npb, pb = pab - pa * npb;
                    const double ea = ex[off[A] + pa], eb = ex[off[B] + pb], cab = cf[off[A] + pa] * cf[off[B] + pb];
                    if (fabs(cab) * exp(-ea * eb / (ea + eb) * Rab2) < 1e-18) continue; // uniform
                    const double p = ea + eb;
                    const double Pc[3] = {(ea * RA[0] + eb * RB[0]) / p, (ea * RA[1] + eb * RB[1]) / p, (ea * RA[2] + eb * RB[2]) / p};
                    const double alpha = p * q / (p + q);
                    const double PQ[3] = {Pc[0] - Q[0], Pc[1] - Q[1], Pc[2] - Q[2]};
                    const double pref = two_pi_52 / (p * q * sqrt(p + q)) * cab * ccd;
                    __syncthreads(); // P complete; the previous contraction is over: Eab, F, H and the R tables are free
                    if (tid < 3) hermite_E_dim<G2_EI, G2_EJ, G2_ET>(la + 1, lb, ea, eb, RA[tid] - RB[tid], Eab + tid * G2_ED);
                    if (tid == (T > 64 ? 64 : 3)) { // F_n scaled to R^n_000 = (-2 alpha)^n F_n (the host's order of operations)
                        boys(L, alpha * (PQ[0] * PQ[0] + PQ[1] * PQ[1] + PQ[2] * PQ[2]), F);
                        double fs = 1.0;
                        for (int m = 0; m <= L; ++m) { F[m] *= fs; fs *= -2.0 * alpha; }
                    }
                    __syncthreads();
                    // R^n_tuv, n = L .. 0, as k_eri_cols: level n holds the orders t + u + v <= L - n and needs level n + 1 only
                    double *cur = Rreg, *nxt = Rreg + RD3;
                    if (tid == 0) cur[0] = F[L];
                    for (int lev = L - 1; lev >= 0; --lev) {
                        __syncthreads();
                        const int smax = L - lev, side = smax + 1;
                        for (int e = tid; e < side * side * side; e += T) {
                            const int t = e / (side * side), u = (e / side) % side, v = e % side;
                            const int s = t + u + v;
                            if (s > smax) continue;
                            double val;
                            if (s == 0) {
                                val = F[lev];
                            } else if (t > 0) {
                                val = PQ[0] * cur[((t - 1) * RD + u) * RD + v];
                                if (t > 1) val += (t - 1) * cur[((t - 2) * RD + u) * RD + v];
                            } else if (u > 0) {
                                val = PQ[1] * cur[(t * RD + u - 1) * RD + v];
                                if (u > 1) val += (u - 1) * cur[(t * RD + u - 2) * RD + v];
                            } else {
                                val = PQ[2] * cur[(t * RD + u) * RD + v - 1];
                                if (v > 1) val += (v - 1) * cur[(t * RD + u) * RD + v - 2];
                            }
                            nxt[(t * RD + u) * RD + v] = val;
                        }
                        double *sw = cur; cur = nxt; nxt = sw;
                    }
                    __syncthreads(); // `cur` = R^0
                    // H over the box (n0 + 2)(n1 + 2)(n2 + 2) of every component pair; at most one direction is raised
                    for (int m = tid; m < nk * hbox; m += T) {
                        const int kbl = m / hbox, bm = m - kbl * hbox, bd = bdim[kbl];
                        const int n0 = bd & 15, n1 = (bd >> 4) & 15, n2 = bd >> 8, by = n1 + 2, bz = n2 + 2;
                        if (bm >= (n0 + 2) * by * bz) continue;
                        const int t = bm / (by * bz), u = (bm / bz) % by, v = bm % bz;
                        if ((t > n0) + (u > n1) + (v > n2) > 1) continue;
                        const double *Rm = cur + (t * RD + u) * RD + v, *pk = P + kbl * ntau;
                        double s = 0.0;
                        for (int ti = 0; ti < ntau; ++ti) s += pk[ti] * Rm[otau[ti]];
                        H[m] = s;
                    }
                    __syncthreads();
                    if (own) {
                        const int n0 = i0 + j0, n1 = i1 + j1, n2 = i2 + j2, by = n1 + 2, bz = n2 + 2;
                        const double *E0 = Eab + (i0 * G2_EJ + j0) * G2_ET, *E1 = Eab + G2_ED + (i1 * G2_EJ + j1) * G2_ET,
                                     *E2 = Eab + 2 * G2_ED + (i2 * G2_EJ + j2) * G2_ET;
                        const double *Eup = Eab + ox * G2_ED + ((ix + 1) * G2_EJ + jx) * G2_ET;
                        const double *Edn = Eab + ox * G2_ED + ((ix > 0 ? ix - 1 : 0) * G2_EJ + jx) * G2_ET;
                        const double *Hk = H + (tid / 3) * hbox;
                        double s = 0.0;
                        for (int t = 0; t <= n0 + (ox == 0); ++t) {
                            const double e0 = ox == 0 ? 2.0 * ea * Eup[t] - (ix ? ix * Edn[t] : 0.0) : E0[t];
                            const double w0 = pref * e0;
                            for (int u = 0; u <= n1 + (ox == 1); ++u) {
                                const double e1 = ox == 1 ? 2.0 * ea * Eup[u] - (ix ? ix * Edn[u] : 0.0) : E1[u];
                                const double w1 = w0 * e1;
                                for (int v = 0; v <= n2 + (ox == 2); ++v) {
                                    const double e2 = ox == 2 ? 2.0 * ea * Eup[v] - (ix ? ix * Edn[v] : 0.0) : E2[v];
                                    s += w1 * e2 * Hk[(t * by + u) * bz + v];
                                }
                            }
                        }
                        acc += s;
                    }
                }
            }
    }

    // the component pairs' sums in component order, per direction
    __syncthreads();
    if (own) red[tid] = acc;
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
        for (int k = 0; k < nk; ++k) s += red[3 * k + tid];
        part[(((size_t)AB * nslice + slice) * G2_MAXCH + ch) * 3 + tid] = s;
    }
}

// out[A][x] = sum over B, slice, chunk of part, in that order (unused chunk slots hold the zeros of the clear)
__global__ void k_grad2e_sum(int nshell, int nslice, const double *__restrict__ part, double *__restrict__ out)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * nshell) return;
    const int A = idx / 3, x = idx - 3 * A;
    const size_t per = (size_t)nshell * nslice * G2_MAXCH;
    const double *p = part + (size_t)A * per * 3 + x;
    double s = 0.0;
    for (size_t k = 0; k < per; ++k) s += p[3 * k];
    out[idx] = s;
}

// the largest box (a + 2)(b + 2)(c + 2) of Hermite orders with a + b + c = lab
int box_max(int lab)
{
    int best = 0;
    for (int a = 0; a <= lab; ++a)
        for (int b = 0; b <= lab - a; ++b) best = std::max(best, (a + 2) * (b + 2) * (lab - a - b + 2));
    return best;
}

template <class T> bool upload(T *&dst, const T *src, size_t n)
{
    if (hipMalloc((void **)&dst, sizeof(T) * std::max<size_t>(n, 1)) != hipSuccess) return false;
    return hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyHostToDevice) == hipSuccess;
}

// Both entries: `d_ms` null is DFT_Grad2e (the closed-shell kernels), otherwise DFT_Grad2eSpin's kernels on the same tables,
// streams and partial sums.  `who` names the entry in the error sentences.
int grad2e_run(Grad2eDev *c, const char *who, const double *d_dm, const double *d_ms, double c_hf, double *d_out)
{
    const bool spin = d_ms != nullptr;
    if (hipMemsetAsync(c->part, 0, sizeof(double) * c->part_doubles, c->stream) != hipSuccess) {
        snprintf(c->err, sizeof c->err, "%s: clearing the partial sums failed", who);
        (void)hipGetLastError();
        return -1;
    }
    // fork: the side streams start behind the clear (and whatever the caller queued before it on the handle's stream)
    (void)hipEventRecord(c->fork, c->stream);
    for (int i = 0; i < 4; ++i) (void)hipStreamWaitEvent(c->side[i], c->fork, 0);
    int nlaunch = 0, rc = 0;
    // the heaviest classes first
    for (int cls = 15; cls >= 0 && rc == 0; --cls) {
        const int cnt = c->cls_off[cls + 1] - c->cls_off[cls];
        if (!cnt) continue;
        const int la = cls / 4, lb = cls % 4, nkb = g2_ncart(la) * g2_ncart(lb);
        const int nch = (nkb + G2_KBC - 1) / G2_KBC, kbc = (nkb + nch - 1) / nch, hbox = box_max(la + lb);
        const size_t bytes = ((size_t)g2_layout(la, lb, c->lmax, kbc, hbox).total * 8 + 15) & ~(size_t)15;
        const bool small = la <= 1 && lb <= 1;   // 3 nkb <= 27 sums: one wave
        static size_t allowed_all[2][2] = {{48 * 1024, 48 * 1024}, {48 * 1024, 48 * 1024}};   // per instantiation
        size_t *allowed = allowed_all[spin];
        auto kern = spin ? (small ? k_grad2e<64, true> : k_grad2e<G2_T, true>) : (small ? k_grad2e<64, false> : k_grad2e<G2_T, false>);
        if (bytes > allowed[small]) {
            if (hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
                snprintf(c->err, sizeof c->err, "%s: LDS request of %zu bytes refused", who, bytes);
                (void)hipGetLastError();
                rc = -1;
                break;
            }
            allowed[small] = bytes;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)cnt * c->nslice * nch), dim3(small ? 64 : G2_T), bytes, c->side[nlaunch++ & 3], c->nao, c->nshell,
                           c->xyz, c->ls, c->nprim, c->off, c->ao0, c->ex, c->cf, d_dm, c_hf, c->cls_pairs + c->cls_off[cls],
                           c->kC, c->kD, c->nket, c->nslice, nch, kbc, c->lmax, hbox, c->part, d_ms);
    }
    for (int i = 0; i < 4; ++i) { // join, also after a refusal: the handle's stream continues behind what was launched
        (void)hipEventRecord(c->join[i], c->side[i]);
        (void)hipStreamWaitEvent(c->stream, c->join[i], 0);
    }
    if (rc != 0) return -1;
    hipLaunchKernelGGL(k_grad2e_sum, dim3((3 * c->nshell + 63) / 64), dim3(64), 0, c->stream, c->nshell, c->nslice, c->part, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(c->err, sizeof c->err, "%s: launch failed: %s", who, hipGetErrorString(e));
        return -1;
    }
    return 0;
}

} // namespace

extern "C" {

void *DFT_Grad2eOpen(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off, const int *ao0,
                     const double *ex, const double *cf, int nao, int nprim_total)
{
    if (nshell <= 0 || nao <= 0 || nprim_total <= 0 || !xyz || !ls || !nprim || !off || !ao0 || !ex || !cf) return nullptr;
    int lmax = 0;
    for (int s = 0; s < nshell; ++s) {
        if (ls[s] < 0 || ls[s] > 3) return nullptr;
        if (ao0[s] < 0 || ao0[s] + 2 * ls[s] + 1 > nao || nprim[s] < 0 || off[s] < 0 || off[s] + nprim[s] > nprim_total) return nullptr;
        lmax = std::max(lmax, ls[s]);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return nullptr;
    }
    Grad2eDev *c = new (std::nothrow) Grad2eDev();
    if (!c) return nullptr;
    c->nshell = nshell; c->nao = nao; c->lmax = lmax;
    std::vector<int> grouped;
    grouped.reserve((size_t)nshell * nshell);
    for (int cls = 0; cls < 16; ++cls) {
        c->cls_off[cls] = (int)grouped.size();
        for (int k = 0; k < nshell * nshell; ++k)
            if (ls[k / nshell] * 4 + ls[k % nshell] == cls) grouped.push_back(k);
        // most primitive pairs first, as in eri_cols.hip: a workgroup's time goes with nprim(a) nprim(b)
        std::stable_sort(grouped.begin() + c->cls_off[cls], grouped.end(), [&](int x, int y) {
            return nprim[x / nshell] * nprim[x % nshell] > nprim[y / nshell] * nprim[y % nshell];
        });
    }
    c->cls_off[16] = (int)grouped.size();
    std::vector<int> kC, kD;
    for (int C = 0; C < nshell; ++C)
        for (int D = 0; D <= C; ++D) { kC.push_back(C); kD.push_back(D); }
    c->nket = (int)kC.size();
    // slices of the ket-pair list: tens of thousands of workgroups per call whatever the molecule's size, so that the
    // most contracted bra pairs (the longest workgroups) do not finish alone
    c->nslice = std::max(1, std::min(c->nket, (32768 + nshell * nshell - 1) / (nshell * nshell)));
    c->part_doubles = (size_t)nshell * nshell * c->nslice * G2_MAXCH * 3;
    int tau[G2_NTAU], nt = 0;
    for (int s = 0; s <= 6; ++s)
        for (int t = 0; t <= s; ++t)
            for (int u = 0; u <= s - t; ++u) tau[nt++] = t | u << 4 | (s - t - u) << 8;
    fill_tables();
    bool ok = hipMemcpyToSymbol(HIP_SYMBOL(c_tau), tau, sizeof tau) == hipSuccess;
    ok = ok && upload(c->xyz, xyz, 3 * (size_t)nshell) && upload(c->ex, ex, (size_t)nprim_total) && upload(c->cf, cf, (size_t)nprim_total) &&
         upload(c->ls, ls, (size_t)nshell) && upload(c->nprim, nprim, (size_t)nshell) && upload(c->off, off, (size_t)nshell) &&
         upload(c->ao0, ao0, (size_t)nshell) && upload(c->kC, kC.data(), kC.size()) && upload(c->kD, kD.data(), kD.size()) &&
         upload(c->cls_pairs, grouped.data(), grouped.size()) && hipMalloc((void **)&c->part, sizeof(double) * c->part_doubles) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&c->fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 4 && ok; ++i)
        ok = hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&c->join[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        DFT_Grad2eClose(c);
        return nullptr;
    }
    return c;
}

void DFT_Grad2eClose(void *h)
{
    Grad2eDev *c = (Grad2eDev *)h;
    if (!c) return;
    for (int i = 0; i < 4; ++i) {
        if (c->side[i]) { (void)hipStreamSynchronize(c->side[i]); (void)hipStreamDestroy(c->side[i]); }
        if (c->join[i]) (void)hipEventDestroy(c->join[i]);
    }
    if (c->fork) (void)hipEventDestroy(c->fork);
    void *bufs[] = {c->xyz, c->ex, c->cf, c->part, c->ls, c->nprim, c->off, c->ao0, c->kC, c->kD, c->cls_pairs};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    delete c;
}

int DFT_Grad2eSetStream(void *h, unsigned long long hip_stream)
{
    Grad2eDev *c = (Grad2eDev *)h;
    if (!c) return -1;
    c->stream = (hipStream_t)hip_stream;
    return 0;
}

const char *DFT_Grad2eLastError(void *h) { return h ? ((Grad2eDev *)h)->err : "null handle"; }

int DFT_Grad2e(void *h, unsigned long long d_dm, double c_hf, unsigned long long d_out)
{
    Grad2eDev *c = (Grad2eDev *)h;
    if (!c) return -1;
    c->err[0] = 0;
    if (!d_dm || !d_out) {
        snprintf(c->err, sizeof c->err, "DFT_Grad2e: null %s pointer", d_dm ? "output" : "density");
        return -1;
    }
    return grad2e_run(c, "DFT_Grad2e", (const double *)d_dm, nullptr, c_hf, (double *)d_out);
}

int DFT_Grad2eSpin(void *h, unsigned long long d_dm, unsigned long long d_ms, double c_hf, unsigned long long d_out)
{
    Grad2eDev *c = (Grad2eDev *)h;
    if (!c) return -1;
    c->err[0] = 0;
    if (!d_dm || !d_ms || !d_out) {
        snprintf(c->err, sizeof c->err, "DFT_Grad2eSpin: null %s pointer", !d_dm ? "density" : !d_ms ? "spin density" : "output");
        return -1;
    }
    return grad2e_run(c, "DFT_Grad2eSpin", (const double *)d_dm, (const double *)d_ms, c_hf, (double *)d_out);
}

} // extern "C"
