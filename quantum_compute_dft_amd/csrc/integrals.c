/*
 * Gaussian integrals for the SCF driver: overlap, kinetic, nuclear attraction, the Coulomb integrals at
 * arbitrary points (external charges, electrostatic potential) and the dense two-electron tensor over
 * contracted real-spherical shells (s, p, d, f).
 *
 * Host-side counterpart of what the reference obtains from PySCF/libcint at grid.py:61-65
 * (mol.intor('int1e_ovlp' | 'int1e_kin' | 'int1e_nuc' | 'int2e')), same conventions: real
 * spherical AOs in the shell order of basis.py, ERI in chemists' notation (ij|kl), full
 * nao^4 storage without symmetry packing (what dft.py:166 reshapes to (nao^2, nao^2)).
 *
 * Method: McMurchie-Davidson.  Primitive Cartesian Gaussians x^i y^j z^k exp(-a r^2) are
 * expanded in Hermite Gaussians (E coefficients), Coulomb-type integrals come from the Hermite
 * integrals R_tuv built on the Boys function; contraction coefficients (radial normalisation
 * included, basis.py) are applied per primitive pair and each Cartesian shell block is rotated
 * to real solid harmonics at the end.  OpenMP over shell pairs.  Plain C, no dependencies.
 */
#include <math.h>
#ifdef _OPENMP
#include <omp.h>
#endif
#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif
#include <stdlib.h>
#include <string.h>

#define LMAX 3
#define NCART(l) (((l) + 1) * ((l) + 2) / 2)
#define MAXCART 10
#define HDIM (2 * LMAX + 1)          /* t index range of one shell pair: 0..la+lb */
#define RDIM (4 * LMAX + 2)          /* t index range of R: 0..la+lb+lc+ld, and one more for a shell raised by a centre derivative */

/* ---- Cartesian component tables and real-solid-harmonic rotation ------------------------- */
static void cart_components(int l, int cx[MAXCART], int cy[MAXCART], int cz[MAXCART])
{
    int n = 0;
    for (int lx = l; lx >= 0; --lx)
        for (int ly = l - lx; ly >= 0; --ly) { cx[n] = lx; cy[n] = ly; cz[n] = l - lx - ly; ++n; }
}

/* T[m][c]: real solid harmonic m of degree l as a combination of Cartesian monomials
 * (orders: p x,y,z; d xy,yz,z2,xz,x2-y2; f m=-3..3), normalisation of ao_kernels.hpp. */
static void sph_matrix(int l, double T[7][MAXCART])
{
    memset(T, 0, sizeof(double) * 7 * MAXCART);
    if (l == 0) { T[0][0] = 0.282094791773878143; return; }
    if (l == 1) { for (int i = 0; i < 3; ++i) T[i][i] = 0.488602511902919921; return; }
    if (l == 2) { /* xx xy xz yy yz zz */
        const double c = 1.092548430592079070, d = 0.315391565252520002, e = 0.546274215296039535;
        T[0][1] = c; T[1][4] = c;
        T[2][0] = -d; T[2][3] = -d; T[2][5] = 2 * d;
        T[3][2] = c;
        T[4][0] = e; T[4][3] = -e;
        return;
    }
    /* l == 3: xxx xxy xxz xyy xyz xzz yyy yyz yzz zzz */
    const double f3 = 0.590043589926643510, f2 = 2.890611442640554055, f1 = 0.457045799464465739,
                 f0 = 0.373176332590115391, f2b = 1.445305721320277020;
    T[0][1] = 3 * f3; T[0][6] = -f3;
    T[1][4] = f2;
    T[2][8] = 4 * f1; T[2][1] = -f1; T[2][6] = -f1;
    T[3][9] = 2 * f0; T[3][2] = -3 * f0; T[3][7] = -3 * f0;
    T[4][5] = 4 * f1; T[4][0] = -f1; T[4][3] = -f1;
    T[5][2] = f2b; T[5][7] = -f2b;
    T[6][0] = f3; T[6][3] = -3 * f3;
}

/* ---- Boys function F_0..F_n(x) -------------------------------------------------------------- */
static void boys(int n, double x, double *F)
{
    if (x < 1e-13) { for (int m = 0; m <= n; ++m) F[m] = 1.0 / (2 * m + 1); return; }
    if (x > 40.0) { /* erf-type asymptote, then stable upward recursion */
        F[0] = 0.5 * sqrt(M_PI / x);
        const double ex = exp(-x);
        for (int m = 0; m < n; ++m) F[m + 1] = ((2 * m + 1) * F[m] - ex) / (2.0 * x);
        return;
    }
    /* series for the highest order, downward recursion for the rest */
    const double ex = exp(-x);
    double term = 1.0 / (2 * n + 1), sum = term;
    for (int k = 1; k < 400; ++k) {
        term *= 2.0 * x / (2 * n + 2 * k + 1);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    F[n] = ex * sum;
    for (int m = n; m > 0; --m) F[m - 1] = (2.0 * x * F[m] + ex) / (2 * m - 1);
}

/* ---- Hermite expansion coefficients E[i][j][t] for one dimension --------------------------- */
static void hermite_E(int la, int lb, double a, double b, double XAB, double E[LMAX + 3][LMAX + 3][2 * LMAX + 5])
{
    const double p = a + b, mu = a * b / p, XPA = -b / p * XAB, XPB = a / p * XAB; /* XAB = A - B */
    memset(E, 0, sizeof(double) * (LMAX + 3) * (LMAX + 3) * (2 * LMAX + 5));
    E[0][0][0] = exp(-mu * XAB * XAB);
    for (int i = 0; i <= la; ++i) {
        if (i > 0)
            for (int t = 0; t <= i; ++t) {
                double v = XPA * E[i - 1][0][t];
                if (t > 0) v += E[i - 1][0][t - 1] / (2 * p);
                v += (t + 1) * E[i - 1][0][t + 1];
                E[i][0][t] = v;
            }
        for (int j = 1; j <= lb; ++j)
            for (int t = 0; t <= i + j; ++t) {
                double v = XPB * E[i][j - 1][t];
                if (t > 0) v += E[i][j - 1][t - 1] / (2 * p);
                v += (t + 1) * E[i][j - 1][t + 1];
                E[i][j][t] = v;
            }
    }
}

/* ---- Hermite Coulomb integrals R[t][u][v] (order 0), t+u+v <= L ----------------------------- */
static void hermite_R(int L, double alpha, const double PQ[3], double R[RDIM][RDIM][RDIM])
{
    static _Thread_local double Rn[RDIM + 1][RDIM][RDIM][RDIM];
    double F[RDIM + 1];
    const double r2 = PQ[0] * PQ[0] + PQ[1] * PQ[1] + PQ[2] * PQ[2];
    boys(L, alpha * r2, F);
    double f = 1.0;
    for (int n = 0; n <= L; ++n) { Rn[n][0][0][0] = f * F[n]; f *= -2.0 * alpha; }
    for (int s = 1; s <= L; ++s)            /* total order t+u+v = s, needs auxiliary n <= L - s */
        for (int n = 0; n <= L - s; ++n)
            for (int t = 0; t <= s; ++t)
                for (int u = 0; u <= s - t; ++u) {
                    const int v = s - t - u;
                    double val;
                    if (t > 0) {
                        val = PQ[0] * Rn[n + 1][t - 1][u][v];
                        if (t > 1) val += (t - 1) * Rn[n + 1][t - 2][u][v];
                    } else if (u > 0) {
                        val = PQ[1] * Rn[n + 1][t][u - 1][v];
                        if (u > 1) val += (u - 1) * Rn[n + 1][t][u - 2][v];
                    } else {
                        val = PQ[2] * Rn[n + 1][t][u][v - 1];
                        if (v > 1) val += (v - 1) * Rn[n + 1][t][u][v - 2];
                    }
                    Rn[n][t][u][v] = val;
                }
    for (int t = 0; t <= L; ++t)
        for (int u = 0; u <= L - t; ++u)
            for (int v = 0; v <= L - t - u; ++v) R[t][u][v] = Rn[0][t][u][v];
}

/* rotate a Cartesian block (na x nb) to spherical on both indices and scatter */
static void put_sph2(int la, int lb, const double *cart, double *out, int ld, int ia, int ib)
{
    double Ta[7][MAXCART], Tb[7][MAXCART];
    sph_matrix(la, Ta);
    sph_matrix(lb, Tb);
    const int nca = NCART(la), ncb = NCART(lb);
    for (int ma = 0; ma < 2 * la + 1; ++ma)
        for (int mb = 0; mb < 2 * lb + 1; ++mb) {
            double s = 0.0;
            for (int ca = 0; ca < nca; ++ca) {
                if (Ta[ma][ca] == 0.0) continue;
                for (int cb = 0; cb < ncb; ++cb) s += Ta[ma][ca] * Tb[mb][cb] * cart[ca * ncb + cb];
            }
            out[(size_t)(ia + ma) * ld + ib + mb] = s;
        }
}

/* ---- one-electron integrals ----------------------------------------------------------------- */
int qc_int1e(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
             const int *ao0, const double *ex, const double *cf, int nao, int natm,
             const double *atm_xyz, const double *atm_z, double *S, double *T, double *V)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX) return -1;
#pragma omp parallel for schedule(dynamic) collapse(2)
    for (int A = 0; A < nshell; ++A)
        for (int B = 0; B < nshell; ++B) {
            const int la = ls[A], lb = ls[B], nca = NCART(la), ncb = NCART(lb);
            int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
            cart_components(la, ax, ay, az);
            cart_components(lb, bx, by, bz);
            double cs[MAXCART * MAXCART] = {0}, ct[MAXCART * MAXCART] = {0}, cv[MAXCART * MAXCART] = {0};
            const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
            for (int pa = 0; pa < nprim[A]; ++pa)
                for (int pb = 0; pb < nprim[B]; ++pb) {
                    const double a = ex[off[A] + pa], b = ex[off[B] + pb], p = a + b;
                    const double cc = cf[off[A] + pa] * cf[off[B] + pb];
                    double E[3][LMAX + 3][LMAX + 3][2 * LMAX + 5];
                    for (int d = 0; d < 3; ++d) hermite_E(la, lb + 2, a, b, RA[d] - RB[d], E[d]);
                    const double P[3] = {(a * RA[0] + b * RB[0]) / p, (a * RA[1] + b * RB[1]) / p,
                                         (a * RA[2] + b * RB[2]) / p};
                    const double s0 = pow(M_PI / p, 1.5);
                    for (int ca = 0; ca < nca; ++ca)
                        for (int cb = 0; cb < ncb; ++cb) {
                            const int i[3] = {ax[ca], ay[ca], az[ca]}, j[3] = {bx[cb], by[cb], bz[cb]};
                            double s1[3], k1[3];
                            for (int d = 0; d < 3; ++d) {
                                s1[d] = E[d][i[d]][j[d]][0];
                                /* -1/2 d^2/dx^2 acting on the ket */
                                double k = -2.0 * b * b * E[d][i[d]][j[d] + 2][0] + b * (2 * j[d] + 1) * s1[d];
                                if (j[d] >= 2) k -= 0.5 * j[d] * (j[d] - 1) * E[d][i[d]][j[d] - 2][0];
                                k1[d] = k;
                            }
                            cs[ca * ncb + cb] += cc * s0 * s1[0] * s1[1] * s1[2];
                            ct[ca * ncb + cb] += cc * s0 * (k1[0] * s1[1] * s1[2] + s1[0] * k1[1] * s1[2] + s1[0] * s1[1] * k1[2]);
                        }
                    /* nuclear attraction */
                    const int L = la + lb;
                    for (int c = 0; c < natm; ++c) {
                        static _Thread_local double R[RDIM][RDIM][RDIM];
                        const double PC[3] = {P[0] - atm_xyz[3 * c], P[1] - atm_xyz[3 * c + 1], P[2] - atm_xyz[3 * c + 2]};
                        hermite_R(L, p, PC, R);
                        const double pref = -atm_z[c] * 2.0 * M_PI / p * cc;
                        for (int ca = 0; ca < nca; ++ca)
                            for (int cb = 0; cb < ncb; ++cb) {
                                double v = 0.0;
                                for (int t = 0; t <= ax[ca] + bx[cb]; ++t)
                                    for (int u = 0; u <= ay[ca] + by[cb]; ++u)
                                        for (int w = 0; w <= az[ca] + bz[cb]; ++w)
                                            v += E[0][ax[ca]][bx[cb]][t] * E[1][ay[ca]][by[cb]][u] *
                                                 E[2][az[ca]][bz[cb]][w] * R[t][u][w];
                                cv[ca * ncb + cb] += pref * v;
                            }
                    }
                }
            put_sph2(la, lb, cs, S, nao, ao0[A], ao0[B]);
            put_sph2(la, lb, ct, T, nao, ao0[A], ao0[B]);
            put_sph2(la, lb, cv, V, nao, ao0[A], ao0[B]);
        }
    return 0;
}

/* ---- dipole integrals ------------------------------------------------------------------------ */
/* D[k][mu][nu] = <mu| (r - O)_k |nu>, k = x, y, z (3, nao, nao).  In the moment's dimension the one-dimensional overlap
 * E_0 sqrt(pi/p) becomes (E_1 + (P - O) E_0) sqrt(pi/p): r - O = (r - P) + (P - O), and the first moment about P of the
 * Hermite Gaussian Lambda_t is sqrt(pi/p) for t = 1 and zero otherwise. */
int qc_dipole(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
              const int *ao0, const double *ex, const double *cf, int nao, const double *origin, double *D)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX) return -1;
#pragma omp parallel for schedule(dynamic) collapse(2)
    for (int A = 0; A < nshell; ++A)
        for (int B = 0; B < nshell; ++B) {
            const int la = ls[A], lb = ls[B], nca = NCART(la), ncb = NCART(lb);
            int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
            cart_components(la, ax, ay, az);
            cart_components(lb, bx, by, bz);
            double cd[3][MAXCART * MAXCART] = {{0}};
            const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
            for (int pa = 0; pa < nprim[A]; ++pa)
                for (int pb = 0; pb < nprim[B]; ++pb) {
                    const double a = ex[off[A] + pa], b = ex[off[B] + pb], p = a + b;
                    const double cc = cf[off[A] + pa] * cf[off[B] + pb];
                    double E[3][LMAX + 3][LMAX + 3][2 * LMAX + 5];
                    double PO[3];
                    for (int d = 0; d < 3; ++d) {
                        hermite_E(la, lb, a, b, RA[d] - RB[d], E[d]);
                        PO[d] = (a * RA[d] + b * RB[d]) / p - origin[d];
                    }
                    const double s0 = pow(M_PI / p, 1.5);
                    for (int ca = 0; ca < nca; ++ca)
                        for (int cb = 0; cb < ncb; ++cb) {
                            const int i[3] = {ax[ca], ay[ca], az[ca]}, j[3] = {bx[cb], by[cb], bz[cb]};
                            double s1[3], m1[3];
                            for (int d = 0; d < 3; ++d) {
                                s1[d] = E[d][i[d]][j[d]][0];
                                m1[d] = E[d][i[d]][j[d]][1] + PO[d] * s1[d];
                            }
                            cd[0][ca * ncb + cb] += cc * s0 * m1[0] * s1[1] * s1[2];
                            cd[1][ca * ncb + cb] += cc * s0 * s1[0] * m1[1] * s1[2];
                            cd[2][ca * ncb + cb] += cc * s0 * s1[0] * s1[1] * m1[2];
                        }
                }
            for (int k = 0; k < 3; ++k) put_sph2(la, lb, cd[k], D + (size_t)k * nao * nao, nao, ao0[A], ao0[B]);
        }
    return 0;
}

/* ---- one-electron Coulomb integrals at arbitrary points -------------------------------------- */
/* A[c][mu][nu] = <mu| 1/|r - R_c| |nu> (the nuclear-attraction integral of qc_int1e for a unit charge at any point,
 * positive sign), never stored: qc_point_matrix sums it over points with weights, qc_point_contract contracts it with
 * a matrix.  Host counterparts of csrc/point_coulomb.hip.  Shell pairs A >= B; primitive pairs whose Gaussian-product
 * prefactor is below 1e-18 are dropped as in ctx_build_pairs. */
static int prim_pair_kept(double a, double b, double cc, double R2) { return !(fabs(cc) * exp(-a * b / (a + b) * R2) < 1e-18); }

static double dist2(const double *RA, const double *RB)
{
    return (RA[0] - RB[0]) * (RA[0] - RB[0]) + (RA[1] - RB[1]) * (RA[1] - RB[1]) + (RA[2] - RB[2]) * (RA[2] - RB[2]);
}

/* M[mu][nu] = sum_c w[c] A[c][mu][nu]: (nao, nao), both triangles written, M == M^T bit for bit.
 * field != 0: M (3, nao, nao), M[k] = sum_c w[c] dA[c] / dR_c,k -- the sums W_tuv of -R_{t+1,u,v}, -R_{t,u+1,v}, -R_{t,u,v+1}
 * from a table one order higher (see point_contract), everything else the same. */
static int point_matrix(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                        const int *ao0, const double *ex, const double *cf, int nao, long long npts,
                        const double *pts, const double *w, int field, double *M)
{
    const int ncomp = field ? 3 : 1;
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX) return -1;
    const int npairs = nshell * (nshell + 1) / 2;
#pragma omp parallel for schedule(dynamic)
    for (int k = 0; k < npairs; ++k) {
        int A = (int)((sqrt(8.0 * k + 1.0) - 1.0) / 2.0);
        while (A * (A + 1) / 2 > k) --A;
        while ((A + 1) * (A + 2) / 2 <= k) ++A;
        const int B = k - A * (A + 1) / 2;
        const int la = ls[A], lb = ls[B], nca = NCART(la), ncb = NCART(lb), L = la + lb;
        int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
        cart_components(la, ax, ay, az);
        cart_components(lb, bx, by, bz);
        double cart[3][MAXCART * MAXCART] = {{0}};
        const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
        const double R2 = dist2(RA, RB);
        for (int pa = 0; pa < nprim[A]; ++pa)
            for (int pb = 0; pb < nprim[B]; ++pb) {
                const double a = ex[off[A] + pa], b = ex[off[B] + pb], p = a + b;
                const double cc = cf[off[A] + pa] * cf[off[B] + pb];
                if (!prim_pair_kept(a, b, cc, R2)) continue;
                double E[3][LMAX + 3][LMAX + 3][2 * LMAX + 5];
                for (int d = 0; d < 3; ++d) hermite_E(la, lb, a, b, RA[d] - RB[d], E[d]);
                const double P[3] = {(a * RA[0] + b * RB[0]) / p, (a * RA[1] + b * RB[1]) / p, (a * RA[2] + b * RB[2]) / p};
                double W[3][HDIM][HDIM][HDIM] = {{{{0}}}};
                for (long long c = 0; c < npts; ++c) {
                    static _Thread_local double R[RDIM][RDIM][RDIM];
                    const double PC[3] = {P[0] - pts[3 * c], P[1] - pts[3 * c + 1], P[2] - pts[3 * c + 2]};
                    hermite_R(L + (field != 0), p, PC, R);
                    for (int t = 0; t <= L; ++t)
                        for (int u = 0; u <= L - t; ++u)
                            for (int v = 0; v <= L - t - u; ++v) {
                                if (!field) { W[0][t][u][v] += w[c] * R[t][u][v]; continue; }
                                W[0][t][u][v] -= w[c] * R[t + 1][u][v];
                                W[1][t][u][v] -= w[c] * R[t][u + 1][v];
                                W[2][t][u][v] -= w[c] * R[t][u][v + 1];
                            }
                }
                const double pref = 2.0 * M_PI / p * cc;
                for (int k = 0; k < ncomp; ++k)
                    for (int ca = 0; ca < nca; ++ca)
                        for (int cb = 0; cb < ncb; ++cb) {
                            double v = 0.0;
                            for (int t = 0; t <= ax[ca] + bx[cb]; ++t)
                                for (int u = 0; u <= ay[ca] + by[cb]; ++u)
                                    for (int q = 0; q <= az[ca] + bz[cb]; ++q)
                                        v += E[0][ax[ca]][bx[cb]][t] * E[1][ay[ca]][by[cb]][u] * E[2][az[ca]][bz[cb]][q] * W[k][t][u][q];
                            cart[k][ca * ncb + cb] += pref * v;
                        }
            }
        for (int k = 0; k < ncomp; ++k) {
            double blk[7 * 7];
            double *Mk = M + (size_t)k * nao * nao;
            put_sph2(la, lb, cart[k], blk, 7, 0, 0);
            for (int ma = 0; ma < 2 * la + 1; ++ma)
                for (int mb = 0; mb < (A == B ? ma + 1 : 2 * lb + 1); ++mb) { /* a diagonal block from its lower triangle */
                    const size_t i = ao0[A] + ma, j = ao0[B] + mb;
                    Mk[i * nao + j] = blk[ma * 7 + mb];
                    Mk[j * nao + i] = blk[ma * 7 + mb];
                }
        }
    }
    return 0;
}

int qc_point_matrix(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                    const int *ao0, const double *ex, const double *cf, int nao, long long npts,
                    const double *pts, const double *w, double *M)
{
    return point_matrix(nshell, xyz, ls, nprim, off, ao0, ex, cf, nao, npts, pts, w, 0, M);
}

/* M (3, nao, nao), M[k][mu][nu] = sum_c w[c] dA[c][mu][nu] / dR_c,k: the derivative integrals themselves (one point of unit
 * weight: dA[c]), host only -- what the contraction of qc_point_field and the device kernel are checked against. */
int qc_point_field_matrix(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                          const int *ao0, const double *ex, const double *cf, int nao, long long npts,
                          const double *pts, const double *w, double *M)
{
    return point_matrix(nshell, xyz, ls, nprim, off, ao0, ex, cf, nao, npts, pts, w, 1, M);
}

/* u[c] = sum_{mu nu} D[mu][nu] A[c][mu][nu] for any (nao, nao) matrix D.  Two steps: the Hermite densities Lambda_tuv of
 * every kept primitive pair from D[A,B] + D[B,A]^T (OpenMP over shell pairs), then u[c] = sum_pairs sum_tuv Lambda_tuv
 * R_tuv(p, P - R_c) (OpenMP over points: every point adds its pairs in the same order).
 * field != 0: the gradient of u with respect to the point instead, out (npts, 3).  The basis does not move with the point,
 * so only R depends on it: d R_tuv(p, P - C) / d C_x = -R_{t+1,u,v}, the same Lambda against a table one order higher,
 * G[c][x] = -sum_pairs sum_tuv Lambda_tuv R_{t+1,u,v} (y: u + 1, z: v + 1). */
static int point_contract(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                          const int *ao0, const double *ex, const double *cf, int nao, long long npts,
                          const double *pts, const double *D, int field, double *out)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX) return -1;
    const int npairs = nshell * (nshell + 1) / 2;
    int *pbeg = (int *)malloc(sizeof(int) * (npairs + 1));
    int npp = 0;
    for (int A = 0, k = 0; A < nshell; ++A)
        for (int B = 0; B <= A; ++B, ++k) {
            pbeg[k] = npp;
            const double R2 = dist2(xyz + 3 * A, xyz + 3 * B);
            for (int pa = 0; pa < nprim[A]; ++pa)
                for (int pb = 0; pb < nprim[B]; ++pb)
                    npp += prim_pair_kept(ex[off[A] + pa], ex[off[B] + pb], cf[off[A] + pa] * cf[off[B] + pb], R2);
        }
    pbeg[npairs] = npp;
    const int NT = HDIM * (HDIM + 1) * (HDIM + 2) / 6; /* 84 entries t + u + v <= 6, in the order t, u, v */
    double *geom = (double *)malloc(sizeof(double) * 4 * (npp + 1));
    int *Ls = (int *)malloc(sizeof(int) * (npp + 1));
    double *lam = (double *)calloc((size_t)NT * (npp + 1), sizeof(double));
#pragma omp parallel for schedule(dynamic)
    for (int A = 0; A < nshell; ++A)
        for (int B = 0; B <= A; ++B) {
            const int k = A * (A + 1) / 2 + B;
            const int la = ls[A], lb = ls[B], nca = NCART(la), ncb = NCART(lb), nsa = 2 * la + 1, nsb = 2 * lb + 1, L = la + lb;
            int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
            cart_components(la, ax, ay, az);
            cart_components(lb, bx, by, bz);
            double Ta[7][MAXCART], Tb[7][MAXCART], Dc[MAXCART * MAXCART] = {0};
            sph_matrix(la, Ta);
            sph_matrix(lb, Tb);
            for (int ma = 0; ma < nsa; ++ma)
                for (int mb = 0; mb < nsb; ++mb) { /* A is symmetric: an off-diagonal shell pair stands for both triangles of D */
                    const size_t i = ao0[A] + ma, j = ao0[B] + mb;
                    const double d = A == B ? D[i * nao + j] : D[i * nao + j] + D[j * nao + i];
                    for (int ca = 0; ca < nca; ++ca)
                        for (int cb = 0; cb < ncb; ++cb) Dc[ca * ncb + cb] += Ta[ma][ca] * Tb[mb][cb] * d;
                }
            const double *RA = xyz + 3 * A, *RB = xyz + 3 * B;
            const double R2 = dist2(RA, RB);
            int pp = pbeg[k];
            for (int pa = 0; pa < nprim[A]; ++pa)
                for (int pb = 0; pb < nprim[B]; ++pb) {
                    const double a = ex[off[A] + pa], b = ex[off[B] + pb], p = a + b;
                    const double cc = cf[off[A] + pa] * cf[off[B] + pb];
                    if (!prim_pair_kept(a, b, cc, R2)) continue;
                    double E[3][LMAX + 3][LMAX + 3][2 * LMAX + 5];
                    for (int d = 0; d < 3; ++d) hermite_E(la, lb, a, b, RA[d] - RB[d], E[d]);
                    geom[4 * pp] = p;
                    for (int d = 0; d < 3; ++d) geom[4 * pp + 1 + d] = (a * RA[d] + b * RB[d]) / p;
                    Ls[pp] = L;
                    const double pref = 2.0 * M_PI / p * cc;
                    double *lm = lam + (size_t)NT * pp;
                    int n = 0;
                    for (int t = 0; t <= L; ++t)
                        for (int u = 0; u <= L - t; ++u)
                            for (int v = 0; v <= L - t - u; ++v, ++n) {
                                double s = 0.0;
                                for (int ca = 0; ca < nca; ++ca)
                                    for (int cb = 0; cb < ncb; ++cb)
                                        if (t <= ax[ca] + bx[cb] && u <= ay[ca] + by[cb] && v <= az[ca] + bz[cb])
                                            s += Dc[ca * ncb + cb] * E[0][ax[ca]][bx[cb]][t] * E[1][ay[ca]][by[cb]][u] * E[2][az[ca]][bz[cb]][v];
                                lm[n] = pref * s;
                            }
                    ++pp;
                }
        }
#pragma omp parallel for schedule(static)
    for (long long c = 0; c < npts; ++c) {
        static _Thread_local double R[RDIM][RDIM][RDIM];
        double acc = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
        for (int pp = 0; pp < npp; ++pp) {
            const double PC[3] = {geom[4 * pp + 1] - pts[3 * c], geom[4 * pp + 2] - pts[3 * c + 1], geom[4 * pp + 3] - pts[3 * c + 2]};
            const int L = Ls[pp];
            hermite_R(L + (field != 0), geom[4 * pp], PC, R);
            const double *lm = lam + (size_t)NT * pp;
            int n = 0;
            if (field) {
                double sx = 0.0, sy = 0.0, sz = 0.0;
                for (int t = 0; t <= L; ++t)
                    for (int u = 0; u <= L - t; ++u)
                        for (int v = 0; v <= L - t - u; ++v, ++n) {
                            sx += lm[n] * R[t + 1][u][v];
                            sy += lm[n] * R[t][u + 1][v];
                            sz += lm[n] * R[t][u][v + 1];
                        }
                gx -= sx; gy -= sy; gz -= sz;
                continue;
            }
            double s = 0.0;
            for (int t = 0; t <= L; ++t)
                for (int u = 0; u <= L - t; ++u)
                    for (int v = 0; v <= L - t - u; ++v, ++n) s += lm[n] * R[t][u][v];
            acc += s;
        }
        if (field) { out[3 * c] = gx; out[3 * c + 1] = gy; out[3 * c + 2] = gz; }
        else out[c] = acc;
    }
    free(pbeg); free(geom); free(Ls); free(lam);
    return 0;
}

int qc_point_contract(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                      const int *ao0, const double *ex, const double *cf, int nao, long long npts,
                      const double *pts, const double *D, double *out)
{
    return point_contract(nshell, xyz, ls, nprim, off, ao0, ex, cf, nao, npts, pts, D, 0, out);
}

/* G[c][k] = sum_{mu nu} D[mu][nu] dA[c][mu][nu] / dR_c,k, k = x, y, z: out (npts, 3).  For a density matrix the electronic
 * part of the electric field at the point (the electronic potential is -u). */
int qc_point_field(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                   const int *ao0, const double *ex, const double *cf, int nao, long long npts,
                   const double *pts, const double *D, double *out)
{
    return point_contract(nshell, xyz, ls, nprim, off, ao0, ex, cf, nao, npts, pts, D, 1, out);
}

/* ---- two-electron integrals ------------------------------------------------------------------ */
typedef struct {
    double p, P[3], cc;
    double E[3][LMAX + 1][LMAX + 1][HDIM]; /* E[d][i][j][t] */
} PrimPair;

static void make_pair(int la, int lb, double a, double b, const double *RA, const double *RB, double cc, PrimPair *pp)
{
    double E[LMAX + 3][LMAX + 3][2 * LMAX + 5];
    pp->p = a + b;
    pp->cc = cc;
    for (int d = 0; d < 3; ++d) {
        pp->P[d] = (a * RA[d] + b * RB[d]) / pp->p;
        hermite_E(la, lb, a, b, RA[d] - RB[d], E);
        for (int i = 0; i <= la; ++i)
            for (int j = 0; j <= lb; ++j)
                for (int t = 0; t <= i + j; ++t) pp->E[d][i][j][t] = E[i][j][t];
    }
}

/* rotate one index of a 4-index Cartesian block to spherical: in (n0, nc, n2) -> out (n0, ns, n2) */
static void rot_axis(int l, int n0, int n2, const double *in, double *out)
{
    if (l <= 1) { /* s and p: the transformation is a scale (sph_matrix: T = c * identity), most shells are these */
        const double c = l == 0 ? 0.282094791773878143 : 0.488602511902919921;
        const size_t n = (size_t)n0 * (l == 0 ? 1 : 3) * n2;
        for (size_t i = 0; i < n; ++i) out[i] = c * in[i];
        return;
    }
    double T[7][MAXCART];
    sph_matrix(l, T);
    const int nc = NCART(l), ns = 2 * l + 1;
    for (int i0 = 0; i0 < n0; ++i0)
        for (int m = 0; m < ns; ++m)
            for (int i2 = 0; i2 < n2; ++i2) {
                double s = 0.0;
                for (int c = 0; c < nc; ++c)
                    if (T[m][c] != 0.0) s += T[m][c] * in[((size_t)i0 * nc + c) * n2 + i2];
                out[((size_t)i0 * ns + m) * n2 + i2] = s;
            }
}

/* Every shell pair A >= B with its primitive-pair data; shared by the dense and the column-wise
 * (Cholesky) drivers. */
typedef struct {
    int nshell, nao, npairs;
    const double *xyz, *ex, *cf;
    const int *ls, *nprim, *off, *ao0;
    int *pA, *pB;
    PrimPair **pairs;
    int *npp;     /* significant primitive pairs kept per shell pair */
    double *qmax; /* Schwarz bound sqrt(max (ab|ab)) per shell pair, filled by qc_eri_diag */
    /* owned copies of the shell table (the context outlives the caller's arrays) */
    double *own_xyz, *own_ex, *own_cf;
    int *own_i;
} EriCtx;

static int pair_index(int A, int B) { return A >= B ? A * (A + 1) / 2 + B : B * (B + 1) / 2 + A; }

static void ctx_build_pairs(EriCtx *c)
{
    const int nshell = c->nshell;
    c->npairs = nshell * (nshell + 1) / 2;
    c->pairs = (PrimPair **)calloc(c->npairs, sizeof(PrimPair *));
    c->npp = (int *)calloc(c->npairs, sizeof(int));
    c->pA = (int *)malloc(sizeof(int) * c->npairs);
    c->pB = (int *)malloc(sizeof(int) * c->npairs);
    c->qmax = NULL;
    for (int A = 0, k = 0; A < nshell; ++A)
        for (int B = 0; B <= A; ++B, ++k) { c->pA[k] = A; c->pB[k] = B; }
#pragma omp parallel for schedule(dynamic)
    for (int k = 0; k < c->npairs; ++k) {
        const int A = c->pA[k], B = c->pB[k];
        c->pairs[k] = (PrimPair *)malloc(sizeof(PrimPair) * c->nprim[A] * c->nprim[B]);
        /* primitive pairs whose Gaussian-product prefactor |c_a c_b| exp(-mu R_AB^2) is below 1e-18 are
         * dropped here once: tight primitives on different centres make up most of a contracted pair's
         * nprim[A]*nprim[B] products and contribute nothing at fp64 */
        const double *RA = c->xyz + 3 * A, *RB = c->xyz + 3 * B;
        const double R2 = (RA[0] - RB[0]) * (RA[0] - RB[0]) + (RA[1] - RB[1]) * (RA[1] - RB[1]) + (RA[2] - RB[2]) * (RA[2] - RB[2]);
        int kept = 0;
        for (int a = 0; a < c->nprim[A]; ++a)
            for (int b = 0; b < c->nprim[B]; ++b) {
                const double ea = c->ex[c->off[A] + a], eb = c->ex[c->off[B] + b];
                const double cc = c->cf[c->off[A] + a] * c->cf[c->off[B] + b];
                if (fabs(cc) * exp(-ea * eb / (ea + eb) * R2) < 1e-18) continue;
                make_pair(c->ls[A], c->ls[B], ea, eb, RA, RB, cc, &c->pairs[k][kept++]);
            }
        c->npp[k] = kept;
    }
}

static void ctx_free_pairs(EriCtx *c)
{
    for (int k = 0; k < c->npairs; ++k) free(c->pairs[k]);
    free(c->pairs); free(c->pA); free(c->pB); free(c->qmax); free(c->npp);
}

#define QUARTET_DOUBLES (MAXCART * MAXCART * MAXCART * MAXCART)

/* (AB|CD) for shell pairs kab = (A >= B), kcd = (C >= D): spherical block [nsa][nsb][nsc][nsd] left
 * in `cart` (t1 is scratch of the same size). */
static void quartet(const EriCtx *c, int kab, int kcd, double *cart, double *t1, double R[RDIM][RDIM][RDIM])
{
    const int A = c->pA[kab], B = c->pB[kab], C = c->pA[kcd], D = c->pB[kcd];
    const int *ls = c->ls;
    const int la = ls[A], lb = ls[B], lc = ls[C], ld = ls[D];
    const int nca = NCART(la), ncb = NCART(lb), ncc = NCART(lc), ncd = NCART(ld);
    int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
    int cx[MAXCART], cy[MAXCART], cz[MAXCART], dx[MAXCART], dy[MAXCART], dz[MAXCART];
    cart_components(la, ax, ay, az); cart_components(lb, bx, by, bz);
    cart_components(lc, cx, cy, cz); cart_components(ld, dx, dy, dz);
    const int Lab = la + lb, Lcd = lc + ld, L = Lab + Lcd;
    (void)Lcd;
    memset(cart, 0, sizeof(double) * nca * ncb * ncc * ncd);
    const int nab = c->npp[kab], ncdp = c->npp[kcd];
    const double two_pi_52 = 34.986836655249725; /* 2 pi^(5/2) */
    /* Sparse Hermite lists.  A component pair's expansion E^x_t E^y_u E^z_v has at most (2+1)^3 = 27 terms
     * (l <= 3 per shell); forming the products once per primitive pair -- the ket side outside the loop over the bra
     * primitives, the bra side once per primitive quartet -- leaves the two contractions below as plain sums of
     * products (the straightforward form multiplied the three factors again for every (t,u,v) and every component
     * of the other side: 77 % of the engine's time under gprof; 1.45x faster on one thread this way). */
    enum { MAXE = 27 };
    static _Thread_local double wk[MAXCART * MAXCART][MAXE], wb[MAXCART * MAXCART][MAXE];
    static _Thread_local int ok_[MAXCART * MAXCART][MAXE], ob[MAXCART * MAXCART][MAXE], nk[MAXCART * MAXCART], nb[MAXCART * MAXCART];
    static _Thread_local double g[RDIM * RDIM * RDIM];
    const double *Rf = &R[0][0][0];
    /* bra-side (t,u,v) set: every t+u+v <= Lab, as flat offsets into R / g */
    int tuv[HDIM * HDIM * HDIM], ntuv = 0;
    for (int t = 0; t <= Lab; ++t)
        for (int u = 0; u <= Lab - t; ++u)
            for (int v = 0; v <= Lab - t - u; ++v) tuv[ntuv++] = (t * RDIM + u) * RDIM + v;
    for (int icd = 0; icd < ncdp; ++icd) {
        const PrimPair *cd = &c->pairs[kcd][icd];
        for (int ic = 0; ic < ncc; ++ic)
            for (int id = 0; id < ncd; ++id) {
                const int k = ic * ncd + id;
                int n = 0;
                for (int a1 = 0; a1 <= cx[ic] + dx[id]; ++a1) {
                    const double e1 = cd->E[0][cx[ic]][dx[id]][a1];
                    for (int a2 = 0; a2 <= cy[ic] + dy[id]; ++a2) {
                        const double e2 = e1 * cd->E[1][cy[ic]][dy[id]][a2];
                        for (int a3 = 0; a3 <= cz[ic] + dz[id]; ++a3) {
                            const double e3 = e2 * cd->E[2][cz[ic]][dz[id]][a3];
                            wk[k][n] = ((a1 + a2 + a3) & 1) ? -e3 : e3;
                            ok_[k][n] = (a1 * RDIM + a2) * RDIM + a3;
                            ++n;
                        }
                    }
                }
                nk[k] = n;
            }
        for (int iab = 0; iab < nab; ++iab) {
            const PrimPair *ab = &c->pairs[kab][iab];
            const double p = ab->p, q = cd->p, alpha = p * q / (p + q);
            const double PQ[3] = {ab->P[0] - cd->P[0], ab->P[1] - cd->P[1], ab->P[2] - cd->P[2]};
            hermite_R(L, alpha, PQ, R);
            const double pref = two_pi_52 / (p * q * sqrt(p + q)) * ab->cc * cd->cc;
            for (int ia = 0; ia < nca; ++ia)
                for (int ib = 0; ib < ncb; ++ib) {
                    const int k = ia * ncb + ib;
                    int n = 0;
                    for (int t = 0; t <= ax[ia] + bx[ib]; ++t) {
                        const double e1 = pref * ab->E[0][ax[ia]][bx[ib]][t];
                        for (int u = 0; u <= ay[ia] + by[ib]; ++u) {
                            const double e2 = e1 * ab->E[1][ay[ia]][by[ib]][u];
                            for (int v = 0; v <= az[ia] + bz[ib]; ++v) {
                                wb[k][n] = e2 * ab->E[2][az[ia]][bz[ib]][v];
                                ob[k][n] = (t * RDIM + u) * RDIM + v;
                                ++n;
                            }
                        }
                    }
                    nb[k] = n;
                }
            for (int kc = 0; kc < ncc * ncd; ++kc) {
                /* g[t][u][v] = sum_{tau,nu,phi} (-1)^(tau+nu+phi) E^cd R[t+tau][u+nu][v+phi] for this ket component */
                const int ne = nk[kc];
                for (int m = 0; m < ntuv; ++m) {
                    const double *Rm = Rf + tuv[m];
                    double sacc = 0.0;
                    for (int e = 0; e < ne; ++e) sacc += wk[kc][e] * Rm[ok_[kc][e]];
                    g[tuv[m]] = sacc;
                }
                const int ic = kc / ncd, id = kc - ic * ncd;
                for (int kb = 0; kb < nca * ncb; ++kb) {
                    double sacc = 0.0;
                    for (int e = 0; e < nb[kb]; ++e) sacc += wb[kb][e] * g[ob[kb][e]];
                    cart[((size_t)kb * ncc + ic) * ncd + id] += sacc;
                }
            }
        }
    }
    /* Cartesian -> spherical on the four indices */
    const int nsa = 2 * la + 1, nsb = 2 * lb + 1, nsc = 2 * lc + 1;
    rot_axis(la, 1, ncb * ncc * ncd, cart, t1);
    rot_axis(lb, nsa, ncc * ncd, t1, cart);
    rot_axis(lc, nsa * nsb, ncd, cart, t1);
    rot_axis(ld, nsa * nsb * nsc, 1, t1, cart);
}

int qc_int2e(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
             const int *ao0, const double *ex, const double *cf, int nao, double *eri)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX) return -1;
    const size_t n = (size_t)nao;
    EriCtx ctx = {nshell, nao, 0, xyz, ex, cf, ls, nprim, off, ao0};
    ctx_build_pairs(&ctx);
#pragma omp parallel
    {
        double *cart = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        double *t1 = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        static _Thread_local double R[RDIM][RDIM][RDIM];
#pragma omp for schedule(dynamic)
        for (int kab = 0; kab < ctx.npairs; ++kab)
            for (int kcd = 0; kcd <= kab; ++kcd) {
                const int A = ctx.pA[kab], B = ctx.pB[kab], C = ctx.pA[kcd], D = ctx.pB[kcd];
                const int nsa = 2 * ls[A] + 1, nsb = 2 * ls[B] + 1, nsc = 2 * ls[C] + 1, nsd = 2 * ls[D] + 1;
                quartet(&ctx, kab, kcd, cart, t1, R);
                /* scatter with the 8-fold permutational symmetry */
                for (int a = 0; a < nsa; ++a)
                    for (int b = 0; b < nsb; ++b)
                        for (int c = 0; c < nsc; ++c)
                            for (int d = 0; d < nsd; ++d) {
                                const double v = cart[(((size_t)a * nsb + b) * nsc + c) * nsd + d];
                                const size_t i = ao0[A] + a, j = ao0[B] + b, k = ao0[C] + c, l = ao0[D] + d;
                                eri[((i * n + j) * n + k) * n + l] = v;
                                eri[((j * n + i) * n + k) * n + l] = v;
                                eri[((i * n + j) * n + l) * n + k] = v;
                                eri[((j * n + i) * n + l) * n + k] = v;
                                eri[((k * n + l) * n + i) * n + j] = v;
                                eri[((l * n + k) * n + i) * n + j] = v;
                                eri[((k * n + l) * n + j) * n + i] = v;
                                eri[((l * n + k) * n + j) * n + i] = v;
                            }
            }
        free(cart);
        free(t1);
    }
    ctx_free_pairs(&ctx);
    return 0;
}

/* ---- column-wise access for the pivoted Cholesky factorisation (no dense ERI) ------------------- */
void *qc_eri_open(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                  const int *ao0, const double *ex, const double *cf, int nao, int nprim_total)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX) return NULL;
    EriCtx *c = (EriCtx *)calloc(1, sizeof(EriCtx));
    c->nshell = nshell; c->nao = nao;
    c->own_xyz = (double *)malloc(sizeof(double) * 3 * nshell);
    c->own_ex = (double *)malloc(sizeof(double) * nprim_total);
    c->own_cf = (double *)malloc(sizeof(double) * nprim_total);
    c->own_i = (int *)malloc(sizeof(int) * 4 * nshell);
    memcpy(c->own_xyz, xyz, sizeof(double) * 3 * nshell);
    memcpy(c->own_ex, ex, sizeof(double) * nprim_total);
    memcpy(c->own_cf, cf, sizeof(double) * nprim_total);
    memcpy(c->own_i, ls, sizeof(int) * nshell);
    memcpy(c->own_i + nshell, nprim, sizeof(int) * nshell);
    memcpy(c->own_i + 2 * nshell, off, sizeof(int) * nshell);
    memcpy(c->own_i + 3 * nshell, ao0, sizeof(int) * nshell);
    c->xyz = c->own_xyz; c->ex = c->own_ex; c->cf = c->own_cf;
    c->ls = c->own_i; c->nprim = c->own_i + nshell; c->off = c->own_i + 2 * nshell; c->ao0 = c->own_i + 3 * nshell;
    ctx_build_pairs(c);
    return c;
}

void qc_eri_close(void *h)
{
    EriCtx *c = (EriCtx *)h;
    if (!c) return;
    ctx_free_pairs(c);
    free(c->own_xyz); free(c->own_ex); free(c->own_cf); free(c->own_i);
    free(c);
}

/* diag[i*nao + j] = (ij|ij); also records the Schwarz bounds used to skip quartets in qc_eri_cols */
int qc_eri_diag(void *h, double *diag)
{
    EriCtx *c = (EriCtx *)h;
    if (!c) return -1;
    const size_t n = (size_t)c->nao;
    if (!c->qmax) c->qmax = (double *)malloc(sizeof(double) * c->npairs);
#pragma omp parallel
    {
        double *cart = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        double *t1 = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        static _Thread_local double R[RDIM][RDIM][RDIM];
#pragma omp for schedule(dynamic)
        for (int kab = 0; kab < c->npairs; ++kab) {
            const int A = c->pA[kab], B = c->pB[kab];
            const int nsa = 2 * c->ls[A] + 1, nsb = 2 * c->ls[B] + 1;
            quartet(c, kab, kab, cart, t1, R);
            double m = 0.0;
            for (int a = 0; a < nsa; ++a)
                for (int b = 0; b < nsb; ++b) {
                    const double v = cart[(((size_t)a * nsb + b) * nsa + a) * nsb + b];
                    const size_t i = c->ao0[A] + a, j = c->ao0[B] + b;
                    diag[i * n + j] = v;
                    diag[j * n + i] = v;
                    if (v > m) m = v;
                }
            c->qmax[kab] = sqrt(m);
        }
        free(cart);
        free(t1);
    }
    return 0;
}

/* All integrals (ij|kl) with k in shell C, l in shell D: out[(k_local*nsd + l_local)][i][j], each an
 * (nao,nao) symmetric matrix.  Quartets below the Schwarz bound `screen` are left zero.
 * qc_eri_diag must have been called. */
int qc_eri_cols2(void *h, int C, int D, double screen, double *out, int lower_only);
int qc_eri_cols(void *h, int C, int D, double screen, double *out) { return qc_eri_cols2(h, C, D, screen, out, 0); }

/* lower_only: each matrix (..|kl) is written for i >= j only (the shell pairs are stored A >= B); the transposed
 * element is the caller's to fill -- the single-element strided stores of the mirror image cost as much as the
 * integrals themselves at nao ~ 500 (cache and TLB misses over up to 95 MB), and a GPU consumer mirrors for free. */
int qc_eri_cols2(void *h, int C, int D, double screen, double *out, int lower_only)
{
    EriCtx *c = (EriCtx *)h;
    if (!c || !c->qmax || C < 0 || D < 0 || C >= c->nshell || D >= c->nshell) return -1;
    const size_t n = (size_t)c->nao;
    const int kcd = pair_index(C, D);
    const int swap = C < D; /* stored pair is (max, min) */
    const int nsc = 2 * c->ls[C] + 1, nsd = 2 * c->ls[D] + 1;
    const size_t nout = n * n * nsc * nsd;
#pragma omp parallel
    {
        /* zero-fill in parallel: up to 49 matrices of nao^2 doubles (95 MB at nao 494), which one thread clears in
         * about the time sixteen take for the block's integrals */
#pragma omp for schedule(static)
        for (long blk = 0; blk < (long)((nout + 65535) / 65536); ++blk) {
            const size_t lo = (size_t)blk * 65536, hi = lo + 65536 < nout ? lo + 65536 : nout;
            memset(out + lo, 0, sizeof(double) * (hi - lo));
        }
        double *cart = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        double *t1 = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        static _Thread_local double R[RDIM][RDIM][RDIM];
#pragma omp for schedule(dynamic)
        for (int kab = 0; kab < c->npairs; ++kab) {
            if (c->qmax[kab] * c->qmax[kcd] < screen) continue;
            const int A = c->pA[kab], B = c->pB[kab];
            const int nsa = 2 * c->ls[A] + 1, nsb = 2 * c->ls[B] + 1;
            quartet(c, kab, kcd, cart, t1, R);
            /* block is [a][b][c'][d'] with (c',d') over the stored (max,min) shells */
            const int n3 = swap ? nsd : nsc, n4 = swap ? nsc : nsd;
            for (int a = 0; a < nsa; ++a)
                for (int b = 0; b < nsb; ++b)
                    for (int k = 0; k < nsc; ++k)
                        for (int l = 0; l < nsd; ++l) {
                            const int c3 = swap ? l : k, c4 = swap ? k : l;
                            const double v = cart[(((size_t)a * nsb + b) * n3 + c3) * n4 + c4];
                            const size_t i = c->ao0[A] + a, j = c->ao0[B] + b;
                            double *m = out + (size_t)(k * nsd + l) * n * n;
                            m[i * n + j] = v;
                            if (!lower_only) m[j * n + i] = v;
                        }
        }
        free(cart);
        free(t1);
    }
    return 0;
}

/* ---- nuclear gradient: derivative integrals, contracted as they are made --------------------- */
/* A Cartesian primitive moves with its centre by  d/dA_x x^i exp(-a x_A^2) = 2 a x^(i+1) exp - i x^(i-1) exp,  so the
 * derivative of an integral by the bra centre is the same integral over the shell raised and lowered in that dimension:
 * E tables to la + 1 (R to L + 1), nothing else new.  Only the bra is differentiated: for symmetric D and W
 *     sum_{mu nu} D_mu,nu d<mu|O|nu>/dR_X (basis part) = 2 sum_{mu on X, nu} D_mu,nu <d mu/dX|O|nu>,
 * and for the two-electron energy, by the eightfold symmetry of (mu nu|lam sig),
 *     d/dR_X [1/2 sum D D (..|..) - c_hf/4 sum D D (..|..)] = sum_{mu on X} sum_{nu lam sig} [2 D_mu,nu D_lam,sig - c_hf D_mu,lam D_nu,sig] (mu' nu|lam sig).
 * The matrices come in over spherical functions; each shell block is rotated to Cartesian components once. */

/* Cartesian block of a spherical one: Mc[ca][cb] = sum Ta[ma][ca] Tb[mb][cb] M[ia + ma][ib + mb] */
static void block_to_cart(int la, int lb, const double *M, int ld, int ia, int ib, double *Mc)
{
    double Ta[7][MAXCART], Tb[7][MAXCART];
    sph_matrix(la, Ta);
    sph_matrix(lb, Tb);
    const int nca = NCART(la), ncb = NCART(lb);
    memset(Mc, 0, sizeof(double) * nca * ncb);
    for (int ma = 0; ma < 2 * la + 1; ++ma)
        for (int mb = 0; mb < 2 * lb + 1; ++mb) {
            const double d = M[(size_t)(ia + ma) * ld + ib + mb];
            for (int ca = 0; ca < nca; ++ca)
                if (Ta[ma][ca] != 0.0)
                    for (int cb = 0; cb < ncb; ++cb) Mc[ca * ncb + cb] += Ta[ma][ca] * Tb[mb][cb] * d;
        }
}

/* out (3, natm, 3): [0] -tr(W dS/dR_A), [1] tr(D dT/dR_A), [2] the basis-centre part of tr(D dV/dR_A) with
 * V = -sum_c q_c / |r - R_c| over the ncen charged centres (the nuclei, and the external charges of an embedded run); the
 * operator part of V -- the field of the electrons at a nucleus -- is qc_point_field's.  D, W symmetric (nao, nao);
 * shl_atom: the atom that owns each shell. */
int qc_grad1e(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
              const int *ao0, const double *ex, const double *cf, int nao, const int *shl_atom, int natm,
              int ncen, const double *cen_xyz, const double *cen_q, const double *D, const double *W, double *out)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX || shl_atom[s] < 0 || shl_atom[s] >= natm) return -1;
    double *acc = (double *)calloc((size_t)nshell * 9, sizeof(double));
#pragma omp parallel for schedule(dynamic)
    for (int A = 0; A < nshell; ++A) {
        double gs[3] = {0, 0, 0}, gt[3] = {0, 0, 0}, gv[3] = {0, 0, 0};
        const int la = ls[A], nca = NCART(la);
        int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
        cart_components(la, ax, ay, az);
        const double *RA = xyz + 3 * A;
        for (int B = 0; B < nshell; ++B) {
            const int lb = ls[B], ncb = NCART(lb), L = la + lb + 1;
            cart_components(lb, bx, by, bz);
            double Dc[MAXCART * MAXCART], Wc[MAXCART * MAXCART];
            block_to_cart(la, lb, D, nao, ao0[A], ao0[B], Dc);
            block_to_cart(la, lb, W, nao, ao0[A], ao0[B], Wc);
            const double *RB = xyz + 3 * B;
            const double R2 = dist2(RA, RB);
            for (int pa = 0; pa < nprim[A]; ++pa)
                for (int pb = 0; pb < nprim[B]; ++pb) {
                    const double a = ex[off[A] + pa], b = ex[off[B] + pb], p = a + b;
                    const double cc = cf[off[A] + pa] * cf[off[B] + pb];
                    if (!prim_pair_kept(a, b, cc, R2)) continue;
                    double E[3][LMAX + 3][LMAX + 3][2 * LMAX + 5];
                    for (int d = 0; d < 3; ++d) hermite_E(la + 1, lb + 2, a, b, RA[d] - RB[d], E[d]);
                    const double P[3] = {(a * RA[0] + b * RB[0]) / p, (a * RA[1] + b * RB[1]) / p, (a * RA[2] + b * RB[2]) / p};
                    const double s0 = cc * pow(M_PI / p, 1.5);
                    /* dE[x][ca][cb][t]: Hermite coefficients, in dimension x, of the bra raised and lowered */
                    static _Thread_local double dE[3][MAXCART][MAXCART][2 * LMAX + 2];
                    for (int ca = 0; ca < nca; ++ca)
                        for (int cb = 0; cb < ncb; ++cb) {
                            const int i[3] = {ax[ca], ay[ca], az[ca]}, j[3] = {bx[cb], by[cb], bz[cb]};
                            double s1[3], k1[3], ds[3], dk[3];
                            for (int d = 0; d < 3; ++d) {
                                const int jd = j[d];
                                double sv[3], kv[3]; /* the 1-D overlap and kinetic factors at i - 1, i, i + 1 */
                                for (int m = 0; m < 3; ++m) {
                                    const int ii = i[d] - 1 + m;
                                    sv[m] = kv[m] = 0.0;
                                    if (ii < 0) continue;
                                    sv[m] = E[d][ii][jd][0];
                                    kv[m] = -2.0 * b * b * E[d][ii][jd + 2][0] + b * (2 * jd + 1) * sv[m];
                                    if (jd >= 2) kv[m] -= 0.5 * jd * (jd - 1) * E[d][ii][jd - 2][0];
                                }
                                s1[d] = sv[1]; k1[d] = kv[1];
                                ds[d] = 2.0 * a * sv[2] - i[d] * sv[0];
                                dk[d] = 2.0 * a * kv[2] - i[d] * kv[0];
                                for (int t = 0; t <= i[d] + jd + 1; ++t)
                                    dE[d][ca][cb][t] = 2.0 * a * E[d][i[d] + 1][jd][t] - (i[d] ? i[d] * E[d][i[d] - 1][jd][t] : 0.0);
                            }
                            const double dw = s0 * Wc[ca * ncb + cb], dd = s0 * Dc[ca * ncb + cb];
                            for (int x = 0; x < 3; ++x) {
                                const int y = (x + 1) % 3, z = (x + 2) % 3;
                                gs[x] += dw * ds[x] * s1[y] * s1[z];
                                gt[x] += dd * (dk[x] * s1[y] * s1[z] + ds[x] * k1[y] * s1[z] + ds[x] * s1[y] * k1[z]);
                            }
                        }
                    for (int c = 0; c < ncen; ++c) {
                        static _Thread_local double R[RDIM][RDIM][RDIM];
                        const double PC[3] = {P[0] - cen_xyz[3 * c], P[1] - cen_xyz[3 * c + 1], P[2] - cen_xyz[3 * c + 2]};
                        hermite_R(L, p, PC, R);
                        const double pref = -cen_q[c] * 2.0 * M_PI / p * cc;
                        for (int ca = 0; ca < nca; ++ca)
                            for (int cb = 0; cb < ncb; ++cb) {
                                const double dd = pref * Dc[ca * ncb + cb];
                                if (dd == 0.0) continue;
                                const int i[3] = {ax[ca], ay[ca], az[ca]}, j[3] = {bx[cb], by[cb], bz[cb]};
                                for (int x = 0; x < 3; ++x) {
                                    const double *e0 = x == 0 ? dE[0][ca][cb] : E[0][i[0]][j[0]];
                                    const double *e1 = x == 1 ? dE[1][ca][cb] : E[1][i[1]][j[1]];
                                    const double *e2 = x == 2 ? dE[2][ca][cb] : E[2][i[2]][j[2]];
                                    double v = 0.0;
                                    for (int t = 0; t <= i[0] + j[0] + (x == 0); ++t)
                                        for (int u = 0; u <= i[1] + j[1] + (x == 1); ++u)
                                            for (int w = 0; w <= i[2] + j[2] + (x == 2); ++w) v += e0[t] * e1[u] * e2[w] * R[t][u][w];
                                    gv[x] += dd * v;
                                }
                            }
                    }
                }
        }
        for (int x = 0; x < 3; ++x) { acc[9 * A + x] = gs[x]; acc[9 * A + 3 + x] = gt[x]; acc[9 * A + 6 + x] = gv[x]; }
    }
    memset(out, 0, sizeof(double) * 9 * natm);
    for (int A = 0; A < nshell; ++A)   /* in shell order: the same sum whatever the thread count */
        for (int x = 0; x < 3; ++x) {
            out[3 * shl_atom[A] + x] -= 2.0 * acc[9 * A + x];
            out[3 * natm + 3 * shl_atom[A] + x] += 2.0 * acc[9 * A + 3 + x];
            out[6 * natm + 3 * shl_atom[A] + x] += 2.0 * acc[9 * A + 6 + x];
        }
    free(acc);
    return 0;
}

/* transposed rotation of one index of a 4-index block, spherical -> Cartesian components of a DENSITY:
 * in (n0, ns, n2) -> out (n0, nc, n2), out[c] = sum_m T[m][c] in[m] */
static void rot_axis_t(int l, int n0, int n2, const double *in, double *out)
{
    double T[7][MAXCART];
    sph_matrix(l, T);
    const int nc = NCART(l), ns = 2 * l + 1;
    for (int i0 = 0; i0 < n0; ++i0)
        for (int c = 0; c < nc; ++c)
            for (int i2 = 0; i2 < n2; ++i2) {
                double s = 0.0;
                for (int m = 0; m < ns; ++m)
                    if (T[m][c] != 0.0) s += T[m][c] * in[((size_t)i0 * ns + m) * n2 + i2];
                out[((size_t)i0 * nc + c) * n2 + i2] = s;
            }
}

/* g3[x] += sum over Cartesian components of Gc[a][b][c][d] d(ab|cd)/dA_x for shells A, B, C, D (any order).  The ket is
 * expanded as in quartet(); the bra's Hermite lists carry the raised and lowered first shell. */
static void grad_quartet(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off, const double *ex,
                         const double *cf, int A, int B, int C, int D, const double *Gc, double g3[3])
{
    (void)nshell;
    const int la = ls[A], lb = ls[B], lc = ls[C], ld = ls[D];
    const int nca = NCART(la), ncb = NCART(lb), ncc = NCART(lc), ncd = NCART(ld), nkb = nca * ncb, nkc = ncc * ncd;
    int ax[MAXCART], ay[MAXCART], az[MAXCART], bx[MAXCART], by[MAXCART], bz[MAXCART];
    int cx[MAXCART], cy[MAXCART], cz[MAXCART], dx[MAXCART], dy[MAXCART], dz[MAXCART];
    cart_components(la, ax, ay, az); cart_components(lb, bx, by, bz);
    cart_components(lc, cx, cy, cz); cart_components(ld, dx, dy, dz);
    const int Lab = la + lb + 1, L = Lab + lc + ld;
    const double *RA = xyz + 3 * A, *RB = xyz + 3 * B, *RC = xyz + 3 * C, *RD = xyz + 3 * D;
    const double R2ab = dist2(RA, RB), R2cd = dist2(RC, RD);
    const double two_pi_52 = 34.986836655249725; /* 2 pi^(5/2) */
    enum { MAXE = 27, MAXD = 48 };   /* bra terms: (i_x + j_x + 2)(i_y + j_y + 1)(i_z + j_z + 1) <= 36 at l = 3 */
    static _Thread_local double wk[MAXCART * MAXCART][MAXE], wb[3][MAXCART * MAXCART][MAXD];
    static _Thread_local int ok_[MAXCART * MAXCART][MAXE], ob[3][MAXCART * MAXCART][MAXD], nk[MAXCART * MAXCART], nb[3][MAXCART * MAXCART];
    static _Thread_local double g[RDIM * RDIM * RDIM], R[RDIM][RDIM][RDIM];
    static _Thread_local double Eab[3][LMAX + 3][LMAX + 3][2 * LMAX + 5], Ecd[3][LMAX + 3][LMAX + 3][2 * LMAX + 5];
    const double *Rf = &R[0][0][0];
    int tuv[(HDIM + 1) * (HDIM + 1) * (HDIM + 1)], ntuv = 0;
    for (int t = 0; t <= Lab; ++t)
        for (int u = 0; u <= Lab - t; ++u)
            for (int v = 0; v <= Lab - t - u; ++v) tuv[ntuv++] = (t * RDIM + u) * RDIM + v;
    int live[MAXCART * MAXCART];   /* ket components that meet a non-zero density */
    for (int kc = 0; kc < nkc; ++kc) {
        live[kc] = 0;
        for (int kb = 0; kb < nkb && !live[kc]; ++kb) live[kc] = Gc[(size_t)kb * nkc + kc] != 0.0;
    }
    for (int pc = 0; pc < nprim[C]; ++pc)
        for (int pd = 0; pd < nprim[D]; ++pd) {
            const double c_ = ex[off[C] + pc], d_ = ex[off[D] + pd], q = c_ + d_;
            const double ccd = cf[off[C] + pc] * cf[off[D] + pd];
            if (!prim_pair_kept(c_, d_, ccd, R2cd)) continue;
            double Q[3];
            for (int d = 0; d < 3; ++d) {
                hermite_E(lc, ld, c_, d_, RC[d] - RD[d], Ecd[d]);
                Q[d] = (c_ * RC[d] + d_ * RD[d]) / q;
            }
            for (int ic = 0; ic < ncc; ++ic)
                for (int id = 0; id < ncd; ++id) {
                    const int k = ic * ncd + id;
                    int n = 0;
                    for (int a1 = 0; a1 <= cx[ic] + dx[id]; ++a1) {
                        const double e1 = Ecd[0][cx[ic]][dx[id]][a1];
                        for (int a2 = 0; a2 <= cy[ic] + dy[id]; ++a2) {
                            const double e2 = e1 * Ecd[1][cy[ic]][dy[id]][a2];
                            for (int a3 = 0; a3 <= cz[ic] + dz[id]; ++a3) {
                                const double e3 = e2 * Ecd[2][cz[ic]][dz[id]][a3];
                                wk[k][n] = ((a1 + a2 + a3) & 1) ? -e3 : e3;
                                ok_[k][n] = (a1 * RDIM + a2) * RDIM + a3;
                                ++n;
                            }
                        }
                    }
                    nk[k] = n;
                }
            for (int pa = 0; pa < nprim[A]; ++pa)
                for (int pb = 0; pb < nprim[B]; ++pb) {
                    const double a = ex[off[A] + pa], b = ex[off[B] + pb], p = a + b;
                    const double cab = cf[off[A] + pa] * cf[off[B] + pb];
                    if (!prim_pair_kept(a, b, cab, R2ab)) continue;
                    double PQ[3];
                    for (int d = 0; d < 3; ++d) {
                        hermite_E(la + 1, lb, a, b, RA[d] - RB[d], Eab[d]);
                        PQ[d] = (a * RA[d] + b * RB[d]) / p - Q[d];
                    }
                    hermite_R(L, p * q / (p + q), PQ, R);
                    const double pref = two_pi_52 / (p * q * sqrt(p + q)) * cab * ccd;
                    for (int ia = 0; ia < nca; ++ia)
                        for (int ib = 0; ib < ncb; ++ib) {
                            const int k = ia * ncb + ib;
                            const int i[3] = {ax[ia], ay[ia], az[ia]}, j[3] = {bx[ib], by[ib], bz[ib]};
                            for (int x = 0; x < 3; ++x) {
                                double dEx[2 * LMAX + 2];
                                for (int t = 0; t <= i[x] + j[x] + 1; ++t)
                                    dEx[t] = 2.0 * a * Eab[x][i[x] + 1][j[x]][t] - (i[x] ? i[x] * Eab[x][i[x] - 1][j[x]][t] : 0.0);
                                const double *e0 = x == 0 ? dEx : Eab[0][i[0]][j[0]];
                                const double *e1 = x == 1 ? dEx : Eab[1][i[1]][j[1]];
                                const double *e2 = x == 2 ? dEx : Eab[2][i[2]][j[2]];
                                int n = 0;
                                for (int t = 0; t <= i[0] + j[0] + (x == 0); ++t)
                                    for (int u = 0; u <= i[1] + j[1] + (x == 1); ++u)
                                        for (int v = 0; v <= i[2] + j[2] + (x == 2); ++v) {
                                            wb[x][k][n] = pref * e0[t] * e1[u] * e2[v];
                                            ob[x][k][n] = (t * RDIM + u) * RDIM + v;
                                            ++n;
                                        }
                                nb[x][k] = n;
                            }
                        }
                    for (int kc = 0; kc < nkc; ++kc) {
                        if (!live[kc]) continue;
                        const int ne = nk[kc];
                        for (int m = 0; m < ntuv; ++m) {
                            const double *Rm = Rf + tuv[m];
                            double sacc = 0.0;
                            for (int e = 0; e < ne; ++e) sacc += wk[kc][e] * Rm[ok_[kc][e]];
                            g[tuv[m]] = sacc;
                        }
                        for (int kb = 0; kb < nkb; ++kb) {
                            const double gv = Gc[(size_t)kb * nkc + kc];
                            if (gv == 0.0) continue;
                            for (int x = 0; x < 3; ++x) {
                                double sacc = 0.0;
                                for (int e = 0; e < nb[x][kb]; ++e) sacc += wb[x][kb][e] * g[ob[x][kb][e]];
                                g3[x] += gv * sacc;
                            }
                        }
                    }
                }
        }
}

/* out (natm, 3): the derivative of  1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum D_ac D_bd (ab|cd)  by the centres, D symmetric
 * (Ms null: qc_grad2e), or with the spin density Ms the open-shell quartet of qc_grad2e_spin below.
 * Every ordered bra pair (A, B) with every ket pair C >= D: the derivative by the centre of A alone, see above.  The dense
 * ERI is never built; primitive pairs are screened as everywhere in the engine.  OpenMP over the first shell. */
static int grad2e_loop(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                       const int *ao0, const double *ex, const double *cf, int nao, const int *shl_atom, int natm,
                       const double *Dm, const double *Ms, double c_hf, double *out)
{
    for (int s = 0; s < nshell; ++s)
        if (ls[s] < 0 || ls[s] > LMAX || shl_atom[s] < 0 || shl_atom[s] >= natm) return -1;
    double *acc = (double *)calloc((size_t)nshell * nshell * 3, sizeof(double));
    const size_t n = (size_t)nao;
#pragma omp parallel
    {
        double *Gs = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
        double *Gc = (double *)malloc(sizeof(double) * QUARTET_DOUBLES);
#pragma omp for schedule(dynamic)
        for (int AB = 0; AB < nshell * nshell; ++AB) {
            const int A = AB / nshell, B = AB - A * nshell;
            const int la = ls[A], lb = ls[B], nsa = 2 * la + 1, nsb = 2 * lb + 1;
            double g3[3] = {0, 0, 0};
            for (int C = 0; C < nshell; ++C)
                for (int D = 0; D <= C; ++D) {
                    const int lc = ls[C], ld = ls[D], nsc = 2 * lc + 1, nsd = 2 * ld + 1;
                    const double f = C == D ? 1.0 : 2.0;   /* (..|lam sig) = (..|sig lam): an off-diagonal ket pair stands for both orders */
                    double big = 0.0;
                    for (int ma = 0; ma < nsa; ++ma)
                        for (int mb = 0; mb < nsb; ++mb)
                            for (int mc = 0; mc < nsc; ++mc)
                                for (int md = 0; md < nsd; ++md) {
                                    const size_t i = ao0[A] + ma, j = ao0[B] + mb, k = ao0[C] + mc, l = ao0[D] + md;
                                    double v = 2.0 * f * Dm[i * n + j] * Dm[k * n + l];
                                    if (c_hf != 0.0 && !Ms)
                                        v -= c_hf * (C == D ? Dm[i * n + k] * Dm[j * n + l]
                                                            : Dm[i * n + k] * Dm[j * n + l] + Dm[i * n + l] * Dm[j * n + k]);
                                    else if (c_hf != 0.0)
                                        v -= c_hf * (C == D ? Dm[i * n + k] * Dm[j * n + l] + Ms[i * n + k] * Ms[j * n + l]
                                                            : Dm[i * n + k] * Dm[j * n + l] + Ms[i * n + k] * Ms[j * n + l] +
                                                                  Dm[i * n + l] * Dm[j * n + k] + Ms[i * n + l] * Ms[j * n + k]);
                                    Gs[((ma * nsb + mb) * nsc + mc) * nsd + md] = v;
                                    if (fabs(v) > big) big = fabs(v);
                                }
                    if (big == 0.0) continue;
                    const int ncb = NCART(lb), ncc = NCART(lc), ncd = NCART(ld);
                    rot_axis_t(la, 1, nsb * nsc * nsd, Gs, Gc);
                    rot_axis_t(lb, NCART(la), nsc * nsd, Gc, Gs);
                    rot_axis_t(lc, NCART(la) * ncb, nsd, Gs, Gc);
                    rot_axis_t(ld, NCART(la) * ncb * ncc, 1, Gc, Gs);
                    (void)ncd;
                    grad_quartet(nshell, xyz, ls, nprim, off, ex, cf, A, B, C, D, Gs, g3);
                }
            for (int x = 0; x < 3; ++x) acc[3 * (size_t)AB + x] = g3[x];
        }
        free(Gs);
        free(Gc);
    }
    memset(out, 0, sizeof(double) * 3 * natm);
    for (int AB = 0; AB < nshell * nshell; ++AB)   /* in pair order: the same sum whatever the thread count */
        for (int x = 0; x < 3; ++x) out[3 * shl_atom[AB / nshell] + x] += acc[3 * (size_t)AB + x];
    free(acc);
    return 0;
}

int qc_grad2e(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
              const int *ao0, const double *ex, const double *cf, int nao, const int *shl_atom, int natm,
              const double *Dm, double c_hf, double *out)
{
    return grad2e_loop(nshell, xyz, ls, nprim, off, ao0, ex, cf, nao, shl_atom, natm, Dm, NULL, c_hf, out);
}

/* The same for an open-shell state, Dm = D_a + D_b and Ms = D_a - D_b (both symmetric): the derivative of
 * 1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum (D_ac D_bd + M_ac M_bd) (ab|cd), one pass with the extended density quartet. */
int qc_grad2e_spin(int nshell, const double *xyz, const int *ls, const int *nprim, const int *off,
                   const int *ao0, const double *ex, const double *cf, int nao, const int *shl_atom, int natm,
                   const double *Dm, const double *Ms, double c_hf, double *out)
{
    if (!Ms) return -1;
    return grad2e_loop(nshell, xyz, ls, nprim, off, ao0, ex, cf, nao, shl_atom, natm, Dm, Ms, c_hf, out);
}

/* worker threads of the OpenMP regions above (default: every visible core, which oversubscribes a
 * cgroup CPU share) */
void qc_set_threads(int n)
{
#ifdef _OPENMP
    if (n > 0) omp_set_num_threads(n);
#else
    (void)n;
#endif
}
