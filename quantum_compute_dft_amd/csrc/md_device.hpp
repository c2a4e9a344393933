// McMurchie-Davidson building blocks on the device, shared by the translation units that evaluate Coulomb-type Gaussian
// integrals (eri_cols.hip: two-electron columns; point_coulomb.hip: one-electron integrals at a point; grad2e.hip: the
// two-electron derivative quartets): the Boys
// function, the Hermite expansion coefficients of one Cartesian direction, the Cartesian component tables and the
// rotation to real solid harmonics.  Device counterparts of integrals.c::boys / hermite_E / cart_components /
// sph_matrix, term for term.  Everything has internal linkage: every unit that includes this header owns its copy of
// the __constant__ tables and fills it with fill_tables() when a handle is opened.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

namespace {

constexpr int EC_MAXC = 10;   // Cartesian components of an f shell
constexpr int EC_ED = 4 * 4 * 7; // E[i][j][t], i, j <= 3, t <= 6

__constant__ int c_cx[4][EC_MAXC], c_cy[4][EC_MAXC], c_cz[4][EC_MAXC];
__constant__ double c_sph[4][7][EC_MAXC];

__device__ __forceinline__ int ncart(int l) { return (l + 1) * (l + 2) / 2; }

// F_0..F_n(x): integrals.c::boys, term for term
__device__ void boys(int n, double x, double *F)
{
    if (x < 1e-13) {
        for (int m = 0; m <= n; ++m) F[m] = 1.0 / (2 * m + 1);
        return;
    }
    if (x > 40.0) {
        F[0] = 0.5 * sqrt(M_PI / x);
        const double ex = exp(-x);
        for (int m = 0; m < n; ++m) F[m + 1] = ((2 * m + 1) * F[m] - ex) / (2.0 * x);
        return;
    }
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

// The same function with the order fixed at compile time: every loop over m unrolls, so an F that lives in registers
// is never indexed at run time (a lane-private array indexed at run time goes to scratch memory).  Same three
// branches, same order of operations.
template <int N> __device__ __forceinline__ void boys_fixed(double x, double (&F)[N + 1])
{
    if (x < 1e-13) {
#pragma unroll
        for (int m = 0; m <= N; ++m) F[m] = 1.0 / (2 * m + 1);
        return;
    }
    const double ex = exp(-x);
    if (x > 40.0) {
        F[0] = 0.5 * sqrt(M_PI / x);
#pragma unroll
        for (int m = 0; m < N; ++m) F[m + 1] = ((2 * m + 1) * F[m] - ex) / (2.0 * x);
        return;
    }
    double term = 1.0 / (2 * N + 1), sum = term;
    for (int k = 1; k < 400; ++k) {
        term *= 2.0 * x / (2 * N + 2 * k + 1);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    F[N] = ex * sum;
#pragma unroll
    for (int m = N; m > 0; --m) F[m - 1] = (2.0 * x * F[m] + ex) / (2 * m - 1);
}

// E[i][j][t] of one Cartesian direction (integrals.c::hermite_E), i <= la, j <= lb; E is [4][4][7]
__device__ void hermite_E(int la, int lb, double a, double b, double XAB, double *E)
{
    const double p = a + b, mu = a * b / p, XPA = -b / p * XAB, XPB = a / p * XAB;
    for (int i = 0; i < EC_ED; ++i) E[i] = 0.0;
    auto at = [&](int i, int j, int t) -> double & { return E[(i * 4 + j) * 7 + t]; };
    auto get = [&](int i, int j, int t) -> double { return (t < 0 || t > i + j) ? 0.0 : E[(i * 4 + j) * 7 + t]; };
    at(0, 0, 0) = exp(-mu * XAB * XAB);
    for (int i = 0; i <= la; ++i) {
        if (i > 0)
            for (int t = 0; t <= i; ++t) at(i, 0, t) = XPA * get(i - 1, 0, t) + get(i - 1, 0, t - 1) / (2 * p) + (t + 1) * get(i - 1, 0, t + 1);
        for (int j = 1; j <= lb; ++j)
            for (int t = 0; t <= i + j; ++t) at(i, j, t) = XPB * get(i, j - 1, t) + get(i, j - 1, t - 1) / (2 * p) + (t + 1) * get(i, j - 1, t + 1);
    }
}

// The same recurrence into a table dimensioned by the caller, E[NI][NJ][NT] (la < NI, lb < NJ, la + lb < NT): a shell
// raised by a centre derivative needs i <= 4, t <= 7 (grad2e.hip).  Rows i <= la, j <= lb are written, zero at t > i + j;
// the others are not touched.
template <int NI, int NJ, int NT> __device__ void hermite_E_dim(int la, int lb, double a, double b, double XAB, double *E)
{
    const double p = a + b, mu = a * b / p, XPA = -b / p * XAB, XPB = a / p * XAB;
    for (int i = 0; i <= la; ++i)
        for (int k = 0; k < (lb + 1) * NT; ++k) E[i * NJ * NT + k] = 0.0;
    auto at = [&](int i, int j, int t) -> double & { return E[(i * NJ + j) * NT + t]; };
    auto get = [&](int i, int j, int t) -> double { return (t < 0 || t > i + j) ? 0.0 : E[(i * NJ + j) * NT + t]; };
    at(0, 0, 0) = exp(-mu * XAB * XAB);
    for (int i = 0; i <= la; ++i) {
        if (i > 0)
            for (int t = 0; t <= i; ++t) at(i, 0, t) = XPA * get(i - 1, 0, t) + get(i - 1, 0, t - 1) / (2 * p) + (t + 1) * get(i - 1, 0, t + 1);
        for (int j = 1; j <= lb; ++j)
            for (int t = 0; t <= i + j; ++t) at(i, j, t) = XPB * get(i, j - 1, t) + get(i, j - 1, t - 1) / (2 * p) + (t + 1) * get(i, j - 1, t + 1);
    }
}

void fill_tables()
{
    int cx[4][EC_MAXC] = {{0}}, cy[4][EC_MAXC] = {{0}}, cz[4][EC_MAXC] = {{0}};
    for (int l = 0; l < 4; ++l) {
        int n = 0;
        for (int lx = l; lx >= 0; --lx)
            for (int ly = l - lx; ly >= 0; --ly) { cx[l][n] = lx; cy[l][n] = ly; cz[l][n] = l - lx - ly; ++n; }
    }
    double T[4][7][EC_MAXC];
    memset(T, 0, sizeof T);
    T[0][0][0] = 0.282094791773878143;
    for (int i = 0; i < 3; ++i) T[1][i][i] = 0.488602511902919921;
    { // l = 2: xx xy xz yy yz zz (integrals.c::sph_matrix)
        const double c = 1.092548430592079070, d = 0.315391565252520002, e = 0.546274215296039535;
        T[2][0][1] = c; T[2][1][4] = c;
        T[2][2][0] = -d; T[2][2][3] = -d; T[2][2][5] = 2 * d;
        T[2][3][2] = c;
        T[2][4][0] = e; T[2][4][3] = -e;
    }
    { // l = 3: xxx xxy xxz xyy xyz xzz yyy yyz yzz zzz
        const double f3 = 0.590043589926643510, f2 = 2.890611442640554055, f1 = 0.457045799464465739,
                     f0 = 0.373176332590115391, f2b = 1.445305721320277020;
        T[3][0][1] = 3 * f3; T[3][0][6] = -f3;
        T[3][1][4] = f2;
        T[3][2][8] = 4 * f1; T[3][2][1] = -f1; T[3][2][6] = -f1;
        T[3][3][9] = 2 * f0; T[3][3][2] = -3 * f0; T[3][3][7] = -3 * f0;
        T[3][4][5] = 4 * f1; T[3][4][0] = -f1; T[3][4][3] = -f1;
        T[3][5][2] = f2b; T[3][5][7] = -f2b;
        T[3][6][0] = f3; T[3][6][3] = -3 * f3;
    }
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_cx), cx, sizeof cx);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_cy), cy, sizeof cy);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_cz), cz, sizeof cz);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(c_sph), T, sizeof T);
}

} // namespace
