"""Independent high-precision reference for the Gaussian integrals of the product (csrc/integrals.c on the host,
csrc/eri_cols.hip on the device).  Test infrastructure only: pure Python on mpmath, never imported by the product.

What it shares with the product is a specification, not code:
  * contracted real-solid-harmonic shells s..f; component order p: x, y, z; d: xy, yz, z2, xz, x2-y2; f: m = -3..3;
  * every contracted function has unit self-overlap.

Everything else is its own:
  * the Cartesian -> real-solid-harmonic coefficients are FITTED: r^l times the real combinations of mpmath.spherharm
    are evaluated at generic points and expanded in the monomials x^i y^j z^k (i + j + k = l) by a linear solve;
  * the normalisation is the reciprocal square root of the self-overlap of each contracted function, computed here from
    the raw exponents and contraction coefficients;
  * the two-electron and nuclear-attraction integrals use the two-dimensional-integral factorisation of Rys, Dupuis and
    King: (ab|cd) = pref * int_0^1 exp(-x t^2) Ix(t^2) Iy(t^2) Iz(t^2) dt, where the I's obey the RDK recurrences in
    the total bra / ket powers followed by a one-dimensional horizontal transfer.  No Hermite expansion coefficients
    E_t^{ij} and no Hermite Coulomb integrals R_tuv appear.  Ix Iy Iz is a polynomial of degree L = la+lb+lc+ld in
    u = t^2, so the t integral is done EXACTLY by an interpolatory rule on L + 1 fixed nodes u_k whose weights solve
    sum_k w_k u_k^m = F_m(x), m = 0..L  (no Rys roots are needed: any L + 1 distinct nodes integrate degree L exactly;
    the price is a Vandermonde solve, paid for with working digits);
  * the Boys function is F_m(x) = gamma(m + 1/2, x) / (2 x^(m + 1/2)) from mpmath.gammainc, 1 / (2m + 1) at x = 0:
    no series, asymptote or recursion of its own;
  * overlap and kinetic energy use the Obara-Saika one-dimensional overlap recurrence.

Working precision: DPS decimal digits (default 100).  The Vandermonde solve loses about 10 digits at L = 12 and the
alternating sum over nodes loses up to ~30 more at x ~ 2000, which leaves well above 40 significant digits.
"""
import math
import random
from functools import lru_cache
from itertools import product

import numpy as np
from mpmath import mp, mpf

DPS = 100


class Shell:
    """One contracted shell: angular momentum, centre (bohr), RAW exponents and contraction coefficients."""

    def __init__(self, l, centre, exps, coefs):
        self.l = int(l)
        self.centre = tuple(float(x) for x in centre)
        self.exps = tuple(float(x) for x in exps)
        self.coefs = tuple(float(x) for x in coefs)
        assert len(self.exps) == len(self.coefs) and 0 <= self.l <= 3

    def key(self):
        return (self.l, self.centre, self.exps, self.coefs)

    def moved(self, axis, step):
        """A copy whose centre is displaced by `step` along `axis` and kept as mpf at DPS digits, NOT rounded to double:
        the finite-difference references (tests/golden/make_grad_reference.py) step by far less than a double resolves."""
        out = Shell(self.l, self.centre, self.exps, self.coefs)
        with mp.workdps(DPS):
            c = [mpf(x) for x in self.centre]
            c[axis] = c[axis] + mpf(step)
            out.centre = tuple(c)
        return out

    @property
    def nfun(self):
        return 2 * self.l + 1


def _work(fn):
    def wrapped(*a, **k):
        with mp.workdps(DPS):
            return fn(*a, **k)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


# ----------------------------------------------------------------------------------------------- angular part
def cart_powers(l):
    return [(i, j, l - i - j) for i in range(l, -1, -1) for j in range(l - i, -1, -1)]


def _m_order(l):
    return [1, -1, 0] if l == 1 else list(range(-l, l + 1))


def _real_solid_harmonic(l, m, x, y, z):
    r = mp.sqrt(x * x + y * y + z * z)
    theta, phi = mp.acos(z / r), mp.atan2(y, x)
    Y = mp.spherharm(l, abs(m), theta, phi)
    if m == 0:
        v = mp.re(Y)
    elif m > 0:
        v = mp.sqrt(2) * (-1) ** m * mp.re(Y)
    else:
        v = mp.sqrt(2) * (-1) ** m * mp.im(Y)
    return v * r ** l


@lru_cache(maxsize=None)
def _sph_coeffs_at(l, prec):
    carts = cart_powers(l)
    n = len(carts)
    rng = random.Random(7919 + l)
    pts = [tuple(mpf(rng.randint(-4000, 4000)) / 1009 for _ in range(3)) for _ in range(n)]
    M = mp.matrix(n, n)
    for r, (x, y, z) in enumerate(pts):
        for c, (i, j, k) in enumerate(carts):
            M[r, c] = x ** i * y ** j * z ** k
    rows = []
    for m in _m_order(l):
        rhs = mp.matrix([_real_solid_harmonic(l, m, *pt) for pt in pts])
        sol = mp.lu_solve(M, rhs)
        big = max(abs(v) for v in sol)
        rows.append([v if abs(v) > big * mpf(10) ** (-(mp.dps - 25)) else mpf(0) for v in sol])
    return rows


def sph_coeffs(l):
    """rows: the 2l+1 components in the project's order; columns: cart_powers(l).  Unnormalised in the radial sense."""
    return _sph_coeffs_at(l, mp.prec)


# ----------------------------------------------------------------------------------------------- Boys and the t rule
def boys(mmax, x):
    """[F_0(x) .. F_mmax(x)], F_m(x) = int_0^1 t^(2m) exp(-x t^2) dt, from the lower incomplete gamma function."""
    x = mpf(x)
    if x == 0:
        return [1 / mpf(2 * m + 1) for m in range(mmax + 1)]
    half = mpf(1) / 2
    return [mp.gammainc(m + half, 0, x) / (2 * x ** (m + half)) for m in range(mmax + 1)]


@lru_cache(maxsize=None)
def _rule_at(L, prec):
    n = L + 1
    nodes = [(1 - mp.cos(mp.pi * (2 * k + 1) / (2 * n))) / 2 for k in range(n)]        # Chebyshev points of [0, 1]
    Vt = mp.matrix(n, n)
    for m in range(n):
        for k in range(n):
            Vt[m, k] = nodes[k] ** m
    inv = Vt ** -1                                                                     # w = inv * F
    return nodes, [[inv[k, m] for m in range(n)] for k in range(n)]


def _rule(L, x):
    nodes, inv = _rule_at(L, mp.prec)
    F = boys(L, x)
    return nodes, [mp.fdot(row, F) for row in inv]


# ----------------------------------------------------------------------------------------------- 1-D building blocks
def _g2d(nmax, mmax, C00, C00p, B10, B01, B00):
    """RDK two-dimensional integrals G[n][m] / G[0][0]: n = total bra power, m = total ket power of one direction."""
    G = [[None] * (mmax + 1) for _ in range(nmax + 1)]
    G[0][0] = mpf(1)
    for n in range(nmax):
        G[n + 1][0] = C00 * G[n][0] + (n * B10 * G[n - 1][0] if n else 0)
    for m in range(mmax):
        for n in range(nmax + 1):
            v = C00p * G[n][m]
            if m:
                v += m * B01 * G[n][m - 1]
            if n:
                v += n * B00 * G[n - 1][m]
            G[n][m + 1] = v
    return G


def _transfer(G, la, lb, lc, ld, AB, CD):
    """G[n][m] -> I[i][j][k][l] with x_b^j = (x_a + AB)^j and x_d^l = (x_c + CD)^l moved over one power at a time."""
    nm = lc + ld + 1
    bra = [G]
    for _ in range(lb):
        prev = bra[-1]
        bra.append([[prev[i + 1][m] + AB * prev[i][m] for m in range(nm)] for i in range(len(prev) - 1)])
    out = [[None] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        for j in range(lb + 1):
            ket = [bra[j][i]]
            for _ in range(ld):
                prev = ket[-1]
                ket.append([prev[k + 1] + CD * prev[k] for k in range(len(prev) - 1)])
            out[i][j] = [[ket[l][k] for l in range(ld + 1)] for k in range(lc + 1)]
    return out


def _ovl1d(imax, jmax, PA, PB, p):
    """Obara-Saika overlap of x_A^i x_B^j in one direction, S[0][0] = 1."""
    S = [[None] * (jmax + 1) for _ in range(imax + 1)]
    S[0][0] = mpf(1)
    h = 1 / (2 * p)
    for i in range(imax):
        S[i + 1][0] = PA * S[i][0] + (i * h * S[i - 1][0] if i else 0)
    for j in range(jmax):
        for i in range(imax + 1):
            v = PB * S[i][j]
            if i:
                v += i * h * S[i - 1][j]
            if j:
                v += j * h * S[i][j - 1]
            S[i][j + 1] = v
    return S


def _vec(c):
    return [mpf(x) for x in c]


# ----------------------------------------------------------------------------------------------- Cartesian primitives
def _prim_eri_tables(la, lb, lc, ld, a, b, c, d, A, B, C, D):
    """pref-weighted node tables: X, Y, Z as object arrays (K, la+1, lb+1, lc+1, ld+1); the integral of the Cartesian
    component with powers (ax.., bx.., cx.., dx..) is sum_k X[k, ax, bx, cx, dx] Y[k, ay, ..] Z[k, az, ..]."""
    p, q = a + b, c + d
    P = [(a * A[i] + b * B[i]) / p for i in range(3)]
    Q = [(c * C[i] + d * D[i]) / q for i in range(3)]
    AB2 = sum((A[i] - B[i]) ** 2 for i in range(3))
    CD2 = sum((C[i] - D[i]) ** 2 for i in range(3))
    PQ2 = sum((P[i] - Q[i]) ** 2 for i in range(3))
    pref = 2 * mp.pi ** (mpf(5) / 2) / (p * q * mp.sqrt(p + q)) * mp.exp(-a * b / p * AB2 - c * d / q * CD2)
    L = la + lb + lc + ld
    nodes, w = _rule(L, p * q / (p + q) * PQ2)
    tabs = []
    for dim in range(3):
        per_node = []
        for k, u in enumerate(nodes):
            B00 = u / (2 * (p + q))
            B10 = 1 / (2 * p) - q * u / (2 * p * (p + q))
            B01 = 1 / (2 * q) - p * u / (2 * q * (p + q))
            C00 = (P[dim] - A[dim]) - q * (P[dim] - Q[dim]) * u / (p + q)
            C00p = (Q[dim] - C[dim]) + p * (P[dim] - Q[dim]) * u / (p + q)
            G = _g2d(la + lb, lc + ld, C00, C00p, B10, B01, B00)
            if dim == 0:
                f = pref * w[k]
                G = [[g * f for g in row] for row in G]
            per_node.append(_transfer(G, la, lb, lc, ld, A[dim] - B[dim], C[dim] - D[dim]))
        tabs.append(np.array(per_node, dtype=object).reshape(len(nodes), la + 1, lb + 1, lc + 1, ld + 1))
    return tabs


@_work
def cart_prim_eri(powers, exps, centres):
    """[a b|c d] of four UNNORMALISED Cartesian primitives x_A^ax y_A^ay z_A^az exp(-alpha r_A^2), ...:
    powers = 4 x (px, py, pz), exps = 4 exponents, centres = 4 x (x, y, z); arguments may be mpf."""
    (pa, pb, pc, pd), (a, b, c, d) = powers, _vec(exps)
    A, B, C, D = (_vec(v) for v in centres)
    X, Y, Z = _prim_eri_tables(sum(pa), sum(pb), sum(pc), sum(pd), a, b, c, d, A, B, C, D)
    tot = mpf(0)
    for k in range(X.shape[0]):
        tot += X[k, pa[0], pb[0], pc[0], pd[0]] * Y[k, pa[1], pb[1], pc[1], pd[1]] * Z[k, pa[2], pb[2], pc[2], pd[2]]
    return tot


def _prim_ovl_kin(la, lb, a, b, A, B):
    """(S, T) blocks over cart_powers(la) x cart_powers(lb) of two unnormalised primitives."""
    p = a + b
    AB2 = sum((A[i] - B[i]) ** 2 for i in range(3))
    pref = (mp.pi / p) ** (mpf(3) / 2) * mp.exp(-a * b / p * AB2)
    s1 = []
    for dim in range(3):
        Pd = (a * A[dim] + b * B[dim]) / p
        s1.append(_ovl1d(la, lb + 2, Pd - A[dim], Pd - B[dim], p))

    def t1(dim, i, j):
        S = s1[dim]
        v = -2 * b * (2 * j + 1) * S[i][j] + 4 * b * b * S[i][j + 2]
        if j >= 2:
            v += j * (j - 1) * S[i][j - 2]
        return -v / 2

    ca, cb = cart_powers(la), cart_powers(lb)
    S = np.empty((len(ca), len(cb)), dtype=object)
    T = np.empty((len(ca), len(cb)), dtype=object)
    for ia, pa in enumerate(ca):
        for ib, pb in enumerate(cb):
            sx, sy, sz = (s1[dd][pa[dd]][pb[dd]] for dd in range(3))
            S[ia, ib] = pref * sx * sy * sz
            T[ia, ib] = pref * (t1(0, pa[0], pb[0]) * sy * sz + sx * t1(1, pa[1], pb[1]) * sz + sx * sy * t1(2, pa[2], pb[2]))
    return S, T


def _prim_nuc(la, lb, a, b, A, B, charges):
    """sum_c -Z_c <a| 1/|r - R_c| |b> over cart_powers(la) x cart_powers(lb), unnormalised primitives."""
    p = a + b
    P = [(a * A[i] + b * B[i]) / p for i in range(3)]
    AB2 = sum((A[i] - B[i]) ** 2 for i in range(3))
    pref = 2 * mp.pi / p * mp.exp(-a * b / p * AB2)
    ca, cb = cart_powers(la), cart_powers(lb)
    V = np.zeros((len(ca), len(cb)), dtype=object)
    for Rc, Zc in charges:
        PC = [P[i] - Rc[i] for i in range(3)]
        nodes, w = _rule(la + lb, p * sum(v * v for v in PC))
        for k, u in enumerate(nodes):
            t = []
            for dim in range(3):
                G = _g2d(la + lb, 0, (P[dim] - A[dim]) - PC[dim] * u, mpf(0), (1 - u) / (2 * p), mpf(0), mpf(0))
                t.append(_transfer(G, la, lb, 0, 0, A[dim] - B[dim], mpf(0)))
            f = -Zc * pref * w[k]
            for ia, pa in enumerate(ca):
                for ib, pb in enumerate(cb):
                    V[ia, ib] += f * t[0][pa[0]][pb[0]][0][0] * t[1][pa[1]][pb[1]][0][0] * t[2][pa[2]][pb[2]][0][0]
    return V


# ----------------------------------------------------------------------------------------------- contracted shells
@lru_cache(maxsize=None)
def _shell_transform_at(key, prec):
    """(2l+1, ncart) object array: fitted harmonic coefficients, each row scaled to unit self-overlap of the contracted
    function."""
    l, centre, exps, _ = key
    coefs = _prim_coefs_at(key, prec)
    Cm = np.array(sph_coeffs(l), dtype=object)
    A = _vec(centre)
    S = np.zeros((len(cart_powers(l)),) * 2, dtype=object)
    for a, ca in zip(exps, coefs):
        for b, cb in zip(exps, coefs):
            S = S + ca * cb * _prim_ovl_kin(l, l, mpf(a), mpf(b), A, A)[0]
    out = np.empty_like(Cm)
    for r in range(Cm.shape[0]):
        nrm = mp.fdot(Cm[r], S.dot(Cm[r]))
        out[r] = Cm[r] / mp.sqrt(nrm)
    return out


def shell_transform(sh):
    return _shell_transform_at(sh.key(), mp.prec)


@lru_cache(maxsize=None)
def _prim_coefs_at(key, prec):
    """The tabulated contraction coefficients multiply UNIT-NORMALISED primitives (the convention of every published
    basis set): coefficient / sqrt(self-overlap of the primitive), the self-overlap taken on the first component."""
    l, centre, exps, coefs = key
    c0 = np.array(sph_coeffs(l)[0], dtype=object)
    A = _vec(centre)
    return tuple(mpf(c) / mp.sqrt(mp.fdot(c0, _prim_ovl_kin(l, l, mpf(a), mpf(a), A, A)[0].dot(c0)))
                 for a, c in zip(exps, coefs))


def _prims(sh):
    """[(exponent, coefficient of the unnormalised primitive)] of a shell, before the shell's overall normalisation."""
    return list(zip((mpf(a) for a in sh.exps), _prim_coefs_at(sh.key(), mp.prec)))


def _index_arrays(ls):
    """All Cartesian component quartets of a shell class, as power index arrays [direction][shell]."""
    comps = list(product(*[range(len(cart_powers(l))) for l in ls]))
    pw = [cart_powers(l) for l in ls]
    idx = [[np.array([pw[s][c[s]][dim] for c in comps], dtype=np.intp) for s in range(4)] for dim in range(3)]
    return idx


@_work
def eri_quartet(shA, shB, shC, shD):
    """(ab|cd) over the spherical components of four contracted shells: object array (nA, nB, nC, nD) of mpf."""
    shs = (shA, shB, shC, shD)
    ls = [s.l for s in shs]
    cen = [_vec(s.centre) for s in shs]
    idx = _index_arrays(ls)
    nc = [len(cart_powers(l)) for l in ls]
    acc = np.zeros(nc[0] * nc[1] * nc[2] * nc[3], dtype=object)
    for (a, ca), (b, cb), (c, cc), (d, cd) in product(*[_prims(s) for s in shs]):
        X, Y, Z = _prim_eri_tables(*ls, a, b, c, d, *cen)
        f = ca * cb * cc * cd
        v = (X[(slice(None), *idx[0])] * Y[(slice(None), *idx[1])] * Z[(slice(None), *idx[2])]).sum(axis=0)
        acc = acc + f * v
    T = acc.reshape(nc)
    for axis, s in enumerate(shs):                      # Cartesian -> normalised real solid harmonics, one index at a time
        T = np.moveaxis(np.tensordot(shell_transform(s), T, axes=([1], [axis])), 0, axis)
    return T


@_work
def one_electron(shells, charges):
    """(S, T, V) over all spherical functions of `shells` (in order), V for point charges [((x, y, z), Z), ...]:
    object arrays (nao, nao) of mpf."""
    off = np.concatenate([[0], np.cumsum([s.nfun for s in shells])])
    n = int(off[-1])
    S, T, V = (np.zeros((n, n), dtype=object) for _ in range(3))
    chg = [(_vec(r), mpf(z)) for r, z in charges]
    for i, si in enumerate(shells):
        for j, sj in enumerate(shells[:i + 1]):
            A, B = _vec(si.centre), _vec(sj.centre)
            s = t = v = 0
            for a, ca in _prims(si):
                for b, cb in _prims(sj):
                    f = ca * cb
                    ps, pt = _prim_ovl_kin(si.l, sj.l, a, b, A, B)
                    s, t = s + f * ps, t + f * pt
                    v = v + f * _prim_nuc(si.l, sj.l, a, b, A, B, chg)
            Ci, Cj = shell_transform(si), shell_transform(sj)
            for M, blk in ((S, s), (T, t), (V, v)):
                sb = Ci.dot(blk).dot(Cj.T)
                M[off[i]:off[i + 1], off[j]:off[j + 1]] = sb
                M[off[j]:off[j + 1], off[i]:off[i + 1]] = sb.T
    return S, T, V


def to_double(arr):
    """Correctly rounded doubles of an object array of mpf."""
    return np.array([float(v) for v in np.asarray(arr, dtype=object).ravel()], dtype=np.float64).reshape(np.shape(arr))


# ----------------------------------------------------------------------------------------------- many quartets at once
_POOL_SHELLS = None


def _pool_init(shells, dps):
    global _POOL_SHELLS, DPS
    _POOL_SHELLS, DPS = shells, dps


def _pool_job(q):
    s = _POOL_SHELLS
    return to_double(eri_quartet(s[q[0]], s[q[1]], s[q[2]], s[q[3]]))


def eri_quartets(shells, quartets, workers=8):
    """[double array (nA, nB, nC, nD) for (A, B, C, D) in quartets], spread over at most 8 worker processes."""
    import multiprocessing
    quartets = [tuple(int(x) for x in q) for q in quartets]
    workers = max(1, min(8, workers, len(quartets)))
    if workers == 1:
        _pool_init(shells, DPS)
        return [_pool_job(q) for q in quartets]
    cost = lambda q: -math.prod(len(shells[i].exps) * len(cart_powers(shells[i].l)) for i in q)
    order = sorted(range(len(quartets)), key=lambda i: cost(quartets[i]))               # the expensive ones first
    with multiprocessing.get_context("fork").Pool(workers, initializer=_pool_init, initargs=(shells, DPS)) as pool:
        res = pool.map(_pool_job, [quartets[i] for i in order], chunksize=1)
    out = [None] * len(quartets)
    for i, r in zip(order, res):
        out[i] = r
    return out
