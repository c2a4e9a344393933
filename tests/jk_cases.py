"""Case tables, input generators and CPU references for the dense and factorised J/K dispatch tests
(tests/test_jk_cases_cpu.py, tests/test_gpu_jk_dispatch.py).

Integer-exact inputs: every entry is a small integer held in a float64, so every product and every partial sum on the
device is an integer far below 2^53 (worst-case bounds: `dense_bounds`, `fact_bounds`) and ANY summation order on fp64
FMA / MFMA gives the same bits -- the GPU assertion is np.array_equal, there is no tolerance to choose.  Real-valued
inputs (the recipes of tests/test_gpu_parity.py) go with references in np.longdouble: small integers would also pass
through a reduced-precision path.

`expected_kernels(case)` restates, in Python, which template instantiations the dispatch of jk() and jk_factorized()
(csrc/dft_api.hip) reaches for a case, as far as that does not depend on the device's CU count.  The CPU suite holds
every instantiation in the compiler's resource report against these claims: a new instantiation needs a new case.
"""
import functools
import re
from collections import namedtuple

import numpy as np

JK_COLS = 1024        # csrc/jk_kernels.hpp: columns per workgroup of the streaming pass
SYM_MIN_N = 48        # csrc/dft_api.hip jk(): the symmetric-J kernels start here

# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
# kind "dense":      calls = J alone, K alone, J and K in one pass (whole matrix)
# kind "rows":       DFT_ComputeJKRows per rank of `world`: J and K together, J alone
# kind "sym":        J alone with option eri_symmetric = `sym`; `cpt` = QCDFT_JSYM8_CPT (None: unset, chosen from num_cu)
# kind "fact":       DFT_ComputeJKFactorized: J and K together (fused dot), J alone, K alone
# `dm_products` = 2: dm is the sum of two products cocc cocc^T, only the first from the orbitals handed over
# `aligned` = False: the ERI / the Cholesky vectors start 8 bytes into their allocation
Case = namedtuple("Case", "kind n naux nocc world sym cpt aligned ksplit dm_products note", defaults=(0, 0, 0, 0, None, True, 0, 1, ""))

DENSE_CASES = [
    Case("dense", 32, note="one exactly full block (KB = 32, 1024 columns)"),
    Case("dense", 33, note="first odd n with ncb = 2; the second block holds 2 k-segments"),
    Case("dense", 34, note="even n, ncb = 2"),
    Case("dense", 45, note="odd n, ncb = 3"),
    Case("dense", 64, note="KB = 16, every block exactly 1024 columns"),
    Case("dense", 65, note="KB = 15, 975 columns"),
    Case("dense", 102, note="jsplit = 1 with 11 column blocks on a 256-CU device; the ERI is 0.87 GB"),
]
DENSE_REAL_N = [33, 64, 65]
ROWS_CASES = [Case("rows", 33, world=2), Case("rows", 40, world=3), Case("rows", 57, world=8)]
UNALIGNED_DENSE = Case("dense", 34, aligned=False, note="ERI 8 bytes into its allocation: 8-byte loads with even n")
SYM_CASES = ([Case("sym", n, sym=1) for n in (48, 49)] +
             [Case("sym", n, sym=2, cpt=cpt) for n in (48, 49, 57) for cpt in (1, 2, 4, None)])

FACT_CASES = [
    Case("fact", 5, 3, 2, note="one contraction stage"),
    Case("fact", 12, 4, 3, note="two stages"),
    Case("fact", 19, 3, 5, note="three stages, odd"),
    Case("fact", 40, 7, 16),
    Case("fact", 41, 7, 17),
    Case("fact", 64, 5, 32),
    Case("fact", 67, 5, 33),
    Case("fact", 70, 4, 48),
    Case("fact", 71, 4, 49),
    Case("fact", 72, 4, 64),
    Case("fact", 75, 4, 65),
    Case("fact", 96, 6, 56, note="MI = 4, even"),
    Case("fact", 97, 6, 57, note="MI = 4, odd"),
    Case("fact", 140, 3, 128),
    Case("fact", 141, 3, 129, note="two 128-row tiles"),
    Case("fact", 258, 2, 9),
    Case("fact", 259, 2, 70, note="second column block, mirrored K tile, odd"),
]
FACT_REAL = [(96, 6, 56), (97, 6, 57), (141, 3, 129), (259, 2, 70)]
FACT_MIXED_DM = Case("fact", 97, 6, 57, dm_products=2, note="dm = sum of two integer products: J follows dm, K the orbitals")
UNALIGNED_FACT = Case("fact", 96, 6, 56, aligned=False, note="L 8 bytes into its allocation")
KSPLIT_CASES = [Case("fact", 97, 6, 57, ksplit=1), Case("fact", 97, 6, 57, ksplit=2), Case("fact", 97, 6, 57, ksplit=5),
                Case("fact", 19, 3, 5, ksplit=3, note="24 chunks of 16 rows for 15 rows of Yt: all but one are empty")]

ALL_CASES = DENSE_CASES + ROWS_CASES + [UNALIGNED_DENSE] + SYM_CASES + FACT_CASES + [FACT_MIXED_DM, UNALIGNED_FACT] + KSPLIT_CASES


def case_id(c):
    s = f"{c.kind}-n{c.n}"
    if c.kind == "fact":
        s += f"-naux{c.naux}-nocc{c.nocc}"
    if c.world:
        s += f"-world{c.world}"
    if c.sym:
        s += f"-sym{c.sym}-cpt{c.cpt if c.cpt else 'auto'}"
    if not c.aligned:
        s += "-unaligned"
    if c.ksplit:
        s += f"-ksplit{c.ksplit}"
    if c.dm_products != 1:
        s += f"-dm{c.dm_products}products"
    return s


# ---------------------------------------------------------------------------------------------------------------------
# dispatch, restated
# ---------------------------------------------------------------------------------------------------------------------
def dense_blocks(n):
    """(KB, ncb, k-segments of the last block): column blocks of the dense streaming pass, as jk() cuts them."""
    KB = max(1, min(n, JK_COLS // n))
    ncb = -(-n // KB)
    return KB, ncb, n - (ncb - 1) * KB


def dense_jsplit(n, ni, num_cu):
    """j-range split of the streaming pass on a device of `num_cu` compute units (jk(): ni rows of i)."""
    ncb = dense_blocks(n)[1]
    jsplit = 1
    while ni * ncb * jsplit < 4 * num_cu and jsplit * 2 <= n:
        jsplit *= 2
    return jsplit


def half_transform_tier(nocc):
    """(WGM, MI, NW, BK, NJ) of the half transform k_gemm_tn<WGM, MI, true, VECB, DOT, NW, BK, NJ>."""
    if nocc <= 16:
        return 1, 1, 4, 8, 4
    if nocc <= 32:
        return 1, 2, 4, 8, 4
    if nocc <= 48:
        return 1, 3, 4, 8, 4
    if nocc <= 64:
        return 1, 4, 4, 8, 4
    return 2, 4, 8, 0, 0


def half_transform_stages(nao, nocc):
    """Stages of the half transform's double-buffered contraction loop (contraction length nao, BK rows a stage)."""
    bk = half_transform_tier(nocc)[3] or 16
    return -(-nao // bk)


def expected_kernels(c):
    """Set of (kernel name, template arguments) the calls of case `c` launch, CU-count independent part."""
    out = set()
    if c.kind in ("dense", "rows", "sym"):
        vec = c.n % 2 == 0 and c.aligned
        if c.kind == "sym" and c.n >= SYM_MIN_N:
            if c.sym == 2:
                if c.cpt:
                    out.add(("k_j_sym8", (c.cpt,)))
            else:
                out.add(("k_j_sym", (vec,)))
        elif c.kind == "sym":
            out.add(("k_jk_stream", (True, False, vec)))
        elif c.kind == "rows":
            out |= {("k_jk_stream", (True, True, vec)), ("k_jk_stream", (True, False, vec))}
        else:
            out |= {("k_jk_stream", (True, False, vec)), ("k_jk_stream", (False, True, vec)), ("k_jk_stream", (True, True, vec))}
    elif c.kind == "fact":
        vecl = c.n % 2 == 0 and c.aligned
        wgm, mi, nw, bk, nj = half_transform_tier(c.nocc)
        for dot in (True, False):                                   # J and K together; K alone (J alone runs no GEMM)
            out.add(("k_gemm_tn", (wgm, mi, True, vecl, dot, nw, bk, nj)))
        out.add(("k_gemm_tn", (2, 4, True, True, False, 8, 0, 0)))   # K = Yt^T Yt
    else:
        raise ValueError(c.kind)
    return out


LEDGER_KERNELS = ("k_gemm_tn", "k_jk_stream", "k_j_sym", "k_j_sym8")


def parse_instantiation(demangled, kernels=LEDGER_KERNELS):
    """(kernel name, template arguments) of a demangled kernel name of the resource report, None for kernels outside
    `kernels` (tests/sweep_cases.py hands over its own families)."""
    m = re.match(r"void qcdft::(\w+)<([^>]*)>\(", demangled)
    if not m or m.group(1) not in kernels:
        return None
    conv = lambda s: True if s == "true" else False if s == "false" else int(s)
    return m.group(1), tuple(conv(a.strip()) for a in m.group(2).split(","))


# ---------------------------------------------------------------------------------------------------------------------
# worst-case magnitudes of the integer cases
# ---------------------------------------------------------------------------------------------------------------------
ERI_MAX, DM_MAX, L_MAX, C_MAX = 8, 4, 3, 2


def dense_bounds(n):
    """Largest |value| any intermediate of the dense passes can take: products, column / row / slab partials, J, K."""
    prod = ERI_MAX * DM_MAX
    full = n * n * prod                      # J[c] and K[i][k] sum n^2 products; every partial sums a subset of them
    sym8 = n * n * ERI_MAX * 2 * DM_MAX      # k_j_sym8 folds the factor 2 of an off-diagonal pair into dm
    return {"product": 2 * prod, "partial": full, "J": full, "K": full, "J_sym8": sym8}


def fact_bounds(nao, naux, nocc, dm_products=1):
    """Same for the factorised path; dm = sum of `dm_products` integer products cocc cocc^T."""
    dm = dm_products * nocc * C_MAX * C_MAX              # |dm| entries (also k_dm_consistency's sums)
    yt = nao * C_MAX * L_MAX                             # Yt_P[i][b] = sum_nu cocc[nu][i] L_P[nu][b]
    fused = nocc * nao * yt * C_MAX                      # v_P = sum_{i,b} Yt_P[i][b] cocc[b][i] (tile partials are subsets)
    dot = nao * nao * L_MAX * dm                         # v_P = L_P : dm (k_cd_dot, k_cd_dot_if)
    v = max(fused, dot)
    return {"dm": dm, "Yt": yt, "fused_dot": fused, "dot": dot,
            "J": naux * v * L_MAX,                       # J = sum_P v_P L_P (slices of P are subsets)
            "K": naux * nocc * yt * yt}                  # K = Yt^T Yt (slabs are subsets of the (P, i) rows)


# ---------------------------------------------------------------------------------------------------------------------
# generators and references
# ---------------------------------------------------------------------------------------------------------------------
def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape, dtype=np.int8).astype(np.float64)


def dense_reference(eri, dm, dtype=np.float64):
    """J = eri^T . vec(dm), K = einsum('ijkl,jl->ik') in `dtype` (plain numpy)."""
    n = dm.shape[0]
    e, d = eri.astype(dtype, copy=False), dm.astype(dtype, copy=False)
    J = (d.reshape(1, -1) @ e).reshape(n, n)
    K = np.einsum("ijkl,jl->ik", e.reshape(n, n, n, n), d)
    return J, K


def factor_reference(chol, dm, dtype=np.float64):
    """J = sum_P (L_P : dm) L_P, K = sum_P L_P dm L_P in `dtype` (plain numpy)."""
    L, d = chol.astype(dtype, copy=False), dm.astype(dtype, copy=False)
    v = (L * d[None]).sum(axis=(1, 2))
    J = (v[:, None, None] * L).sum(axis=0)
    K = np.zeros_like(d)
    for P in range(L.shape[0]):
        K += L[P] @ d @ L[P]
    return J, K


@functools.lru_cache(maxsize=None)
def dense_int_case(n):
    """(eri, dm, J, K): integer ERI in [-8, 8] (NOT symmetric: pins which index is contracted), dm in [-4, 4]."""
    rng = np.random.default_rng(7000 + n)
    eri = _ints(rng, -ERI_MAX, ERI_MAX, (n * n, n * n))
    dm = _ints(rng, -DM_MAX, DM_MAX, (n, n))
    return (eri, dm) + dense_reference(eri, dm)


@functools.lru_cache(maxsize=None)
def dense_real_case(n):
    """(eri, dm, J, K): the standard-normal recipe of test_coulomb_and_exchange_match_oracle, longdouble reference."""
    rng = np.random.default_rng(100 + n)
    eri = rng.standard_normal((n * n, n * n))
    dm = rng.standard_normal((n, n))
    return (eri, dm) + dense_reference(eri, dm, np.longdouble)


def pair_index(n):
    """Packed index P(i, j) = a (a + 1) / 2 + b, a = max, b = min, of every (i, j), flattened."""
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b = np.maximum(ii, jj), np.minimum(ii, jj)
    return (a * (a + 1) // 2 + b).reshape(-1), (ii >= jj).reshape(-1)


@functools.lru_cache(maxsize=None)
def sym_int_case(n, sym):
    """(eri, dm, J): sym = 1: ERI symmetric as an (n^2, n^2) matrix, dm general; sym = 2: eight-fold symmetric ERI,
    dm = dm^T (what k_j_sym8 requires).  Entries in [-8, 8] and [-4, 4]."""
    rng = np.random.default_rng(7100 + 10 * n + sym)
    if sym == 1:
        A = _ints(rng, -ERI_MAX // 2, ERI_MAX // 2, (n * n, n * n))
        eri = A + A.T
        dm = _ints(rng, -DM_MAX, DM_MAX, (n, n))
    else:
        npk = n * (n + 1) // 2
        G = _ints(rng, -ERI_MAX // 2, ERI_MAX // 2, (npk, npk))
        G = G + G.T
        P, _ = pair_index(n)
        eri = np.ascontiguousarray(G[P][:, P])
        B = _ints(rng, -DM_MAX // 2, DM_MAX // 2, (n, n))
        dm = B + B.T
    return eri, dm, dense_reference(eri, dm)[0]


def sym_read_mask(n, sym):
    """Boolean (n^2, n^2): the ERI elements the symmetric-J kernels may read."""
    N2 = n * n
    if sym == 1:
        return np.triu(np.ones((N2, N2), dtype=bool))
    P, low = pair_index(n)
    return low[:, None] & low[None, :] & (P[None, :] <= P[:, None])


def _int_factors(rng, nao, naux, nocc):
    A = _ints(rng, -L_MAX, L_MAX, (naux, nao, nao))
    chol = np.triu(A) + np.triu(A, 1).transpose(0, 2, 1)            # symmetric, entries in [-3, 3]
    cocc = _ints(rng, -C_MAX, C_MAX, (nao, nocc))
    return chol, cocc


@functools.lru_cache(maxsize=None)
def fact_int_case(nao, naux, nocc):
    """(chol, cocc, dm, J, K): symmetric integer L_P, integer cocc, dm = cocc cocc^T (exact)."""
    chol, cocc = _int_factors(np.random.default_rng(7200 + 1000 * nao + nocc), nao, naux, nocc)
    dm = cocc @ cocc.T
    return (chol, cocc, dm) + factor_reference(chol, dm)


@functools.lru_cache(maxsize=None)
def fact_mixed_dm_case(nao, naux, nocc):
    """(chol, cocc, dm, J, K): dm = cocc cocc^T + c2 c2^T is NOT the product of the orbitals handed over: J is the
    Coulomb matrix of dm, K the exchange matrix of cocc cocc^T."""
    rng = np.random.default_rng(7300 + 1000 * nao + nocc)
    chol, cocc = _int_factors(rng, nao, naux, nocc)
    c2 = _ints(rng, -C_MAX, C_MAX, (nao, nocc))
    dm = cocc @ cocc.T + c2 @ c2.T
    return chol, cocc, dm, factor_reference(chol, dm)[0], factor_reference(chol, cocc @ cocc.T)[1]


@functools.lru_cache(maxsize=None)
def fact_real_case(nao, naux, nocc):
    """(chol, cocc, dm, J, K): the recipe of test_gpu_parity._factor_case; longdouble reference from cocc cocc^T
    taken in longdouble as well (the device never sees the rounded dm on the K side)."""
    rng = np.random.default_rng(100 + nao)
    A = rng.normal(0, 0.3, (naux, nao, nao))
    chol = 0.5 * (A + A.transpose(0, 2, 1))
    cocc = rng.normal(0, 0.7, (nao, nocc))
    cl = cocc.astype(np.longdouble)
    return (chol, cocc, cocc @ cocc.T) + factor_reference(chol, cl @ cl.T, np.longdouble)


def clear_caches():
    for f in (dense_int_case, dense_real_case, sym_int_case, fact_int_case, fact_mixed_dm_case, fact_real_case):
        f.cache_clear()
