"""numpy restatement of the device factorisation of a density matrix (csrc/dm_factor.hip) and of its acceptance bound
(k_dm_consistency, csrc/cd_kernels.hpp).  A test helper: the product never imports it.

Left-looking pivoted Cholesky: per step the pivot is the largest residual diagonal entry (the lowest index among
equals), the loop stops when that entry is <= tol * max_i dm_ii and fails when it would take more than max_rank steps;
afterwards a residual diagonal entry below -10 tol scale marks an indefinite matrix.  Acceptance is element-wise
|dm - L L^T| <= 1e-11 (|L| |L|^T + |dm|) + 1e-14 over the whole matrix."""
import numpy as np

OK, RANK_EXCEEDED, NOT_PSD, INCONSISTENT, SIZE = 0, 1, 2, 3, 4
MIN_NAO, MAX_NAO = 2, 8192


def consistency_bound(dm, L):
    return 1e-11 * (np.abs(L) @ np.abs(L).T + np.abs(dm)) + 1e-14


def consistent(dm, L):
    """The acceptance rule; False for a dm holding a NaN or an infinity."""
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.isfinite(dm)) and np.all(np.abs(dm - L @ L.T) <= consistency_bound(dm, L)))


def pivoted_cholesky(dm, max_rank=None, tol=None):
    """(L (nao, rank) or None, info) with info = dict(rank=steps taken, resid=last residual maximum / scale, reason,
    scale, pivots)."""
    dm = np.asarray(dm, dtype=np.float64)
    nao = dm.shape[0]
    info = dict(rank=0, resid=0.0, reason=SIZE, scale=0.0, pivots=[])
    if nao < MIN_NAO or nao > MAX_NAO:
        return None, info
    max_rank = min(nao, max_rank) if max_rank and max_rank > 0 else nao // 2
    tol = tol if tol and tol > 0 else 1e-13
    d = np.diag(dm).copy()
    Lt = np.zeros((max_rank, nao))                      # the factor transposed, as the kernel keeps it

    def argmax(v):                                      # NaN never wins; the lowest index among equals
        v = np.where(np.isnan(v), -np.inf, v)
        at = int(np.argmax(v))                          # first occurrence of the maximum
        return (v[at], at) if v[at] > -np.inf else (-np.inf, nao)

    k = 0
    while True:
        gv, p = argmax(d)
        if k == 0:
            info["scale"] = scale = gv
            if not (scale > 0.0) or not (scale < np.inf):
                info["reason"] = NOT_PSD
                return None, info
        info["rank"], info["resid"] = k, gv / scale
        if gv <= tol * scale:
            break
        if k == max_rank:
            info["reason"] = RANK_EXCEEDED
            return None, info
        with np.errstate(invalid="ignore", over="ignore"):
            col = (dm[p, :] - Lt[:k].T @ Lt[:k, p]) / np.sqrt(gv)
            Lt[k] = col
            d = d - col * col
        d[p] = 0.0
        info["pivots"].append(p)
        k += 1
    if k == 0 or not np.all(d >= -10.0 * tol * scale):
        info["reason"] = NOT_PSD
        return None, info
    L = np.ascontiguousarray(Lt[:k].T)
    if not consistent(dm, L):
        info["reason"] = INCONSISTENT
        return None, info
    info["reason"] = OK
    return L, info


def occ_inputs(ngrid, nao, nocc, seed):
    """The recipe of tests/test_gpu_occ.py (SURVEY 8(d) with the orbitals kept), restated: that file is a test module."""
    rng = np.random.default_rng(seed)
    ao = 0.4 * rng.standard_normal((ngrid, nao))
    gr = 0.3 * rng.standard_normal((3, ngrid, nao))
    w = 0.05 * rng.random(ngrid)
    cocc = np.sqrt(2.0) * 0.7 * rng.standard_normal((nao, nocc))
    return cocc, cocc @ cocc.T, ao, gr, w


def s_orthonormal_density(nao, nocc, cond, seed):
    """dm = 2 C C^T with C^T S C = 1 for an overlap matrix S of condition number `cond` (eigenvalues spread
    geometrically from 1 / cond to 1): what a closed-shell SCF loop in a nearly dependent basis hands over."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((nao, nao)))
    ev = np.logspace(-np.log10(cond), 0.0, nao)
    X = (Q / np.sqrt(ev)) @ Q.T                         # S^(-1/2)
    U, _ = np.linalg.qr(rng.standard_normal((nao, nocc)))
    C = X @ U
    dm = 2.0 * C @ C.T
    return 0.5 * (dm + dm.T), np.sqrt(2.0) * C


# shapes (nao, nocc) of the factor tests: one lane up to more rows than any workgroup holds (1030 > 1024)
FACTOR_SHAPES = [(2, 1), (13, 3), (65, 13), (129, 26), (257, 65), (494, 47), (610, 250), (1030, 40)]


def factor_case(nao, nocc):
    cocc, dm, *_ = occ_inputs(1, nao, nocc, seed=9100 + nao + nocc)
    return cocc, dm
