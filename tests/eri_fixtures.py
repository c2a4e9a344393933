"""Reader of tests/golden/eri_ref_*.npz (written by tests/golden/make_eri_reference.py from oracle/eri_reference.py):
shell definitions turned into a basis.ShellTable WITHOUT build_shells (which re-sorts shells by l), reference values
unpacked to the layouts the engines return.  Needs neither mpmath nor the oracle package."""
import functools
import json
import os

import numpy as np

from quantum_compute_dft_amd import basis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Bound of every comparison with the fixtures: |got - ref| <= BOUND * max(1, max|ref| of the column block).  The host
# engine meets it with a factor 40 to spare in every family (profiles/eri_reference_parity.txt), so no family needed a
# measured fp64 floor; the device engine is held to the same bound.
BOUND = 1e-12


def shell_table(centre, l, nprim, exp, coef):
    """basis.ShellTable straight from a stored definition; the contraction goes through basis.normalized_coefficients."""
    l, nprim = np.asarray(l, dtype=np.int32), np.asarray(nprim, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(nprim)[:-1]]).astype(np.int32)
    nf = 2 * l + 1
    ao = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int32)
    c = np.concatenate([basis.normalized_coefficients(int(ll), exp[o:o + n], coef[o:o + n]) for ll, o, n in zip(l, off, nprim)])
    _, atom = np.unique(np.asarray(centre), axis=0, return_inverse=True)
    return basis.ShellTable(np.ascontiguousarray(centre, dtype=np.float64), l, nprim, off, ao, np.array(exp, dtype=np.float64),
                            c, np.asarray(atom, dtype=np.int32).ravel(), int(nf.sum()))


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(d["meta"].tobytes().decode())
    return d


def symbols(charge_z):
    return [basis.ELEMENTS[int(z)] for z in charge_z]


def shell_lower_mask(sh, nfun=None):
    """(n, n) bool: what the engines write with lower_only / on the device -- the shell blocks A >= B, the diagonal
    blocks whole.  That contains every element i >= j (all the consumer reads, cholesky.py takes tril); elements i < j
    of a diagonal shell block hold the mirrored value, every block A < B stays zero."""
    owner = np.repeat(np.arange(sh.nshell), 2 * np.asarray(sh.l) + 1)[:nfun]
    return owner[:, None] >= owner[None, :]


def lower_to_full(cols, sh, n):
    """(nq, n (n + 1) / 2) unique bra elements over the first n functions -> (nq, n, n) in the engines' layout."""
    i, j = np.tril_indices(n)
    out = np.zeros((cols.shape[0], n, n))
    out[:, i, j] = cols
    out[:, j, i] = cols
    return out * shell_lower_mask(sh, n)


@functools.lru_cache(maxsize=None)
def z1():
    """dict: sh, syms, charge_xyz, S, T, V, eri (the dense (25,)*4 tensor rebuilt from the unique elements), raw (file)."""
    d = _load("eri_ref_z1.npz")
    sh = shell_table(d["centre"], d["l"], d["nprim"], d["exp"], d["coef"])
    n = sh.nao
    i, j = np.tril_indices(n)
    I, K = np.tril_indices(len(i))
    M = np.zeros((len(i), len(i)))
    M[I, K] = d["eri_unique"]
    M = M + np.tril(M, -1).T
    eri = np.zeros((n, n, n, n))
    eri[i[:, None], j[:, None], i[None, :], j[None, :]] = M
    eri[j[:, None], i[:, None], i[None, :], j[None, :]] = M
    eri[i[:, None], j[:, None], j[None, :], i[None, :]] = M
    eri[j[:, None], i[:, None], j[None, :], i[None, :]] = M
    return dict(sh=sh, syms=symbols(d["charge_z"]), charge_xyz=d["charge_xyz"], S=d["S"], T=d["T"], V=d["V"], eri=eri, raw=d)


def z1_columns(C, D):
    """Reference columns of ket shell pair (C, D) of Z1 in the engines' layout (nq, 25, 25), see shell_lower_mask."""
    f = z1()
    sh, eri = f["sh"], f["eri"]
    c0, d0, nc, nd = int(sh.ao[C]), int(sh.ao[D]), 2 * int(sh.l[C]) + 1, 2 * int(sh.l[D]) + 1
    blk = eri[:, :, c0:c0 + nc, d0:d0 + nd].reshape(sh.nao, sh.nao, nc * nd).transpose(2, 0, 1)
    return blk * shell_lower_mask(sh)


@functools.lru_cache(maxsize=None)
def z2():
    """list of 6 dicts (R = 0, 3e-7, 1.3, 5, 6.32, 40): R, sh (8 shells, 32 functions), kets [(C, D)], cols [(nq, 16, 16) over X per ket, engines' layout]."""
    d = _load("eri_ref_z2.npz")
    out = []
    for g, R in enumerate(d["R"]):
        sh = shell_table(d["centres"][g], d["l"], d["nprim"], d["exp"], d["coef"])
        kets = [tuple(int(x) for x in k) for k in d["ket_pairs"]]
        full = lower_to_full(d["cols"][g], sh, 16)
        nqs = [(2 * int(sh.l[C]) + 1) * (2 * int(sh.l[D]) + 1) for C, D in kets]
        o = np.concatenate([[0], np.cumsum(nqs)])
        out.append(dict(R=float(R), sh=sh, kets=kets, cols=[full[o[k]:o[k + 1]] for k in range(len(kets))], raw=d))
    return out


@functools.lru_cache(maxsize=None)
def z3():
    """dict: sh (C-H, def2-TZVP, 37 functions), syms, charge_xyz, S, T, V, kets, cols [(nq, 37, 37) per ket, engines' layout]."""
    d = _load("eri_ref_z3.npz")
    sh = shell_table(d["centre"], d["l"], d["nprim"], d["exp"], d["coef"])
    kets = [tuple(int(x) for x in k) for k in d["ket_pairs"]]
    full = lower_to_full(d["cols"], sh, sh.nao)
    nqs = [(2 * int(sh.l[C]) + 1) * (2 * int(sh.l[D]) + 1) for C, D in kets]
    o = np.concatenate([[0], np.cumsum(nqs)])
    return dict(sh=sh, syms=symbols(d["charge_z"]), charge_xyz=d["charge_xyz"], S=d["S"], T=d["T"], V=d["V"], kets=kets,
                cols=[full[o[k]:o[k + 1]] for k in range(len(kets))], raw=d)


def swapped(cols, nc, nd):
    """Columns of (C, D), rows k * nd + l  ->  columns of (D, C), rows l * nc + k."""
    return cols.reshape(nc, nd, *cols.shape[1:]).swapaxes(0, 1).reshape(cols.shape)


def within(got, ref, bound=BOUND):
    """(ok, error, allowed) of one column block."""
    err = float(np.abs(got - ref).max())
    allowed = bound * max(1.0, float(np.abs(ref).max()))
    return err <= allowed, err, allowed
