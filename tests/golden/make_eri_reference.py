"""Writes tests/golden/eri_ref_z1.npz, eri_ref_z2.npz, eri_ref_z3.npz: shell definitions (settings) and the integrals
of oracle/eri_reference.py (mpmath, 100 digits) rounded to double.  Deterministic: running it again re-creates the
files byte for byte (fixed zip time stamps, no compression).  Takes a few minutes on eight cores.

    python tests/golden/make_eri_reference.py [z1] [z2] [z3]

Layout of the files (see tests/eri_fixtures.py for the reader):
  centre (nshell, 3), l, nprim, exp, coef   raw shell definition, primitives concatenated in shell order
  charge_xyz, charge_z                      point charges of V
  z1: eri_unique[IJ (IJ + 1) / 2 + KL], IJ = i (i + 1) / 2 + j >= KL, i >= j, k >= l: the whole tensor; S, T, V;
      check_quartets (n, 4), check_values: a few shell quartets computed a second time in another index order
  z2: R (6,), centres (6, 8, 3), ket_pairs (3, 2), cols (6, 65, 136): columns of the ket pairs on Y against the unique
      elements i (i + 1) / 2 + j of the 16 functions on X
  z3: ket_pairs (3, 2), cols (57, 703): columns of the ket pairs against all unique bra elements; S, T, V
  meta: JSON text (working digits, bound, measured fp64 floors where a family needed one)
"""
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import eri_reference as R  # noqa: E402

BOUND = 1e-12

Z1_CENTRES = [(0.10, -0.20, 0.05), (1.25, 0.90, 1.60), (-1.10, 0.70, -0.40), (0.30, -1.30, 1.20)]
Z1_SHELLS = [                                       # s p d f d p s; 3 2 2 1 1 3 2 primitives
    (0, [(60.0, 0.05), (4.1, 0.4), (0.35, 0.7)]),
    (1, [(7.3, 0.15), (0.62, 0.9)]),
    (2, [(2.9, 0.3), (0.45, 0.8)]),
    (3, [(0.9, 1.0)]),
    (2, [(0.27, 1.0)]),
    (1, [(22.0, 0.02), (1.7, -0.35), (0.12, 1.1)]),
    (0, [(1.3, 0.6), (0.19, -0.25)]),
]
Z1_CHARGES = [6.0, 1.0, 8.0, 7.0]                   # on the four centres

Z2_X = (0.10, -0.20, 0.05)
Z2_DIR = (0.36, 0.48, 0.80)                         # unit vector, no zero component
Z2_R = [0.0, 3e-7, 1.3, 5.0, 6.32, 40.0]                            # x = rho R^2, rho in [0.8, 1.25]
Z2_EXPS = [0.80, 0.95, 1.10, 1.25, 0.85, 1.00, 1.15, 1.20]          # X: s p d f, Y: s p d f
Z2_KETS = [(7, 7), (6, 5), (4, 4)]

Z3_XYZ = [(0.10, -0.20, 0.05), (1.25, 0.90, 1.60)]  # C, H of tests/test_integral_identities.py
Z3_KETS = [(10, 10), (9, 0), (14, 11)]              # (f_C, f_C), (last d_C, first s_C), (p_H, first s_H)


def save(path, meta, **arrays):
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
    print(path, os.path.getsize(path), "bytes")


def definition(shells, charges):
    return dict(centre=np.array([s.centre for s in shells]), l=np.array([s.l for s in shells], dtype=np.int32),
                nprim=np.array([len(s.exps) for s in shells], dtype=np.int32),
                exp=np.array([e for s in shells for e in s.exps]), coef=np.array([c for s in shells for c in s.coefs]),
                charge_xyz=np.array([r for r, _ in charges]).reshape(-1, 3), charge_z=np.array([z for _, z in charges]))


def offsets(shells):
    return np.concatenate([[0], np.cumsum([s.nfun for s in shells])]).astype(int)


def shell_pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1)]


def columns(shells, bra_shells, kets):
    """[(nC * nD, nbra (nbra + 1) / 2) per ket pair]: unique bra elements over the functions of `bra_shells`."""
    bras = [(bra_shells[a], bra_shells[b]) for a, b in shell_pairs(len(bra_shells))]
    quartets = [(a, b, c, d) for c, d in kets for a, b in bras]
    blocks = R.eri_quartets(shells, quartets)
    boff = offsets([shells[i] for i in bra_shells])
    pos = {s: i for i, s in enumerate(bra_shells)}
    nb = int(boff[-1])
    ti, tj = np.tril_indices(nb)
    out, it = [], iter(blocks)
    for c, d in kets:
        nq = shells[c].nfun * shells[d].nfun
        full = np.zeros((nb, nb, nq))
        for a, b in bras:
            blk = next(it).reshape(shells[a].nfun, shells[b].nfun, nq)
            full[boff[pos[a]]:boff[pos[a] + 1], boff[pos[b]]:boff[pos[b] + 1]] = blk
        out.append(full[ti, tj].T.copy())            # lower triangle: the blocks a >= b cover it (diagonal blocks whole)
    return out


def make_z1():
    shells = [R.Shell(l, Z1_CENTRES[i % 4], [e for e, _ in p], [c for _, c in p]) for i, (l, p) in enumerate(Z1_SHELLS)]
    charges = list(zip(Z1_CENTRES, Z1_CHARGES))
    pairs = shell_pairs(len(shells))
    quartets = [(a, b, c, d) for i, (a, b) in enumerate(pairs) for (c, d) in pairs[:i + 1]]
    check = [(1, 3, 2, 0), (0, 2, 3, 1), (4, 5, 3, 3), (3, 3, 6, 2)]   # stored as (3 1|2 0), (3 1|2 0)^T, (3 3|5 4), (6 2|3 3)
    blocks = R.eri_quartets(shells, quartets + check)
    off = offsets(shells)
    n = int(off[-1])
    eri = np.full((n, n, n, n), np.nan)
    for (a, b, c, d), blk in zip(quartets, blocks):
        sa, sb, sc, sd = (slice(off[i], off[i + 1]) for i in (a, b, c, d))
        eri[sa, sb, sc, sd] = blk                    # i >= j, k >= l, ij >= kl lies inside these two orders; the other six
        eri[sc, sd, sa, sb] = blk.transpose(2, 3, 0, 1)     # are never written (check_quartets computes some of them afresh)
    i, j = np.tril_indices(n)
    M = eri[i, j][:, i, j]                           # (npair, npair)
    I, K = np.tril_indices(len(i))
    unique = M[I, K]
    assert not np.isnan(unique).any()
    S, T, V = (R.to_double(m) for m in R.one_electron(shells, charges))
    meta = dict(dps=R.DPS, bound=BOUND, family="z1")
    save(os.path.join(HERE, "eri_ref_z1.npz"), meta, eri_unique=unique, S=S, T=T, V=V,
         check_quartets=np.array(check, dtype=np.int32),
         check_values=np.concatenate([b.ravel() for b in blocks[len(quartets):]]), **definition(shells, charges))


def z2_shells(Rsep):
    Y = tuple(x + Rsep * d for x, d in zip(Z2_X, Z2_DIR))
    return [R.Shell(i % 4, Z2_X if i < 4 else Y, [e], [1.0]) for i, e in enumerate(Z2_EXPS)]


def make_z2():
    cols, centres = [], []
    for Rsep in Z2_R:
        shells = z2_shells(Rsep)
        centres.append([s.centre for s in shells])
        cols.append(np.concatenate(columns(shells, [0, 1, 2, 3], Z2_KETS)))
        print("z2 R =", Rsep, "done", flush=True)
    d = definition(z2_shells(0.0), [])
    del d["centre"]
    meta = dict(dps=R.DPS, bound=BOUND, family="z2")
    save(os.path.join(HERE, "eri_ref_z2.npz"), meta, R=np.array(Z2_R), centres=np.array(centres),
         ket_pairs=np.array(Z2_KETS, dtype=np.int32), cols=np.array(cols), **d)


def make_z3():
    from quantum_compute_dft_amd import basis           # the shipped def2-TZVP table: exponents and coefficients only
    table = basis._BASIS_SETS["def2-tzvp"]
    shells = [R.Shell(l, xyz, [e for e, _ in p], [c for _, c in p])
              for sym, xyz in zip("CH", Z3_XYZ) for l, p in sorted(table[sym], key=lambda t: t[0])]
    assert [s.l for s in shells] == [0] * 5 + [1] * 3 + [2] * 2 + [3] + [0] * 3 + [1]
    charges = list(zip(Z3_XYZ, [6.0, 1.0]))
    cols = np.concatenate(columns(shells, list(range(len(shells))), Z3_KETS))
    S, T, V = (R.to_double(m) for m in R.one_electron(shells, charges))
    meta = dict(dps=R.DPS, bound=BOUND, family="z3")
    save(os.path.join(HERE, "eri_ref_z3.npz"), meta, ket_pairs=np.array(Z3_KETS, dtype=np.int32), cols=cols, S=S, T=T, V=V,
         **definition(shells, charges))


if __name__ == "__main__":
    which = sys.argv[1:] or ["z1", "z2", "z3"]
    for name in which:
        {"z1": make_z1, "z2": make_z2, "z3": make_z3}[name]()
