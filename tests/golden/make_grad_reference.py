"""Writes tests/golden/grad_ref_g1.npz, grad_ref_g2.npz, grad_ref_g3.npz: shell definitions (settings), fixed symmetric
matrices and the centre derivatives of the two-electron energy and of the one-electron traces, from
oracle/eri_reference.py (mpmath, 100 digits) rounded to double last.  Deterministic: running it again re-creates the
files byte for byte.  Measured: 4.5 minutes for the three families on eight cores (g1 0.6, g2 1.0, g3 2.9).

    python tests/golden/make_grad_reference.py [g1] [g2] [g3]

Every family is four shells, each alone on one of the four centres of the ERI reference's Z1 family, so that every
quartet with several shells of high angular momentum has them on DIFFERENT centres:
  g1: s p d f, 2 2 2 1 primitives   every bra and ket class, mixed L, the lmax = 3 layout
  g2: d d d d, 2 1 2 1 primitives   four-centre (dd|dd), the lmax = 2 layout
  g3: f f f f, single primitives    four-centre (ff|ff), L = 13 with the derivative

The derivative by the centre of shell s along axis k is the central difference  (E(+h) - E(-h)) / 2h,  h = 1e-30 bohr,
with the displaced centre carried as mpf (Shell.moved) and every sum formed in 100-digit arithmetic: the step error is
h^2 f''' / 6 f' ~ 1e-58, the cancellation leaves 70 digits.  Only the shell quartets (pairs) that contain s differ
between +h and -h; the others cancel exactly and are not computed.

Layout of the files (tests/grad_fixtures.py is the reader):
  centre (4, 3), l, nprim, exp, coef   raw shell definition, primitives concatenated in shell order
  charge_xyz, charge_z                 the point charges of V: Z1's charges on the four centres, NOT moved with the shells
  D, M, W (nao, nao)                   symmetric; D is grad2e_helper.random_density (seed 7), M seed 23, W seed 31
  c_hf (2,)                            0, 0.25
  g2e (2, 4, 3)                        d/dR_s of  1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum D_ac D_bd (ab|cd)
  g2e_spin (2, 4, 3)                   the same with (D_ac D_bd + M_ac M_bd) in the exchange part
  g1e (3, 4, 3)                        [-tr(W dS/dR_s), tr(D dT/dR_s), tr(D dV/dR_s) without the operator part]
  part_quartets (34, 4), part_values (34, 3)
                                       the coordinate (shell 0, x) once more, one unique shell quartet A >= B, C >= D,
                                       AB >= CD at a time: its share of d/dR of [J, K_D, K_M] = [sum D_ab D_cd (ab|cd),
                                       sum D_ac D_bd (ab|cd), sum M_ac M_bd (ab|cd)], summed over the quartet's whole
                                       orbit of index permutations; g2e = J / 2 - c_hf K_D / 4 summed over the parts.  So
                                       that a test can recompute stored values without paying for a whole coordinate.
  meta: JSON text: working digits, step, bound and the two self-checks --
        `step_check`: one coordinate (shell 2, y) done again at h = 1e-25; the largest relative change of the six stored
                      quantities, asserted <= 1e-40;
        `net_force`:  |sum over the shells| / max|row| of the two-electron derivatives (J, K_D, K_M) and of -tr(W dS),
                      tr(D dT) in 100-digit arithmetic, asserted <= 1e-30.
"""
import json
import math
import multiprocessing
import os
import sys
import time

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import eri_reference as R  # noqa: E402
from make_eri_reference import BOUND, Z1_CENTRES, Z1_CHARGES, Z1_SHELLS, definition, offsets, save, shell_pairs  # noqa: E402

C_HF = (0.0, 0.25)
STEP_EXP, STEP_CHECK_EXP = -30, -25
CHECK_COORD = (2, 1)                                 # shell, axis of the coordinate that is done again at the larger step
PART_COORD = (0, 0)                                  # shell, axis of the coordinate whose two-electron sum is also stored in parts
SEEDS = dict(D=7, M=23, W=31)

_S, _P, _D, _F = Z1_SHELLS[0][1][1:], Z1_SHELLS[1][1], Z1_SHELLS[2][1], Z1_SHELLS[3][1]
FAMILIES = {
    "g1": [(0, _S), (1, _P), (2, _D), (3, _F)],
    "g2": [(2, _D), (2, [(0.27, 1.0)]), (2, [(1.6, 0.5), (0.38, 0.6)]), (2, [(0.7, 1.0)])],
    "g3": [(3, [(0.9, 1.0)]), (3, [(0.55, 1.0)]), (3, [(1.4, 1.0)]), (3, [(0.33, 1.0)])],
}


def symmetric(nao, seed):
    """grad2e_helper.random_density."""
    a = np.random.default_rng(seed).standard_normal((nao, nao))
    return 0.1 * (a + a.T)


def family_shells(name):
    return [R.Shell(l, Z1_CENTRES[i], [e for e, _ in p], [c for _, c in p]) for i, (l, p) in enumerate(FAMILIES[name])]


# ----------------------------------------------------------------------------------------------- the jobs of the pool
_FAM = None


def _pool_init(fam, dps):
    global _FAM
    _FAM, R.DPS = fam, dps


def _exact(m):
    return np.array([[mpf(float(v)) for v in row] for row in m], dtype=object)


def _two_electron_job(s, axis, step, quartet):
    """[dJ, dK_D, dK_M] of one unique shell quartet A >= B, C >= D, AB >= CD: E(+step) - E(-step) with
    J = sum D_ab D_cd (ab|cd), K_X = sum X_ac X_bd (ab|cd), both summed over the whole orbit of the quartet under the
    eight index permutations (`deg` distinct members; K averages the two exchange pairings the orbit alternates between)."""
    shells, off, mats = _FAM["shells"], _FAM["off"], _FAM["mats"]
    A, B, C, D = quartet
    deg = (1 if A == B else 2) * (1 if C == D else 2) * (1 if (A, B) == (C, D) else 2)
    blk = lambda m, i, j: m[off[i]:off[i + 1], off[j]:off[j + 1]]
    with mp.workdps(R.DPS):
        T = None
        for sign in (1, -1):
            sh = list(shells)
            sh[s] = shells[s].moved(axis, sign * step)
            t = R.eri_quartet(sh[A], sh[B], sh[C], sh[D])
            T = t if T is None else T - t
        Dm = mats["D"]
        out = [deg * (np.tensordot(T, blk(Dm, C, D), axes=([2, 3], [0, 1])) * blk(Dm, A, B)).sum()]
        for X in (Dm, mats["M"]):
            k = (np.tensordot(T, blk(X, A, C), axes=([0, 2], [0, 1])) * blk(X, B, D)).sum()
            k = k + (np.tensordot(T, blk(X, A, D), axes=([0, 3], [0, 1])) * blk(X, B, C)).sum()
            out.append(deg * k / 2)
        return out


def _one_electron_job(s, axis, step):
    """[-tr(W dS), tr(D dT), tr(D dV)]: E(+step) - E(-step), the charges staying where they are."""
    shells, mats, charges = _FAM["shells"], _FAM["mats"], _FAM["charges"]
    with mp.workdps(R.DPS):
        tot = [mpf(0)] * 3
        for sign in (1, -1):
            sh = list(shells)
            sh[s] = shells[s].moved(axis, sign * step)
            S, T, V = R.one_electron(sh, charges)
            e = [-(mats["W"] * S).sum(), (mats["D"] * T).sum(), (mats["D"] * V).sum()]
            tot = [a + sign * b for a, b in zip(tot, e)]
        return tot


def _job(j):
    return _two_electron_job(*j[1:]) if j[0] == "2e" else _one_electron_job(*j[1:])


def _cost(fam, j):
    if j[0] == "1e":
        return 1
    return math.prod(len(fam["shells"][i].exps) * len(R.cart_powers(fam["shells"][i].l)) ** 2 for i in j[4])


# ----------------------------------------------------------------------------------------------- one family
def family(name):
    """What the jobs need of family `name`: shells, offsets, charges, the exact mpf images of D, M, W (and the doubles)."""
    shells = family_shells(name)
    off = offsets(shells)
    dbl = {k: symmetric(int(off[-1]), seed) for k, seed in SEEDS.items()}
    return dict(name=name, shells=shells, off=off, charges=list(zip(Z1_CENTRES, Z1_CHARGES)), dbl=dbl,
                mats={k: _exact(v) for k, v in dbl.items()})


def unique_quartets(nshell, s=None):
    """The shell quartets A >= B, C >= D, AB >= CD; with `s`, those that contain shell s."""
    pairs = shell_pairs(nshell)
    quartets = [(a, b, c, d) for i, (a, b) in enumerate(pairs) for (c, d) in pairs[:i + 1]]
    return quartets if s is None else [q for q in quartets if s in q]


def derivatives(fam, coords, workers=8, parts=None, only=None):
    """{(shell, axis, step exponent): [dJ, dK_D, dK_M, -tr(W dS), tr(D dT), tr(D dV)] by that coordinate, mpf}.
    `parts`: a dict that receives {the same key: [(quartet, [dJ, dK_D, dK_M] of that quartet alone), ...]}.
    `only`: the shell quartets to do (default: all that contain the shell); the sums are then partial."""
    shells = fam["shells"]
    with mp.workdps(R.DPS):
        steps = {e: mpf(10) ** e for _, _, e in coords}
    jobs, owner = [], []
    for s, k, e in coords:
        mine = [("1e", s, k, steps[e])] + [("2e", s, k, steps[e], q) for q in unique_quartets(len(shells), s)
                                           if only is None or q in only]
        jobs += mine
        owner += [(s, k, e)] * len(mine)
    order = sorted(range(len(jobs)), key=lambda i: -_cost(fam, jobs[i]))               # the expensive ones first
    if workers == 1:
        _pool_init(fam, R.DPS)
        res = [_job(jobs[i]) for i in order]
    else:
        with multiprocessing.get_context("fork").Pool(workers, initializer=_pool_init, initargs=(fam, R.DPS)) as pool:
            res = pool.map(_job, [jobs[i] for i in order], chunksize=1)
    done = dict(zip(order, res))
    out = {}
    with mp.workdps(R.DPS):
        for i, (j, key) in enumerate(zip(jobs, owner)):                                # summed in the order of `jobs`
            slot = out.setdefault(key, [mpf(0)] * 6)
            lo = 3 if j[0] == "1e" else 0
            for n, v in enumerate(done[i]):
                slot[lo + n] = slot[lo + n] + v / (2 * j[3])
            if parts is not None and j[0] == "2e":
                parts.setdefault(key, []).append((j[4], [v / (2 * j[3]) for v in done[i]]))
    return out


def stored_rows(q):
    """(g2e, g2e_spin, g1e) as the files hold them, from q[..., 6] = [dJ, dK_D, dK_M, -tr(W dS), tr(D dT), tr(D dV)]."""
    q = np.asarray(q, dtype=object)
    with mp.workdps(R.DPS):
        g2e = [q[..., 0] / 2 - mpf(c) / 4 * q[..., 1] for c in C_HF]
        g2e_spin = [q[..., 0] / 2 - mpf(c) / 4 * (q[..., 1] + q[..., 2]) for c in C_HF]
        g1e = [q[..., 3 + n] for n in range(3)]
        return tuple(R.to_double(np.array(a, dtype=object)) for a in (g2e, g2e_spin, g1e))


def make(name, workers=8):
    t0 = time.time()
    fam = family(name)
    shells = fam["shells"]
    coords = [(s, k, STEP_EXP) for s in range(len(shells)) for k in range(3)] + [(*CHECK_COORD, STEP_CHECK_EXP)]
    parts = {}
    deriv = derivatives(fam, coords, workers, parts)
    with mp.workdps(R.DPS):
        q = np.array([[deriv[(s, k, STEP_EXP)] for k in range(3)] for s in range(len(shells))], dtype=object)     # (4, 3, 6)
        again = deriv[(*CHECK_COORD, STEP_CHECK_EXP)]
        step_check = max(abs(a - b) / abs(b) for a, b in zip(again, q[CHECK_COORD]))
        assert step_check <= mpf(10) ** -40, step_check
        net = max(max(abs(v) for v in q[:, :, n].sum(axis=0)) / max(abs(v) for v in q[:, :, n].ravel()) for n in range(5))
        assert net <= mpf(10) ** -30, net
        g2e, g2e_spin, g1e = stored_rows(q)
        part = parts[(*PART_COORD, STEP_EXP)]
        meta = dict(dps=R.DPS, bound=BOUND, family=name, step=f"1e{STEP_EXP}", step_of_check=f"1e{STEP_CHECK_EXP}",
                    check_coordinate=list(CHECK_COORD), step_check=f"{float(step_check):.1e}", net_force=f"{float(net):.1e}",
                    part_coordinate=list(PART_COORD), seeds=SEEDS)
        save(os.path.join(HERE, f"grad_ref_{name}.npz"), meta, c_hf=np.array(C_HF), g2e=g2e, g2e_spin=g2e_spin, g1e=g1e,
             part_quartets=np.array([qt for qt, _ in part], dtype=np.int32),
             part_values=R.to_double(np.array([v for _, v in part], dtype=object)),
             **fam["dbl"], **definition(shells, fam["charges"]))
    print(f"{name}: {time.time() - t0:.0f} s, step check {float(step_check):.1e}, net force {float(net):.1e}", flush=True)


if __name__ == "__main__":
    for fam_name in sys.argv[1:] or list(FAMILIES):
        make(fam_name)
