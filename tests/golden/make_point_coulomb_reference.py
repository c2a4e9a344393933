"""Writes tests/golden/point_coulomb_ref_z1.npz and point_coulomb_ref_z3.npz: the one-electron Coulomb integrals at
points, A[c, mu, nu] = <mu| 1/|r - R_c| |nu>, of oracle/eri_reference.py (mpmath, 100 digits; A = -V of a unit point
charge in one_electron) rounded to double.  The shell definitions are READ from eri_ref_z1.npz / eri_ref_z3.npz, not
restated.  Deterministic: running it again re-creates the files byte for byte.  About a minute on eight cores.

    python tests/golden/make_point_coulomb_reference.py [z1] [z3]

Layout (reader: tests/point_coulomb_fixtures.py):
  points (P, 3) bohr, A (P, nao, nao)
  meta: JSON text -- working digits, bound, and for z1 `boys_regimes`: how many (primitive pair, point) combinations
        fall into each regime of the Boys argument x = p |P - r|^2 (every one must be hit: asserted here)
"""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, HERE):
    if d not in sys.path:
        sys.path.insert(0, d)

from oracle import eri_reference as R  # noqa: E402
from make_eri_reference import BOUND, save  # noqa: E402

OFF_CENTRE = (3e-7, 0.0, 0.0)
Z1_EXTRA = [(0.4, -0.3, 0.7), (3.0, 2.0, -1.5), (12.0, -9.0, 7.0), (60.0, 45.0, -30.0),
            (-0.9, 0.5, -0.2), (0.7, 0.3, 0.9), (2.1, -1.7, 0.4), (-4.0, 5.0, 3.0)]
Z3_EXTRA = [(0.4, -0.3, 0.7), (3.0, 2.0, -1.5), (12.0, -9.0, 7.0), (60.0, 45.0, -30.0),
            (0.65, 0.35, 0.8), (-1.2, 0.4, -0.6), (1.9, 1.4, 2.4), (0.1, -0.2, 1.1)]
REGIMES = [("x == 0", lambda x: x == 0.0), ("0 < x < 1e-13", lambda x: (x > 0.0) & (x < 1e-13)),
           ("1e-13 <= x < 1", lambda x: (x >= 1e-13) & (x < 1.0)), ("1 <= x < 20", lambda x: (x >= 1.0) & (x < 20.0)),
           ("20 <= x < 40", lambda x: (x >= 20.0) & (x < 40.0)), ("40 <= x <= 50", lambda x: (x >= 40.0) & (x <= 50.0)),
           ("x > 1000", lambda x: x > 1000.0)]


def stored_shells(name):
    with np.load(os.path.join(HERE, name)) as z:
        centre, l, nprim, exp, coef = (z[k] for k in ("centre", "l", "nprim", "exp", "coef"))
    off = np.concatenate([[0], np.cumsum(nprim)])
    return [R.Shell(l[s], centre[s], exp[off[s]:off[s + 1]], coef[off[s]:off[s + 1]]) for s in range(len(l))]


def centres(shells):
    out = []
    for s in shells:
        if s.centre not in out:
            out.append(s.centre)
    return out


def points_of(shells, extra):
    cen = centres(shells)
    return np.array(cen + [tuple(x + d for x, d in zip(c, OFF_CENTRE)) for c in cen] + list(extra), dtype=np.float64)


def boys_arguments(shells, points):
    """x = p |P - r|^2 of every (primitive pair of a shell pair A >= B, point), in the engines' double arithmetic."""
    xs = []
    for i, si in enumerate(shells):
        for sj in shells[:i + 1]:
            A, B = np.array(si.centre), np.array(sj.centre)
            for a in si.exps:
                for b in sj.exps:
                    p = a + b
                    PC = (a * A + b * B) / p - points
                    xs.append(p * (PC[:, 0] * PC[:, 0] + PC[:, 1] * PC[:, 1] + PC[:, 2] * PC[:, 2]))
    return np.concatenate(xs)


_SHELLS = None


def _init(shells, dps):
    global _SHELLS
    _SHELLS, R.DPS = shells, dps


def _job(point):
    return -R.to_double(R.one_electron(_SHELLS, [(tuple(point), 1.0)])[2])


def make(family, source, extra, max_points, check_regimes):
    shells = stored_shells(source)
    pts = points_of(shells, extra)
    assert len(pts) <= max_points
    meta = dict(dps=R.DPS, bound=BOUND, family=family, shells_from=source)
    if check_regimes:
        x = boys_arguments(shells, pts)
        meta["boys_regimes"] = {name: int(sel(x).sum()) for name, sel in REGIMES}
        print(meta["boys_regimes"])
        assert all(n > 0 for n in meta["boys_regimes"].values()), "a regime of the Boys function is not hit: add points"
    with multiprocessing.Pool(min(8, len(pts)), _init, (shells, R.DPS)) as pool:
        A = np.array(pool.map(_job, [tuple(p) for p in pts], chunksize=1))
    save(os.path.join(HERE, f"point_coulomb_ref_{family}.npz"), meta, points=pts, A=A)


if __name__ == "__main__":
    for name in sys.argv[1:] or ["z1", "z3"]:
        {"z1": lambda: make("z1", "eri_ref_z1.npz", Z1_EXTRA, 32, True),
         "z3": lambda: make("z3", "eri_ref_z3.npz", Z3_EXTRA, 16, False)}[name]()
