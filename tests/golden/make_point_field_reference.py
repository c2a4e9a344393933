"""Writes tests/golden/point_field_ref_z1.npz and point_field_ref_z3.npz: the derivative of the one-electron Coulomb
integrals at a point with respect to that point, dA[c, k, mu, nu] = d/dR_c,k <mu| 1/|r - R_c| |nu>, k = x, y, z, at
every point of point_coulomb_ref_z1.npz / point_coulomb_ref_z3.npz.  oracle/eri_reference.py (mpmath, 100 digits) has no
derivative: dA is the central difference of A = -V of a unit point charge (one_electron) with h = 1e-30 in the same
100-digit arithmetic (truncation h^2 ~ 1e-60, cancellation 1e-100 / h = 1e-70), rounded to double.  Every stored
(point, direction) is computed a second time with h = 1e-20 and the two must agree below 1e-35 (asserted).  The shell
definitions are READ from eri_ref_z1.npz / eri_ref_z3.npz and the points from the potential's files, not restated.
Deterministic: running it again re-creates the files byte for byte.  About five minutes on eight cores.

    python tests/golden/make_point_field_reference.py [z1] [z3]

Layout (reader: tests/point_field_fixtures.py):
  points (P, 3) bohr, point_index (P,) into the points of point_coulomb_ref_<family>.npz, dA (P, 3, nao, nao)
  meta: JSON text -- working digits, bound, the two steps, the largest disagreement between them, and for z1
        `boys_regimes` as in the potential's file (every regime must be hit: asserted here)
"""
import multiprocessing
import os
import sys

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for d in (ROOT, HERE):
    if d not in sys.path:
        sys.path.insert(0, d)

from oracle import eri_reference as R  # noqa: E402
from make_eri_reference import BOUND, save  # noqa: E402
from make_point_coulomb_reference import REGIMES, boys_arguments, stored_shells  # noqa: E402

H, H_CHECK, AGREE = "1e-30", "1e-20", "1e-35"
LARGEST_FIXTURE = 452154            # eri_ref_z1.npz: no new file may be larger


def potential_integrals(shells, point):
    """A[mu, nu] at `point` (three mpf): object array of mpf."""
    return -R.one_electron(shells, [(tuple(point), 1)])[2]


def derivative(shells, point, k, h=H):
    """dA[mu, nu] / d point[k] as an object array of mpf: central difference with step `h` (text).  The oracle raises
    the precision inside its own functions only, so the displaced point and the difference are formed here at R.DPS
    digits -- at the default 15 the step would vanish in point + h."""
    with mp.workdps(R.DPS):
        h = mpf(h)
        up, dn = [mpf(float(x)) for x in point], [mpf(float(x)) for x in point]
        up[k] += h
        dn[k] -= h
        return (potential_integrals(shells, up) - potential_integrals(shells, dn)) / (2 * h)


def derivative_double(shells, point, k):
    """What the files store for one (point, direction): (nao, nao) doubles."""
    return R.to_double(derivative(shells, point, k))


_SHELLS = None


def _init(shells, dps):
    global _SHELLS
    _SHELLS, R.DPS = shells, dps


def _job(arg):
    point, k = arg
    with mp.workdps(R.DPS):
        d = derivative(_SHELLS, point, k)
        diff = max(abs(v) for v in (d - derivative(_SHELLS, point, k, H_CHECK)).ravel())
        assert diff < mpf(AGREE), (point, k, diff)
        return R.to_double(d), float(diff)


def make(family, source, check_regimes):
    shells = stored_shells(source)
    with np.load(os.path.join(HERE, f"point_coulomb_ref_{family}.npz")) as z:
        all_pts = z["points"]
    index = np.arange(len(all_pts))                          # every point of the potential's file is kept
    pts = all_pts[index]
    meta = dict(dps=R.DPS, bound=BOUND, family=family, shells_from=source, points_from=f"point_coulomb_ref_{family}.npz",
                h=H, h_check=H_CHECK, agree=AGREE)
    if check_regimes:
        x = boys_arguments(shells, pts)
        meta["boys_regimes"] = {name: int(sel(x).sum()) for name, sel in REGIMES}
        print(meta["boys_regimes"])
        assert all(n > 0 for n in meta["boys_regimes"].values()), "a regime of the Boys function is not hit: add points"
    jobs = [(tuple(p), k) for p in pts for k in range(3)]
    with multiprocessing.Pool(min(8, len(jobs)), _init, (shells, R.DPS)) as pool:
        res = pool.map(_job, jobs, chunksize=1)
    nao = res[0][0].shape[0]
    dA = np.array([r[0] for r in res]).reshape(len(pts), 3, nao, nao)
    meta["largest_step_disagreement"] = max(r[1] for r in res)
    print("largest |dA(h) - dA(h_check)|:", meta["largest_step_disagreement"])
    path = os.path.join(HERE, f"point_field_ref_{family}.npz")
    save(path, meta, points=pts, point_index=index, dA=dA)
    assert os.path.getsize(path) <= LARGEST_FIXTURE, "larger than the largest committed fixture: keep a subset of the points"


if __name__ == "__main__":
    for name in sys.argv[1:] or ["z1", "z3"]:
        {"z1": lambda: make("z1", "eri_ref_z1.npz", True), "z3": lambda: make("z3", "eri_ref_z3.npz", False)}[name]()
