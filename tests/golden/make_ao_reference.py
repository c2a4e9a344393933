"""Writes tests/golden/ao_ref_*.npz: raw shell definitions, points and the AO planes of oracle/ao_reference.py (mpmath,
100 digits) rounded once to double.  Deterministic: running it again re-creates the files byte for byte.  Measured: 13 s
for all files on eight cores (the self-check of the reference's derivative planes against mp.diff included).

    python tests/golden/make_ao_reference.py

Files (tests/ao_reference_cases.py is the reader; sets P, C, T, S as its docstring lists them):
  ao_ref_p_vg.npz, ao_ref_p_h.npz   set P, even nao: planes v x y z / xx xy xz yy yz zz (two files for the size limit)
  ao_ref_p_extra.npz                the additional s shell of the odd variant: its definition, where it goes, its column
  ao_ref_c.npz                      set C, with ref_cut40 (every primitive of a r^2 >= 40 left out), run (the 32 leading
                                    points), near (the two of them inside), far_point, cut_points (point, shell, primitive, side)
  ao_ref_t.npz                      set T
  ao_ref_s_<table>.npz              set S: v x y z at the 43 points of the table's AO case, sampled columns
  ao_ref_h_t130.npz                 the six Hessian planes of t130 at the same points, sampled columns

Every file: centre, l, nprim, exp, coef (raw, as eri_ref_z*.npz), points, planes (indices into PLANES), cols (the AO columns
stored), ref (len(planes), ngrid, len(cols)), scale_shells, scale_T, scale_d (fitted transform rows and primitive
coefficients of the shells that own the stored columns, as doubles: the tests' fp64 magnitude A uses them, so that the
scale does not come from the product's normalisation either), meta (JSON: digits, self-check).

Points of P (99): the five centres; per centre one point off it along one axis and one in a coordinate plane (the other
components exactly 0); 1e-3 and 1e-8 bohr from every centre; r = 1 / sqrt(2a) of the tightest and the most diffuse
primitive of every shell; generic points.  T: every third point of P, molecule and points moved by SHIFT and rounded to
double, the result taken as exact.
"""
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ao_reference as AR, eri_reference as R  # noqa: E402
from make_eri_reference import save  # noqa: E402
import ao_reference_cases as arc  # noqa: E402
import sweep_cases as sc  # noqa: E402

NP_TOTAL = 99


def unit(i):
    """A generic direction, no zero component, different for every i."""
    v = np.array([np.cos(1.0 + 2.3 * i), np.sin(0.7 + 1.1 * i) * 0.9 + 0.05, np.cos(2.9 * i - 0.4) * 0.8 + 0.1])
    return v / np.linalg.norm(v)


# ------------------------------------------------------------------------------------------------------------- point sets
def p_points(raw):
    cen = arc.P_XYZ
    pts = [c.copy() for c in cen]
    for i, c in enumerate(cen):
        a = np.zeros(3); a[i % 3] = 0.7 + 0.1 * i
        b = np.array([0.6, -0.45, 0.35]); b[(i + 2) % 3] = 0.0
        pts += [c + a, c + b]
    for i, c in enumerate(cen):
        pts += [c + 1e-3 * unit(i), c + 1e-8 * unit(i + 7)]
    k = 20
    for c, l, e, _ in raw:
        for a in sorted({max(e), min(e)}, reverse=True):
            pts.append(np.asarray(c) + unit(k) / np.sqrt(2.0 * a))
            k += 1
    rng = np.random.default_rng(20261021)
    n_gen = NP_TOTAL - len(pts)
    assert n_gen >= 8, len(pts)
    pts += list(cen[rng.integers(0, len(cen), n_gen)] + 1.2 * rng.standard_normal((n_gen, 3)))
    pts = np.array(pts)
    assert len(pts) % 8 != 0
    return pts


C_CENTRES = [(0.0, 0.0, 0.0), (1.5, -0.8, 0.6)]
C_SHELLS = [(0, [(2.5, 1.0)]), (0, [(40.0, 0.3), (6.0, 0.5), (0.9, 0.4)]),
            (1, [(1.1, 1.0)]), (1, [(12.0, 0.4), (2.2, 0.6), (0.6, 0.3)]),
            (2, [(0.8, 1.0)]), (2, [(5.0, 0.5), (1.2, 0.7), (0.5, 0.2)]),
            (3, [(0.7, 1.0)]), (3, [(2.4, 0.6), (0.55, 0.5)])]
C_CUT_PRIMS = [(0, 0), (2, 0), (4, 0), (6, 0), (1, 0), (5, 2)]          # (shell, primitive) whose cut radius gets four points
C_SIDES = (-1e-2, 1e-2, -1e-6, 1e-6)


def c_raw():
    return [(C_CENTRES[i % 2], l, [e for e, _ in p], [c for _, c in p]) for i, (l, p) in enumerate(C_SHELLS)]


def c_points(raw):
    rng = np.random.default_rng(46)
    a_min = min(min(e) for _, _, e, _ in raw)
    run = []
    for i in range(32):
        if i in (5, 29):
            run.append(np.asarray(C_CENTRES[i % 2]) + 0.5 * unit(i))
        else:
            run.append(rng.uniform(12.5, 16.0) * unit(3 * i + 1))
    for i, p in enumerate(run):                       # all but 5 and 29 beyond every primitive's cut of every shell, with margin
        t = min(a_min * float(np.sum((p - np.asarray(c)) ** 2)) for c in C_CENTRES)
        assert (t < 10.0) if i in (5, 29) else (t > 46.0 * 1.2), (i, t)
    pts, marks = list(run), []
    for n, (s, p) in enumerate(C_CUT_PRIMS):
        c, _, e, _ = raw[s]
        for side in C_SIDES:
            marks.append((len(pts), s, p, side))
            pts.append(np.asarray(c) + np.sqrt(46.0 * (1.0 + side) / e[p]) * unit(40 + n))
    far = len(pts)
    pts.append(np.array([37.0, -41.0, 28.0]))        # 60 bohr from everything
    pts += list(np.asarray(C_CENTRES)[rng.integers(0, 2, 6)] + 1.5 * rng.standard_normal((6, 3)))
    pts = np.array(pts)
    assert len(pts) % 8 != 0 and min(np.linalg.norm(pts[far] - np.asarray(c)) for c in C_CENTRES) > 59.0
    return pts, np.array(marks), far


def s_sample(sh, cap, per_l):
    """Sampled columns of a table: the first and the last column of every column block, the columns either side of every
    block seam and of the seam before a borrowed shell moved over, the last column, and `per_l` whole shells of every l
    spread over the table; at most `cap` columns.  Returns (the shells that own them, the columns), both ascending."""
    blocks, _ = sc.ao_blocks(sh.l)
    cols = []
    for lo, hi, c0, nc in blocks:
        cols += [c0, c0 + nc - 1]
        if lo:                                          # the seam as the shells alone would put it (odd where a shell was borrowed)
            end = int(sh.ao[lo]) + 2 * int(sh.l[lo]) + 1
            cols += [c0 - 1, end - 1, min(end, sh.nao - 1)]
    cols.append(sh.nao - 1)
    for l in range(4):
        ids = np.nonzero(np.asarray(sh.l) == l)[0]
        for j in range(per_l if len(ids) else 0):        # (borrow has no f shell)
            s = int(ids[(len(ids) - 1) * j // max(1, per_l - 1)])
            cols += list(range(int(sh.ao[s]), int(sh.ao[s]) + 2 * l + 1))
    cols = np.array(sorted(set(cols)))
    assert len(cols) <= cap, len(cols)
    owner = np.repeat(np.arange(sh.nshell), 2 * np.asarray(sh.l) + 1)
    return sorted(set(int(s) for s in owner[cols])), cols


def table_raw(name):
    """Raw definition of a sweep_cases table.  ao_table hands RAW coefficients to eri_fixtures.shell_table; they are drawn
    again here from the same generator state, and the result is held against the table (exponents, shapes) before use."""
    captured = {}
    import eri_fixtures
    orig = eri_fixtures.shell_table

    def spy(centre, l, nprim, exp, coef):
        captured.update(centre=np.array(centre), l=np.array(l), nprim=np.array(nprim), exp=np.array(exp), coef=np.array(coef))
        return orig(centre, l, nprim, exp, coef)

    eri_fixtures.shell_table = spy
    try:
        sc.ao_table.cache_clear()
        sh = sc.ao_table(name)
    finally:
        eri_fixtures.shell_table = orig
        sc.ao_table.cache_clear()
    assert np.array_equal(captured["exp"], sh.exp) and np.array_equal(captured["l"], sh.l)
    off = np.concatenate([[0], np.cumsum(captured["nprim"])])
    raw = [(tuple(captured["centre"][s]), int(captured["l"][s]), list(captured["exp"][off[s]:off[s + 1]]),
            list(captured["coef"][off[s]:off[s + 1]])) for s in range(len(captured["l"]))]
    return raw, sh


def s_case(table):
    return next(c for c in sc.AO_CASES if c.table == table)


# ------------------------------------------------------------------------------------------------------------- the work
def _job(args):
    key, l, centre, exps, coefs, points, deriv, skip = args
    sh = R.Shell(l, centre, exps, coefs)
    ref, _ = AR.shell_planes(sh, points, deriv, skip)
    T, d = AR.shell_scale(sh)
    return key, R.to_double(ref), T, d


def definition(raw):
    return dict(centre=np.array([c for c, _, _, _ in raw]), l=np.array([l for _, l, _, _ in raw], dtype=np.int32),
                nprim=np.array([len(e) for _, _, e, _ in raw], dtype=np.int32),
                exp=np.array([x for _, _, e, _ in raw for x in e]), coef=np.array([x for _, _, _, k in raw for x in k]))


def main():
    t_all = time.time()
    worst_self = AR.self_check(30)
    print(f"self-check against mp.diff: worst relative difference {worst_self:.1e}  ({time.time() - t_all:.1f} s)")

    # (file key) -> raw shells, points, deriv, shells to compute, stored planes
    sets = {}
    p_even, p_odd = arc.p_raw_shells(False), arc.p_raw_shells(True)
    ins = next(i for i, (a, b) in enumerate(zip(p_even + [None], p_odd)) if a != b)
    assert p_odd[:ins] + p_odd[ins + 1:] == p_even and p_odd[ins][1] == 0
    assert sum(2 * l + 1 for _, l, _, _ in p_even) == 76
    pp = p_points(p_even)
    sets["p"] = (p_even, pp, 2, list(range(len(p_even))), None)
    sets["p_extra"] = ([p_odd[ins]], pp, 2, [0], None)
    craw = c_raw()
    cp, marks, far = c_points(craw)
    sets["c"] = (craw, cp, 2, list(range(len(craw))), None)
    sets["c40"] = (craw, cp, 2, list(range(len(craw))), 40.0)
    t_idx = np.arange(len(pp))[::3][:32]
    assert len(t_idx) == 32
    t_raw = [(tuple(float(x) for x in (np.asarray(c) + arc.SHIFT)), l, e, k) for c, l, e, k in p_even]
    sets["t"] = (t_raw, pp[t_idx] + arc.SHIFT, 2, list(range(len(t_raw))), None)
    samples = {}
    for tb in arc.S_TABLES:
        raw, sh = table_raw(tb)
        pts = np.array(sc.grid_inputs(s_case(tb))[0])
        shells, cols = s_sample(sh, 160, 3)
        samples["s_" + tb] = (sh, shells, cols)
        sets["s_" + tb] = (raw, pts, 1, shells, None)
        if tb == arc.H_TABLE:
            shells_h, cols_h = s_sample(sh, 64, 2)
            samples["h_" + tb] = (sh, shells_h, cols_h)
            sets["h_" + tb] = (raw, pts, 2, shells_h, None)

    jobs = []
    for key, (raw, pts, deriv, shells, skip) in sets.items():
        for s in shells:
            c, l, e, k = raw[s]
            jobs.append(((key, s), l, c, e, k, pts, deriv, skip))
    jobs.sort(key=lambda j: -len(j[4]) * (j[1] + 1) * (j[1] + 2) * len(j[5]) * (1, 4, 10)[j[6]])
    t0 = time.time()
    with multiprocessing.get_context("fork").Pool(8) as pool:
        done = dict((k, v) for k, *v in pool.imap_unordered(_job, jobs, chunksize=1))
    seconds = time.time() - t0
    print(f"{len(jobs)} shell jobs: {seconds:.1f} s")

    def assemble(key):
        raw, pts, deriv, shells, skip = sets[key]
        ref = np.concatenate([done[(key, s)][0] for s in shells], axis=2)
        if key in samples:                              # whole shells were computed: keep the sampled columns
            sh, _, cols = samples[key]
            have = np.concatenate([np.arange(int(sh.ao[s]), int(sh.ao[s]) + 2 * int(sh.l[s]) + 1) for s in shells])
            ref = ref[:, :, np.searchsorted(have, cols)]
        T = np.concatenate([done[(key, s)][1].ravel() for s in shells])
        d = np.concatenate([done[(key, s)][2] for s in shells])
        return raw, pts, ref, shells, T, d

    meta = dict(dps=R.DPS, self_check=worst_self, self_check_digits=30, floor=arc.FLOOR)       # (no run time: byte-for-byte files)

    def write(name, raw, pts, planes, cols, ref, shells, T, d, **more):
        save(os.path.join(HERE, f"ao_ref_{name}.npz"), meta, points=pts, planes=np.array(planes, dtype=np.int32), cols=np.array(cols, dtype=np.int32),
             ref=ref, scale_shells=np.array(shells, dtype=np.int32), scale_T=T, scale_d=d, **definition(raw), **more)

    raw, pts, ref, shells, T, d = assemble("p")
    write("p_vg", raw, pts, range(4), range(76), ref[:4], shells, T, d)
    write("p_h", raw, pts, range(4, 10), range(76), ref[4:], shells, T, d)
    raw, pts, ref, shells, T, d = assemble("p_extra")
    write("p_extra", raw, pts, range(10), [int(sum(2 * l + 1 for _, l, _, _ in p_odd[:ins]))], ref, shells, T, d, insert_shell=np.array(ins))
    raw, pts, ref, shells, T, d = assemble("c")
    ref40 = assemble("c40")[2]
    nao_c = ref.shape[2]
    write("c", raw, pts, range(10), range(nao_c), ref, shells, T, d, ref_cut40=ref40, run=np.arange(32), near=np.array([5, 29]),
          far_point=np.array(far), cut_points=marks.astype(np.float64))
    raw, pts, ref, shells, T, d = assemble("t")
    write("t", raw, pts, range(10), range(76), ref, shells, T, d)
    for key, (sh, shells_k, cols) in samples.items():
        raw, pts, ref, shells, T, d = assemble(key)
        assert ref.shape[2] == len(cols)
        planes = range(4) if key.startswith("s_") else range(4, 10)
        write(key, raw, pts, planes, cols, ref if key.startswith("s_") else ref[4:], shells, T, d)
    print(f"all files: {time.time() - t_all:.1f} s")


if __name__ == "__main__":
    main()
