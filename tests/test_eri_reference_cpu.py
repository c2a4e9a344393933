"""The integral engines against a reference that shares no code and no formulation with them.

oracle/eri_reference.py (mpmath, 100 digits) evaluates the same contracted real-solid-harmonic integrals through the
Rys-Dupuis-King two-dimensional integrals, an exact interpolatory rule in t^2 and mpmath's incomplete gamma function;
csrc/integrals.c and csrc/eri_cols.hip use McMurchie-Davidson with a Boys function of their own.  The values, rounded to
double, are stored in tests/golden/eri_ref_z{1,2,3}.npz (written by tests/golden/make_eri_reference.py).

First part (needs mpmath): evidence that the reference is right -- a derivative ladder that raises the angular momentum
without the reference's own recurrence, textbook numbers, properties of the stored values, and a spot-check that the
stored values are what the reference computes.  Second part (numpy only): the HOST engine against the fixtures; the
device engine's turn is tests/test_gpu_eri_reference.py.

Bound of the second part: eri_fixtures.BOUND = 1e-12 * max(1, max|ref| of the block), in every family (measured worst
host error 2.5e-14, at the R = 3e-7 geometry where the engines' x < 1e-13 switch of the Boys function drops a term of
that size; see profiles/eri_reference_parity.txt)."""
import numpy as np
import pytest

import eri_fixtures as F
from quantum_compute_dft_amd import basis, integrals


def _ref():
    pytest.importorskip("mpmath")
    from oracle import eri_reference
    return eri_reference


def _ulps(got, stored):
    return abs(got - stored) / np.spacing(abs(stored)) if stored != 0.0 else (0.0 if got == 0.0 else np.inf)


# ------------------------------------------------------------------------------------------ the reference itself
def test_boys_function_is_its_defining_integral():
    R = _ref()
    from mpmath import mp, mpf
    with mp.workdps(50):
        for x in (0, mpf("1e-13"), mpf("0.37"), 9, 41):
            F_ = R.boys(12, x)
            for m in (0, 5, 12):
                want = mp.quad(lambda t: t ** (2 * m) * mp.exp(-x * t * t), mp.linspace(0, 1, 9))
                assert abs(F_[m] - want) <= mpf(10) ** -40 * want, (x, m)
        F_ = R.boys(12, 1900)                         # the part of the integral beyond t = 1 is below exp(-1900)
        for m in (0, 5, 12):
            want = mp.gamma(m + mpf(1) / 2) / (2 * mpf(1900) ** (m + mpf(1) / 2))
            assert abs(F_[m] - want) <= mpf(10) ** -40 * want, m


def test_fitted_harmonics_have_the_project_order_and_sign():
    R = _ref()
    from mpmath import mp
    with mp.workdps(R.DPS):
        def shape(l, row):
            c = R.sph_coeffs(l)[row]
            big = max(abs(v) for v in c)
            return {p: int(mp.nint(v / big * 12)) for p, v in zip(R.cart_powers(l), c) if v != 0}
        assert [max(shape(1, r), key=lambda p: shape(1, r)[p]) for r in range(3)] == [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
        assert shape(2, 0) == {(1, 1, 0): 12} and shape(2, 1) == {(0, 1, 1): 12} and shape(2, 3) == {(1, 0, 1): 12}
        assert shape(2, 2) == {(2, 0, 0): -6, (0, 2, 0): -6, (0, 0, 2): 12}                # 2 z2 - x2 - y2
        assert shape(2, 4) == {(2, 0, 0): 12, (0, 2, 0): -12}                              # x2 - y2
        assert shape(3, 0) == {(2, 1, 0): 12, (0, 3, 0): -4}                               # y (3 x2 - y2)
        assert shape(3, 1) == {(1, 1, 1): 12}                                              # x y z
        assert shape(3, 3) == {(2, 0, 1): -12, (0, 2, 1): -12, (0, 0, 3): 8}               # z (2 z2 - 3 x2 - 3 y2)
        assert shape(3, 6) == {(3, 0, 0): 4, (1, 2, 0): -12}                               # x (x2 - 3 y2)
        assert shape(3, 2)[(0, 1, 2)] > 0 and shape(3, 4)[(1, 0, 2)] > 0 and shape(3, 5) == {(2, 0, 1): 12, (0, 2, 1): -12}


@pytest.mark.parametrize("pos", range(4))
def test_derivative_ladder_from_s_to_f(pos):
    """d/dA_x [a b|c d] = 2 alpha [a + 1_x b|c d] - a_x [a - 1_x b|c d] for Cartesian primitives, the left side by a
    central difference (step 1e-18; the reference works at 100 digits): the raised function on the right comes from
    the reference's recurrences, the left side only from integrals of the lower one."""
    R = _ref()
    from mpmath import mp, mpf
    exps = [mpf("0.9"), mpf("1.4"), mpf("0.55"), mpf("2.1")]
    cen = [[mpf(x) for x in c] for c in ((0.10, -0.20, 0.05), (1.25, 0.90, 1.60), (-1.10, 0.70, -0.40), (0.30, -1.30, 1.20))]
    others = [(1, 0, 0), (0, 1, 1), (0, 0, 1), (1, 1, 0)]
    h = mpf("1e-18")
    with mp.workdps(R.DPS):
        for comp in ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 1), (2, 0, 0), (0, 1, 1)):       # s, p, d at `pos`: raised to p, d, f
            pw = list(others)

            def val(p, shift=0):
                pw[pos] = p
                c = [list(v) for v in cen]
                c[pos][0] += shift
                return R.cart_prim_eri(pw, exps, c)

            lhs = (val(comp, h) - val(comp, -h)) / (2 * h)
            rhs = 2 * exps[pos] * val((comp[0] + 1, comp[1], comp[2]))
            if comp[0]:
                rhs -= comp[0] * val((comp[0] - 1, comp[1], comp[2]))
            assert abs(rhs) > mpf("1e-8") and abs(lhs - rhs) <= mpf("1e-25") * abs(rhs), (pos, comp)


def test_szabo_ostlund_h2_sto3g():
    R = _ref()
    ex = basis._STO3G_EXPS["H"][0]
    co = basis._STO3G_1S[1]
    sh = [R.Shell(0, (0, 0, 0), ex, co), R.Shell(0, (0, 0, 1.4), ex, co)]
    S, T, _ = (R.to_double(m) for m in R.one_electron(sh, []))
    assert abs(S[0, 1] - 0.6593) < 5e-5 and abs(T[0, 0] - 0.7600) < 5e-5
    assert abs(float(R.eri_quartet(sh[0], sh[0], sh[0], sh[0])[0, 0, 0, 0]) - 0.7746) < 5e-5
    assert abs(float(R.eri_quartet(sh[0], sh[0], sh[1], sh[1])[0, 0, 0, 0]) - 0.5697) < 5e-5


# ------------------------------------------------------------------------------------------ the stored values
def _same(a, b):
    return np.all(np.abs(a - b) <= np.spacing(np.abs(a)) + 1e-30)


def test_fixtures_are_small():
    import os
    sizes = [os.path.getsize(os.path.join(F.GOLDEN, f"eri_ref_z{k}.npz")) for k in (1, 2, 3)]
    assert max(sizes) <= 512 * 1024 and sum(sizes) <= 1.25 * 1024 * 1024


def test_symmetry_where_the_generator_did_not_impose_it():
    """Z1 stores one copy of every element, so its check_quartets were computed a second time in another index order;
    the Z3 columns hold (kl|ij), (lk|ij) and elements of different shell quartets ((ff|ds) and (ds|ff)) side by side."""
    f = F.z1()
    sh, eri, d = f["sh"], f["eri"], f["raw"]
    o = 0
    for q in d["check_quartets"]:
        sl = tuple(slice(int(sh.ao[s]), int(sh.ao[s]) + 2 * int(sh.l[s]) + 1) for s in q)
        n = int(np.prod([s.stop - s.start for s in sl]))
        assert _same(d["check_values"][o:o + n].reshape([s.stop - s.start for s in sl]), eri[sl]), q
        o += n
    assert o == len(d["check_values"])
    z = F.z3()
    sh = z["sh"]
    ff, ds = z["cols"][0], z["cols"][1]
    f0, d0, s0 = int(sh.ao[10]), int(sh.ao[9]), int(sh.ao[0])
    blk = ff[:, f0:f0 + 7, f0:f0 + 7].reshape(7, 7, 7, 7)                       # [k, l, i, j]
    assert _same(blk, blk.transpose(1, 0, 2, 3)) and _same(blk, blk.transpose(2, 3, 0, 1)) and _same(blk, blk.transpose(0, 1, 3, 2))
    assert _same(ff[:, d0:d0 + 5, s0].reshape(7, 7, 5), ds[:, f0:f0 + 7, f0:f0 + 7].transpose(1, 2, 0))


def test_schwarz_inequality_positive_matrix_and_unit_diagonal():
    f = F.z1()
    eri, n = f["eri"], f["sh"].nao
    M = eri.reshape(n * n, n * n)
    dg = np.sqrt(np.diag(M))
    assert np.all(np.abs(M) <= np.outer(dg, dg) * (1 + 1e-14) + 1e-300)
    w = np.linalg.eigvalsh(M)
    assert w[0] >= -1e-13 * np.abs(w).max()
    z = F.z3()
    f0 = int(z["sh"].ao[10])
    blk = z["cols"][0][:, f0:f0 + 7, f0:f0 + 7].reshape(49, 49)
    dg = np.sqrt(np.diag(blk))
    assert np.all(np.abs(blk) <= np.outer(dg, dg) * (1 + 1e-14)) and np.linalg.eigvalsh(blk)[0] >= -1e-13 * np.abs(blk).max()
    g0 = F.z2()[0]                                                             # R = 0: X and Y coincide, (ss|ss) is a diagonal-like element
    assert g0["cols"][2][0, 0, 0] > 0
    for fx in (f, z):
        assert np.abs(np.diag(fx["S"]) - 1.0).max() <= 1e-15
        for name in "STV":
            assert _same(fx[name], fx[name].T)
        assert np.linalg.eigvalsh(fx["S"])[0] > 0 and np.linalg.eigvalsh(fx["T"])[0] > 0 and np.linalg.eigvalsh(fx["V"])[-1] < 0


def _ref_shells(R, d, centre=None):
    centre = d["centre"] if centre is None else centre
    off = np.concatenate([[0], np.cumsum(d["nprim"])])
    return [R.Shell(int(l), c, d["exp"][off[i]:off[i + 1]], d["coef"][off[i]:off[i + 1]]) for i, (l, c) in enumerate(zip(d["l"], centre))]


def test_stored_values_are_what_the_reference_computes():
    """About 40 stored integrals recomputed now, equal to the stored double to 2 ulp: one (ff|ff) element, every Z2
    geometry, every one-electron matrix."""
    R = _ref()
    count = 0

    def check(got, stored, what):
        nonlocal count
        count += 1
        assert abs(float(stored)) > 1e-12 and _ulps(float(got), float(stored)) <= 2, (what, float(got), float(stored))

    f = F.z1()
    sh, eri, sr = f["sh"], f["eri"], _ref_shells(R, f["raw"])
    picks = [((3, 3, 3, 3), [(3, 2, 3, 2)]),                                                 # the (ff|ff) element
             ((5, 0, 6, 1), [(0, 0, 0, 0), (2, 0, 0, 1), (1, 0, 0, 2)]), ((2, 1, 0, 0), [(4, 2, 0, 0), (0, 1, 0, 0)]),
             ((4, 2, 1, 1), [(0, 0, 0, 0), (3, 4, 2, 1), (4, 1, 1, 2)]), ((6, 5, 5, 0), [(0, 1, 2, 0), (0, 0, 0, 0)]),
             ((3, 0, 6, 6), [(6, 0, 0, 0), (0, 0, 0, 0), (3, 0, 0, 0)]), ((4, 4, 2, 2), [(1, 3, 4, 0), (2, 2, 2, 2)]),
             ((3, 1, 5, 4), [(5, 2, 1, 3)]), ((6, 6, 6, 6), [(0, 0, 0, 0)]), ((1, 1, 0, 0), [(0, 0, 0, 0), (2, 1, 0, 0)])]
    for q, elems in picks:
        blk = R.eri_quartet(*[sr[s] for s in q])
        for e in elems:
            check(blk[e], eri[tuple(int(sh.ao[s]) + c for s, c in zip(q, e))], ("z1", q, e))
    for g, (A, B, k, elems) in zip(F.z2(), [(3, 3, 2, [(6, 6, 0, 0), (0, 0, 0, 0)]), (2, 2, 2, [(4, 4, 0, 0), (1, 1, 0, 0)]),
                                            (3, 0, 2, [(1, 0, 0, 0), (0, 0, 0, 0)]), (2, 0, 1, [(3, 0, 2, 1)]), (1, 0, 0, [(0, 0, 6, 6), (0, 0, 0, 0)]),
                                            (3, 2, 1, [(2, 4, 0, 2), (0, 0, 0, 0)])]):
        srg = _ref_shells(R, g["raw"], g["sh"].xyz)
        C, D = g["kets"][k]
        blk = R.eri_quartet(srg[A], srg[B], srg[C], srg[D])
        nd = 2 * int(g["sh"].l[D]) + 1
        for e in elems:
            check(blk[e], g["cols"][k][e[2] * nd + e[3], int(g["sh"].ao[A]) + e[0], int(g["sh"].ao[B]) + e[1]], ("z2", g["R"], e))
    z = F.z3()
    sh, sr = z["sh"], _ref_shells(R, z["raw"])
    for (A, B, k, e) in [(14, 9, 1, (1, 3, 4, 0)), (14, 5, 1, (1, 2, 4, 0)), (12, 1, 2, (0, 0, 2, 0)), (8, 7, 2, (3, 1, 1, 0))]:
        C, D = z["kets"][k]
        blk = R.eri_quartet(sr[A], sr[B], sr[C], sr[D])
        nd = 2 * int(sh.l[D]) + 1
        check(blk[e], z["cols"][k][e[2] * nd + e[3], int(sh.ao[A]) + e[0], int(sh.ao[B]) + e[1]], ("z3", A, B, k, e))
    for fx, srx, (A, B), name in ((f, _ref_shells(R, f["raw"]), (3, 2), "z1"), (z, sr, (14, 10), "z3")):
        chg = list(zip(fx["raw"]["charge_xyz"], fx["raw"]["charge_z"]))
        mats = R.one_electron([srx[A], srx[B]], chg)
        nA = srx[A].nfun
        i, j = int(fx["sh"].ao[A]) + 2, int(fx["sh"].ao[B]) + 1
        for m, key in zip(mats, "STV"):
            check(m[2, nA + 1], fx[key][i, j], (name, key))
            check(m[1, 1], fx[key][i - 1, i - 1], (name, key, "diagonal"))
    assert count >= 40


# ------------------------------------------------------------------------------------------ the host engine
def _assert_within(got, ref, what):
    ok, err, allowed = F.within(got, ref)
    assert ok, (what, err, allowed)
    return err


def test_host_int2e_and_int1e_on_z1():
    f = F.z1()
    _assert_within(integrals.int2e(f["sh"]), f["eri"], "z1 int2e")
    for got, name in zip(integrals.int1e(f["sh"], f["syms"], f["charge_xyz"]), "STV"):
        _assert_within(got, f[name], "z1 " + name)


def test_host_int1e_and_int2e_on_z3():
    z = F.z3()
    sh = z["sh"]
    for got, name in zip(integrals.int1e(sh, z["syms"], z["charge_xyz"]), "STV"):
        _assert_within(got, z[name], "z3 " + name)
    eri = integrals.int2e(sh)
    mask = F.shell_lower_mask(sh)
    for (C, D), ref in zip(z["kets"], z["cols"]):
        c0, d0, nc, nd = int(sh.ao[C]), int(sh.ao[D]), 2 * int(sh.l[C]) + 1, 2 * int(sh.l[D]) + 1
        got = eri[:, :, c0:c0 + nc, d0:d0 + nd].reshape(sh.nao, sh.nao, nc * nd).transpose(2, 0, 1)
        _assert_within(got * mask, ref, ("z3 int2e", C, D))


def _host_columns(sh, C, D, ref, what, nfun=None):
    """EriColumns.cols for (C, D) and (D, C), lower_only and mirrored, against ref (engines' layout)."""
    host = integrals.EriColumns(sh)
    host.diag()
    nc, nd, n = 2 * int(sh.l[C]) + 1, 2 * int(sh.l[D]) + 1, nfun or sh.nao
    full = ref + ref.transpose(0, 2, 1) * ~F.shell_lower_mask(sh, n)                     # the symmetric matrices
    worst = 0.0
    for (c, d), r, rf in (((C, D), ref, full), ((D, C), F.swapped(ref, nc, nd), F.swapped(full, nc, nd))):
        worst = max(worst, _assert_within(host.cols(c, d, 0.0, lower_only=True)[:, :n, :n], r, (what, c, d, "lower")))
        worst = max(worst, _assert_within(host.cols(c, d, 0.0, lower_only=False)[:, :n, :n], rf, (what, c, d, "full")))
    host.close()
    return worst


def test_host_columns_on_z1_every_pair_both_orders():
    sh = F.z1()["sh"]
    for C in range(sh.nshell):
        for D in range(C + 1):
            _host_columns(sh, C, D, F.z1_columns(C, D), "z1")


@pytest.mark.parametrize("g", range(6))
def test_host_columns_on_z2(g):
    z = F.z2()[g]
    sh = z["sh"]
    eri = integrals.int2e(sh)
    for (C, D), ref in zip(z["kets"], z["cols"]):
        _host_columns(sh, C, D, ref, ("z2", z["R"]), nfun=16)
        c0, d0, nc, nd = int(sh.ao[C]), int(sh.ao[D]), 2 * int(sh.l[C]) + 1, 2 * int(sh.l[D]) + 1
        got = eri[:16, :16, c0:c0 + nc, d0:d0 + nd].reshape(16, 16, nc * nd).transpose(2, 0, 1)
        _assert_within(got * F.shell_lower_mask(sh, 16), ref, ("z2 int2e", z["R"], C, D))


def test_host_columns_on_z3():
    z = F.z3()
    for (C, D), ref in zip(z["kets"], z["cols"]):
        _host_columns(z["sh"], C, D, ref, "z3")
