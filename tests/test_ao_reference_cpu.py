"""The host statements of the AO planes -- oracle.eval_ao (values, gradients) and gradients.ao_hessian_host (Hessians) --
against the 100-digit reference of tests/golden/ao_ref_*.npz, element by element under the error model of
tests/ao_reference_cases.py; the teeth of that check; the sampling and ledger rules the device file relies on.
Golden files only: no mpmath (but for the regeneration spot-check, which runs where mpmath imports).

With QCDFT_WRITE_PROFILES set the worst ratios are recorded as "cpu ..." lines of ao_reference_parity.txt in that directory.
"""
import math

import numpy as np
import pytest

import oracle
from quantum_compute_dft_amd import basis, gradients

import ao_reference_cases as arc
import sweep_cases as sc

ALL = ["p_even", "p_odd", "c", "t"] + ["s_" + t for t in arc.S_TABLES] + ["h_" + arc.H_TABLE]
_HOST = {}


def host_planes(name):
    """Engine output (len(planes), ngrid, ncol) of the host statements on fixture `name`, at its stored planes and columns."""
    if name not in _HOST:
        f = arc.load(name)
        ao, gr = oracle.eval_ao(f.sh, f.points, deriv=1)
        full = np.concatenate([ao[None], gr])
        if max(f.planes) >= 4:
            full = np.concatenate([full, gradients.ao_hessian_host(f.sh, f.points)])
        got = f.take(full[f.planes], f.planes)
        got.setflags(write=False)
        _HOST[name] = got
    return _HOST[name]


@pytest.mark.parametrize("name", ALL)
def test_host_statements_match_the_reference(name):
    f = arc.load(name)
    A, CUT = arc.scales(name)
    arc.check(f, host_planes(name), f.planes, A, CUT, name, tag="cpu")


def test_k_comes_from_the_host_ratios():
    """K = 4 x the worst host ratio over P, C, T, up to a power of two -- here: K is at least that and at most 256."""
    worst = {"vg": 0.0, "h": 0.0}
    for name in ("p_even", "p_odd", "c", "t"):
        f = arc.load(name)
        A, CUT = arc.scales(name)
        r = arc.ratios(host_planes(name), f.ref, A, CUT)
        worst["vg"] = max(worst["vg"], float(r[:4].max()))
        worst["h"] = max(worst["h"], float(r[4:].max()))
    arc.record("cpu", "K-source oracle.eval_ao over P, C, T", worst["vg"], arc.K_VG)
    arc.record("cpu", "K-source gradients.ao_hessian_host over P, C, T", worst["h"], arc.K_HESS)
    for w, K in ((worst["vg"], arc.K_VG), (worst["h"], arc.K_HESS)):
        assert 4.0 * w <= K <= 256.0 and math.log2(K) == int(math.log2(K))


def test_the_sets_hold_what_they_are_for():
    p = arc.load("p_even")
    assert p.sh.nao == 76 and arc.load("p_odd").sh.nao == 77 and p.points.shape[0] % 8
    assert p.sh.exp.max() > 13000 and set(int(x) for x in p.sh.l) == {0, 1, 2, 3}
    A, _ = arc.scales("p_even")
    assert ((p.ref == 0.0) & (A == 0.0)).sum() > 1000          # on-centre points and zeros of the harmonics
    c = arc.load("c")
    run, near, far = c.extra["run"], c.extra["near"], int(np.ravel(c.extra["far_point"])[0])
    assert list(run) == list(range(32)) and list(near) == [5, 29]
    a_min = np.array([c.sh.exp[o:o + n].min() for o, n in zip(c.sh.off, c.sh.nprim)])
    r2 = ((c.points[:, None, :] - c.sh.xyz[None, :, :]) ** 2).sum(axis=2)
    beyond = (a_min[None, :] * r2 >= 1.2 * arc.AO_EXP_CUT).all(axis=1)
    assert list(np.nonzero(~beyond[:32])[0]) == [5, 29] and beyond[far] and r2[far].min() > 59.0 ** 2
    for g, s, p_, side in c.extra["cut_points"]:                # a r^2 = 46 (1 + side) of the chosen primitive, to the point's rounding
        t = c.sh.exp[c.sh.off[int(s)] + int(p_)] * r2[int(g), int(s)]
        assert abs(t / (arc.AO_EXP_CUT * (1.0 + side)) - 1.0) < 1e-12
    t_ = arc.load("t")
    assert np.abs(t_.sh.xyz).min() > 900.0 and t_.points.shape[0] == 32


@pytest.mark.parametrize("odd", [False, True])
def test_build_shells_reproduces_the_reference_shell_by_shell(odd):
    """basis.build_shells on P's molecule: its normalised coefficients through the host statements, per shell, so that a
    normalisation error names its shell."""
    f = arc.load("p_odd" if odd else "p_even")
    sh = basis.build_shells(arc.P_SYMS, arc.P_XYZ, arc.p_basis(odd))
    assert np.array_equal(sh.l, f.sh.l) and np.array_equal(sh.exp, f.sh.exp) and np.array_equal(sh.xyz, f.sh.xyz)
    ao, gr = oracle.eval_ao(sh, f.points, deriv=1)
    got = np.concatenate([ao[None], gr, gradients.ao_hessian_host(sh, f.points)])
    A, CUT = arc.scales(f.name)
    for s in range(sh.nshell):
        cols = slice(int(sh.ao[s]), int(sh.ao[s]) + 2 * int(sh.l[s]) + 1)
        for k in range(10):
            ok = arc.within(got[k][:, cols], f.ref[k][:, cols], A[k][:, cols], CUT[k][:, cols], arc.k_of(k))
            assert ok.all(), f"shell {s} (atom {int(sh.atom[s])}, l={int(sh.l[s])}, {int(sh.nprim[s])} primitives) plane {arc.PLANES[k]}"


# --------------------------------------------------------------------------------------------------------------- teeth
def _column_of(f, l, which=0):
    return int(np.nonzero(f.col_l == l)[0][which])


@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_teeth_a_column_scaled_by_1e_minus_13_fails(l):
    f = arc.load("p_even")
    A, CUT = arc.scales("p_even")
    got = host_planes("p_even").copy()
    assert arc.passes(f, got, f.planes, A, CUT)
    got[:, :, _column_of(f, l, 1)] *= 1.0 + 1e-13
    assert not arc.passes(f, got, f.planes, A, CUT)
    only_values = [0]
    assert not arc.passes(f, got[:1], only_values, A[:1], CUT[:1])


def test_teeth_a_flipped_sign_in_one_f_gradient_entry_fails():
    """Sx of the f component y (4 z2 - x2 - y2) with the wrong sign: grad_x = R0 Sx + R1 S x becomes -R0 Sx + R1 S x.  On the
    single-primitive f shell of C, R1 = -2 a R0, so R0 Sx = grad_x + 2 a x value."""
    f = arc.load("c")
    A, CUT = arc.scales("c")
    got = host_planes("c").copy()
    s = next(i for i in range(f.sh.nshell) if f.sh.l[i] == 3 and f.sh.nprim[i] == 1)
    col, a = int(f.sh.ao[s]) + 2, float(f.sh.exp[f.sh.off[s]])
    x = f.points[:, 0] - f.sh.xyz[s, 0]
    r0sx = got[1, :, col] + 2.0 * a * x * got[0, :, col]
    got[1, :, col] -= 2.0 * r0sx
    assert arc.passes(f, host_planes("c"), f.planes, A, CUT) and not arc.passes(f, got, f.planes, A, CUT)


def test_teeth_a_cut_taken_too_early_fails():
    """The oracle keeps every primitive; ref_cut40 leaves out those of a r^2 >= 40: a cut at 40 is outside the allowance."""
    f = arc.load("c")
    A, CUT = arc.scales("c")
    assert not arc.passes(f, host_planes("c"), f.planes, A, CUT, ref=f.extra["ref_cut40"])
    assert not arc.passes(f, host_planes("c")[:1], [0], A[:1], CUT[:1], ref=f.extra["ref_cut40"])


def test_teeth_two_swapped_d_components_fail():
    f = arc.load("p_even")
    A, CUT = arc.scales("p_even")
    got = host_planes("p_even").copy()
    c0 = _column_of(f, 2)
    got[:, :, [c0, c0 + 1]] = got[:, :, [c0 + 1, c0]]
    assert not arc.passes(f, got, f.planes, A, CUT)


# ------------------------------------------------------------------------------------------- sampling, ledger, regeneration
@pytest.mark.parametrize("table", arc.S_TABLES)
def test_sample_rules(table):
    f = arc.load("s_" + table)
    sh = sc.ao_table(table)
    for k in ("xyz", "l", "nprim", "exp", "coef"):
        assert np.array_equal(getattr(f.sh, k), getattr(sh, k)), k          # the file's table is the case's table
    case = next(c for c in sc.AO_CASES if c.table == table)
    assert np.array_equal(f.points, sc.grid_inputs(case)[0]) and f.ref.shape[1] == sc.NG_AO      # no row is left out
    blocks, borrowed = sc.ao_blocks(sh.l)
    cols = set(int(c) for c in f.cols)
    for lo, hi, c0, nc in blocks:
        assert c0 in cols and c0 + nc - 1 in cols, (table, c0, nc)
    assert sh.nao - 1 in cols and set(int(x) for x in f.col_l) == set(int(x) for x in sh.l)
    assert len(cols) <= 160 and f.planes == [0, 1, 2, 3]
    if table == "borrow":
        assert borrowed == 1 and {124, 125} <= cols                           # either side of the odd seam
    if table == arc.H_TABLE:
        h = arc.load("h_" + table)
        assert len(h.cols) <= 64 and h.planes == [4, 5, 6, 7, 8, 9] and len(blocks) == 2
        assert np.array_equal(h.points, f.points) and set(int(x) for x in h.col_l) == set(int(x) for x in sh.l)
        assert all(c0 in h.cols and c0 + nc - 1 in h.cols for _, _, c0, nc in blocks)


def test_device_runs_reach_every_instantiation_of_k_eval_ao():
    reached = {sc.ao_kernel(arc.load(n).sh, grad, pt, aligned) for n, grad, pt, aligned in arc.ao_runs()}
    every = {("k_eval_ao", (g, v, pt, tab)) for g in (False, True) for v in (False, True) for pt in (8, 16) for tab in (False, True)}
    assert reached == every and len(every) == sc.LEDGER_FLOOR["k_eval_ao"]
    in_lds = {k for n, g, pt, al in arc.ao_runs() if not n.startswith("s_") for k in [sc.ao_kernel(arc.load(n).sh, g, pt, al)]}
    assert in_lds == {k for k in every if k[1][3]}                             # P, C, T: the eight TAB = true ones


def test_regenerated_elements_are_the_stored_bits():
    """Twenty stored elements of P recomputed at 100 digits (where mpmath imports)."""
    pytest.importorskip("mpmath")
    from oracle import ao_reference as AR, eri_reference as R
    f = arc.load("p_odd")
    rng = np.random.default_rng(99)
    off = np.concatenate([[0], np.cumsum(f.raw["nprim"])])
    for _ in range(20):
        k, g, col = int(rng.integers(0, 10)), int(rng.integers(0, f.points.shape[0])), int(rng.integers(0, f.sh.nao))
        s = int(f.col_shell[col])
        shell = R.Shell(int(f.raw["l"][s]), f.raw["centre"][s], f.raw["exp"][off[s]:off[s + 1]], f.raw["coef"][off[s]:off[s + 1]])
        ref, _ = AR.shell_planes(shell, f.points[g:g + 1], 2)
        assert float(ref[k, 0, col - int(f.sh.ao[s])]) == f.ref[k, g, col], (k, g, col)
