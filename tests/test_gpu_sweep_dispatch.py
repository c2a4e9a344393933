"""Every instantiation of the closed-shell sweep and AO kernels against the CPU oracle on a real MI355X: the case tables
of tests/sweep_cases.py, which tests/test_sweep_cases_cpu.py holds against the compiler's list of instantiations.

Bounds (tests/test_gpu_parity.py, unchanged): Exc relative 1e-12 (absolute 1e-14), Vxc 1e-11 max|V| + 1e-13; AO values
1e-13 and gradients 1e-12 of max(1, max|.|); the direct sweep against the resident call 1e-12 max|V|.  The CPU file
shows that every sweep case is an input on which the oracle itself moves by less than a tenth of the Vxc bound.
With QCDFT_WRITE_PROFILES=<dir> the worst figure per kernel family goes to <dir>/sweep_dispatch_parity.txt.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import quantum_compute_dft_amd as q  # noqa: E402
import sweep_cases as sc  # noqa: E402

NOTED = [0]
WORST = {}   # family -> [Exc relative, Vxc / max|V| (AO: values, gradients), case id of the worst Vxc]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(c, **more):
    s = q.DFTSolverWrapper(q.build_library(), c.xc)
    for k, v in {**sc.options(c), **more}.items():
        s.set_option(k, v)
    return s


def _place(a, dev, aligned=True):
    """Device copy of `a`; `aligned` False: 8 bytes into its allocation."""
    a = np.ascontiguousarray(a)
    if aligned:
        return torch.tensor(a, device=dev)           # (a copy: the shared inputs are read-only)
    t = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), torch.tensor(a, device=dev).reshape(-1)])[1:].view(a.shape)
    assert t.data_ptr() % 16 == 8
    return t


def _note(c, e_exc, e_v):
    NOTED[0] += 1
    for fam in {k[0] for k in sc.expected_kernels(c)} - {"k_eval_ao"}:     # (the AO kernels have figures of their own)
        w = WORST.setdefault(fam, [0.0, 0.0, ""])
        w[0] = max(w[0], e_exc)
        if e_v >= w[1]:
            w[1], w[2] = e_v, sc.case_id(c)


def _check(c, exc, v, exc_ref, v_ref, note=True):
    scale = np.abs(v_ref).max()
    e_exc, e_v = abs(exc - exc_ref) / abs(exc_ref), np.abs(v - v_ref).max() / scale
    print(f"{sc.case_id(c):70s} dExc/Exc {e_exc:9.2e}   dV/max|V| {e_v:9.2e}")
    if note:
        _note(c, e_exc, e_v)
    assert exc == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    assert np.abs(v - v_ref).max() <= 1e-11 * scale + 1e-13


def _run_sweep(c, dev, **more):
    cocc, dm, ao, gr, w = sc.sweep_inputs(c)
    s = _solver(c, **more)
    gga = c.xc != "LDA"
    d_ao, d_gr = _place(ao, dev, c.aligned), (_place(gr, dev, c.aligned) if gga else None)
    d_w, d_dm = _place(w, dev), _place(dm, dev)
    d_v = torch.full((c.nao, c.nao), 7.0, dtype=torch.float64, device=dev)     # must be overwritten
    if c.entry == "xc_occ" and "path" not in more:
        exc = s.compute_xc_occ(c.ngrid, c.nao, cocc.shape[1], _place(cocc, dev), d_ao, d_w, d_v, d_gr, d_dm if c.pass_dm else None)
    else:
        exc = s.compute_xc(c.ngrid, c.nao, d_dm, d_ao, d_w, d_v, d_gr)
    torch.cuda.synchronize()
    return s, exc, d_v.cpu().numpy()


@pytest.mark.parametrize("c", sc.SWEEP_CASES, ids=sc.case_id)
def test_sweep_case_matches_oracle(dev, monkeypatch, c):
    for k, v in c.env:
        monkeypatch.setenv(k, v)          # occ_plan reads them with getenv at every plan
    exc_ref, v_ref = sc.sweep_reference(c)
    s, exc, v = _run_sweep(c, dev)
    # the kernel that ran is the one claimed, as far as the library says what it did
    assert bool(s.get_option("used_occ")) == sc.uses_occ(c, c.nao)
    assert bool(s.get_option("used_vxc_fringe")) == (sc.fringe(c, c.nao) and not sc.takes_tiny(c, c.nao))
    _check(c, exc, v, exc_ref, v_ref)


def _one_per_family():
    seen, out = set(), []
    for c in sc.SWEEP_CASES:
        fams = {k[0] for k in sc.expected_kernels(c)} - {"k_reduce_slabs8", "k_rho_valu", "k_vxc_valu"}
        if c.path is None and not c.env and c.aligned and fams - seen:
            seen |= fams
            out.append(c)
    return out


@pytest.mark.parametrize("c", _one_per_family(), ids=sc.case_id)
def test_plain_valu_kernels_give_the_oracle_numbers_on_the_same_inputs(dev, c):
    """An independent device answer: one case per kernel family again through path = 1 (plain-VALU kernels on dm), held
    to the oracle at the same bounds -- a difference in the case above is then the instantiation's, not the inputs'."""
    exc_ref, v_ref = sc.sweep_reference(c)
    s, exc, v = _run_sweep(c, dev, path=1)
    assert not s.get_option("used_occ") and not s.get_option("used_vxc_fringe")
    _check(c, exc, v, exc_ref, v_ref, note=False)


def _eval_ao(s, sh, coords, dev, grad, aligned=True):
    ngrid = coords.shape[0]
    d_c = _place(coords, dev)
    d_ao = _place(np.full((ngrid, sh.nao), 9.0), dev, aligned)
    d_gr = _place(np.full((3, ngrid, sh.nao), 9.0), dev, aligned) if grad else None
    assert s.eval_ao(sh, d_c, ngrid, d_ao, d_gr) == 0
    torch.cuda.synchronize()
    return d_ao, d_gr


@pytest.mark.parametrize("c", sc.AO_CASES, ids=sc.case_id)
def test_ao_case_matches_oracle(dev, c):
    sh = sc.ao_table(c.table)
    coords, _, _ = sc.grid_inputs(c)
    grad = c.xc != "LDA"
    ref = oracle.eval_ao(sh, coords, deriv=1 if grad else 0)
    ao_ref = ref[0] if grad else ref
    d_ao, d_gr = _eval_ao(_solver(c), sh, coords, dev, grad, c.aligned)
    e_ao = np.abs(d_ao.cpu().numpy() - ao_ref).max() / max(1.0, np.abs(ao_ref).max())
    e_gr = np.abs(d_gr.cpu().numpy() - ref[1]).max() / max(1.0, np.abs(ref[1]).max()) if grad else 0.0
    print(f"{sc.case_id(c):70s} dAO {e_ao:9.2e}   dgrad {e_gr:9.2e}   max|AO| {np.abs(ao_ref).max():.3g}")
    NOTED[0] += 1
    w = WORST.setdefault("k_eval_ao", [0.0, 0.0, sc.case_id(c)])
    w[0], w[1] = max(w[0], e_ao), max(w[1], e_gr)
    assert np.abs(ao_ref).max() > 0.1            # the points see the shells
    assert e_ao <= 1e-13
    assert e_gr <= 1e-12


@pytest.mark.parametrize("table,grad", sc.AO_TAB_PAIRS)
def test_shell_table_in_and_out_of_lds_agree_bitwise(dev, table, grad):
    """Tile heights 16 and 8 put the same shell table out of and into LDS (test_sweep_cases_cpu asserts that they do):
    the outputs are the same bits."""
    sh = sc.ao_table(table)
    c = sc.Case("eval_ao", "GGA" if grad else "LDA", sc.NG_AO, 0, table=table, seed=47)
    coords, _, _ = sc.grid_inputs(c)
    outs = [_eval_ao(_solver(c, ao_pt=pt), sh, coords, dev, grad) for pt in (16, 8)]
    assert torch.equal(outs[0][0], outs[1][0])
    assert not grad or torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].abs().max()) > 0.1


@pytest.mark.parametrize("c", sc.DIRECT_CASES, ids=sc.case_id)
def test_direct_case_matches_resident_call_and_oracle(dev, c):
    sh = sc.ao_table(c.table)
    coords, w, dm = sc.grid_inputs(c)
    nao, grad = sh.nao, c.xc != "LDA"
    ref = oracle.eval_ao(sh, coords, deriv=1 if grad else 0)
    exc_ref, v_ref = oracle.compute_xc(sc.oracle_type(c.xc), dm, ref[0] if grad else ref, w, ref[1] if grad else None)
    s = _solver(c)
    d_c, d_w, d_dm = _place(coords, dev), _place(w, dev), _place(dm, dev)
    d_ao, d_gr = _eval_ao(s, sh, coords, dev, grad)
    d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=dev)
    exc0 = s.compute_xc(c.ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
    v0 = d_v.cpu().numpy()
    d_v.fill_(7.0)                                                   # outputs are overwritten, not accumulated into
    d_e = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    assert s.compute_xc_direct(sh, c.ngrid, d_c, d_w, d_dm, d_v, d_e, c.chunk) == 0
    torch.cuda.synchronize()
    exc, v = float(d_e.item()), d_v.cpu().numpy()
    print(f"{sc.case_id(c):70s} against the resident call: dExc/Exc {abs(exc - exc0) / abs(exc0):9.2e}   dV/max|V| {np.abs(v - v0).max() / np.abs(v0).max():9.2e}")
    assert exc == pytest.approx(exc0, rel=1e-12)
    assert np.abs(v - v0).max() <= 1e-12 * np.abs(v0).max()
    _check(c, exc, v, exc_ref, v_ref)
    _check(c, exc0, v0, exc_ref, v_ref, note=False)


def test_worst_figures_per_family():
    """Prints (and, with QCDFT_WRITE_PROFILES, records) the worst figure of every kernel family over the cases above."""
    if not WORST:
        return            # run on its own: nothing was measured
    lines = ["# Sweep and AO kernels against the CPU oracle, every instantiation (tests/test_gpu_sweep_dispatch.py on the cases of",
             "# tests/sweep_cases.py): worst figure per kernel family.  Bars: Exc 1e-12 relative, Vxc 1e-11 max|V|; AO values 1e-13,",
             "# AO gradients 1e-12 of max(1, max|.|).  Written with QCDFT_WRITE_PROFILES=profiles."]
    for fam in sc.LEDGER_KERNELS:
        if fam in WORST:
            a, b, worst = WORST[fam]
            names = ("dAO", "dgrad") if fam == "k_eval_ao" else ("dExc/Exc", "dV/max|V|")
            lines.append(f"{fam:18s} {names[0]} {a:9.2e}   {names[1]} {b:9.2e}   worst: {worst}")
    print("\n".join(lines))
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "sweep_dispatch_parity.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
    if NOTED[0] == len(sc.ALL_CASES):            # the whole file ran
        assert set(WORST) == set(sc.LEDGER_KERNELS)
