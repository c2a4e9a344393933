"""DFT_EvalAO (all 16 instantiations of k_eval_ao) and DFT_EvalAOHess (k_eval_ao_hess) on a real MI355X against the
100-digit reference of tests/golden/ao_ref_*.npz, element by element under the error model and the K of
tests/ao_reference_cases.py (K measured on the host, not on the kernels).  Golden files only: neither mpmath nor
oracle/ao_reference.py.  Every output buffer is pre-filled with 9.0, so a column that is not written fails.

Measured on one MI355X (profiles/ao_reference_parity.txt, "gpu" lines): worst ratio 5.16 for values and gradients (the
host's own worst element), 6.23 for Hessians, against K = 32; the whole file runs in under three seconds.

tests/test_ao_reference_cpu.py holds the runs listed in ao_reference_cases.ao_runs() against the ledger of instantiations.
With QCDFT_WRITE_PROFILES set the worst ratios are recorded as "gpu ..." lines of ao_reference_parity.txt in that directory.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import quantum_compute_dft_amd as q  # noqa: E402
import ao_reference_cases as arc  # noqa: E402
import sweep_cases as sc  # noqa: E402

FILL = 9.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _place(a, dev, aligned=True):
    """Device copy of `a`; `aligned` False: 8 bytes into its allocation (tests/test_gpu_sweep_dispatch.py)."""
    a = np.ascontiguousarray(a)
    if aligned:
        return torch.tensor(a, device=dev)
    t = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), torch.tensor(a, device=dev).reshape(-1)])[1:].view(a.shape)
    assert t.data_ptr() % 16 == 8
    return t


def _solver(ao_pt=None):
    s = q.DFTSolverWrapper(q.build_library(), "GGA")
    if ao_pt is not None:
        s.set_option("ao_pt", ao_pt)
    return s


def _eval_ao(f, dev, grad, ao_pt, aligned):
    """Device planes (1 or 4, ngrid, nao) of fixture `f`."""
    ngrid = f.points.shape[0]
    d_ao = _place(np.full((ngrid, f.sh.nao), FILL), dev, aligned)
    d_gr = _place(np.full((3, ngrid, f.sh.nao), FILL), dev, aligned) if grad else None
    assert _solver(ao_pt).eval_ao(f.sh, _place(f.points, dev), ngrid, d_ao, d_gr) == 0
    torch.cuda.synchronize()
    ao = d_ao.cpu().numpy()[None]
    return np.concatenate([ao, d_gr.cpu().numpy()]) if grad else ao


def _eval_hess(f, dev, ngrid):
    d_h = torch.full((6, ngrid, f.sh.nao), FILL, dtype=torch.float64, device=dev)
    assert _solver().eval_ao_hess(f.sh, _place(f.points[:ngrid], dev), ngrid, d_h) == 0
    torch.cuda.synchronize()
    return d_h.cpu().numpy()


def _label(name, grad, pt, aligned):
    return f"DFT_EvalAO {name} {'v+grad' if grad else 'v'} pt={pt or 'auto'}{'' if aligned else ' unaligned'}"


RESIDENT = sorted({(n, g, al) for n, g, pt, al in arc.ao_runs() if not n.startswith("s_")})


@pytest.mark.parametrize("name,grad,aligned", RESIDENT, ids=lambda v: str(v))
def test_eval_ao_matches_the_reference_at_both_tile_heights(dev, name, grad, aligned):
    """P (even and odd nao), C, T: the eight TAB = true instantiations.  On C also the ballot skip: of the 32 leading points
    all but 5 and 29 lie beyond every cut -- exact zeros there and at the point 60 bohr away, the two near points in the
    same waves pass the check."""
    f = arc.load(name)
    wanted = [0, 1, 2, 3] if grad else [0]
    A, CUT = arc.scales_for(name, wanted)
    out = {}
    for pt in (16, 8):
        assert (name, grad, pt, aligned) in arc.ao_runs()
        got = _eval_ao(f, dev, grad, pt, aligned)
        assert not np.any(got == FILL), "an element was not written"
        arc.check(f, f.take(got, wanted), wanted, A, CUT, _label(name, grad, pt, aligned), tag="gpu", group=f"k_eval_ao in LDS, {name}")
        out[pt] = got
    assert np.array_equal(out[16], out[8]), "tile heights 16 and 8 differ"
    if name == "c":
        far = [g for g in f.extra["run"] if g not in f.extra["near"]] + [int(np.ravel(f.extra["far_point"])[0])]
        assert len(far) == 31 and np.all(out[16][:, far, :] == 0.0)
        assert np.abs(out[16][0][f.extra["near"]]).max() > 0.05


S_RUNS = [r for r in arc.ao_runs() if r[0].startswith("s_")]


@pytest.mark.parametrize("name,grad,pt,aligned", S_RUNS, ids=lambda v: str(v))
def test_eval_ao_matches_the_reference_on_the_sampled_tables(dev, name, grad, pt, aligned):
    """The AO cases' own (table, planes, tile height, alignment): the eight TAB = false instantiations, the odd seam, the
    misaligned 8-byte stores; checked at the sampled columns, every row."""
    f = arc.load(name)
    wanted = [0, 1, 2, 3] if grad else [0]
    A, CUT = arc.scales_for(name, wanted)
    got = _eval_ao(f, dev, grad, pt, aligned)
    assert not np.any(got == FILL), "an element was not written"
    where = "in" if sc.ao_kernel(f.sh, grad, pt, aligned)[1][3] else "out of"
    arc.check(f, f.take(got, wanted), wanted, A, CUT, _label(name, grad, pt, aligned), tag="gpu", group=f"k_eval_ao {where} LDS, {name}")


@pytest.mark.parametrize("name", ["p_even", "p_odd", "c", "t", "h_" + arc.H_TABLE])
def test_eval_ao_hess_matches_the_reference(dev, name):
    f = arc.load(name)
    wanted = [4, 5, 6, 7, 8, 9]
    A, CUT = arc.scales_for(name, wanted)
    got = _eval_hess(f, dev, f.points.shape[0])
    assert not np.any(got == FILL), "an element was not written"
    arc.check(f, f.take(got, wanted), wanted, A, CUT, f"DFT_EvalAOHess {name}", tag="gpu", group=f"k_eval_ao_hess, {name}")
    if name == "c":
        far = [g for g in f.extra["run"] if g not in f.extra["near"]] + [int(np.ravel(f.extra["far_point"])[0])]
        assert np.all(got[:, far, :] == 0.0)


@pytest.mark.parametrize("name", ["p_odd", "h_" + arc.H_TABLE])
def test_eval_ao_hess_of_one_point(dev, name):
    """ngrid = 1 (the other runs: 99, 63, 43 points, no multiple of 8): the first stored point alone gives the bits of
    the full run's first row, and passes the check."""
    f = arc.load(name)
    wanted = [4, 5, 6, 7, 8, 9]
    A, CUT = arc.scales_for(name, wanted)
    one, full = _eval_hess(f, dev, 1), _eval_hess(f, dev, f.points.shape[0])
    assert f.points.shape[0] % 8 != 0 and np.array_equal(one[:, 0], full[:, 0])
    got = np.concatenate([one, full[:, 1:]], axis=1)
    arc.check(f, f.take(got, wanted), wanted, A, CUT, f"DFT_EvalAOHess {name} ngrid=1")
