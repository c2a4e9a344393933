"""k_vxc_ws at widths of whole tiles plus 1..4 fringe lines (nao = 16 k + 1..4, option "vxc_fringe"): the matrix pipe
takes the k x k whole tiles, dealt by tile row, and the last MFMA wave accumulates the fringe lines on the vector ALU
(csrc/xc_ws_kernels.hpp, vxc_ws_mfma_fringe).  Against the CPU oracle with test_gpu_parity.py's tolerances (Exc rel 1e-12,
Vxc 1e-11 max|V| + 1e-13), and against the padded kernel of the same library (option 0): Vxc to 1e-13 max|V| (the
fringe sums run in grid order, the MFMA's four rows at a time), Exc bit for bit (the density step is the same kernel)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import quantum_compute_dft_amd as q  # noqa: E402
from helpers import synth_inputs  # noqa: E402

FRINGE_NAO = [17, 18, 20, 33, 50, 98, 114, 116]      # odd widths: the 8-byte plane loads
PADDED_NAO = [16, 21, 112, 128]                      # no fringe of 1..4 lines: the padded kernel, whatever the option says
NGRID = [1, 15, 16, 17, 4096 + 5]                    # below, at and above one sub-tile; more sub-tiles than workgroups
ORACLE_TYPE = {"LDA": 0, "GGA": 1, "pbe_x + pbe_c": 1, "B3LYP": 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(name, fringe, sweep_order=2):
    s = q.DFTSolverWrapper(q.build_library(), name)
    s.set_option("vxc_fringe", fringe)
    s.set_option("sweep_order", sweep_order)
    s.set_option("graph", 0)
    s.set_option("tiny", 0)           # widths of at most 32 functions would take the one-pass kernel instead of k_vxc_ws
    return s


def _run(s, name, dm, ao, gr, w, dev):
    ngrid, nao = ao.shape
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=dev)
    exc = s.compute_xc(ngrid, nao, t(dm), t(ao), t(w), d_v, t(gr) if name != "LDA" else None)
    torch.cuda.synchronize()
    return exc, d_v.cpu().numpy()


def _check_oracle(exc, v, exc_ref, v_ref):
    assert exc == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    assert np.abs(v - v_ref).max() <= 1e-11 * np.abs(v_ref).max() + 1e-13


def _both_variants(name, dm, ao, gr, w, dev, sweep_order, expect_fringe):
    """(exc, V) of the fringe variant after it was compared with the padded kernel."""
    out = {}
    for fringe in (0, 1):
        s = _solver(name, fringe, sweep_order)
        out[fringe] = _run(s, name, dm, ao, gr, w, dev)
        assert s.get_option("used_vxc_fringe") == float(bool(fringe) and expect_fringe)   # the kernel under test is the one that ran
    (e0, v0), (e1, v1) = out[0], out[1]
    assert e1 == e0
    assert np.abs(v1 - v0).max() <= 1e-13 * np.abs(v0).max()
    return out


@pytest.mark.parametrize("nao", FRINGE_NAO)
@pytest.mark.parametrize("name", ["GGA", "LDA"])
def test_fringe_widths_against_oracle_and_padded_kernel(dev, name, nao):
    for ngrid in NGRID:
        dm, ao, gr, w = synth_inputs(ngrid, nao, need_grad=name != "LDA", seed=4000 + 7 * nao + ngrid)
        exc_ref, v_ref = oracle.compute_xc(ORACLE_TYPE[name], dm, ao, w, gr)     # once per shape, shared by the four runs
        for sweep_order in (0, 3):
            out = _both_variants(name, dm, ao, gr, w, dev, sweep_order, expect_fringe=True)
            for exc, v in out.values():
                _check_oracle(exc, v, exc_ref, v_ref)


@pytest.mark.parametrize("nao", [50, 114])
def test_mix_functional_takes_the_fringe_variant(dev, nao):
    name = "pbe_x + pbe_c"          # a mix solver with PBE's two components: the GGA oracle's numbers
    for ngrid in (17, 4096 + 5):
        dm, ao, gr, w = synth_inputs(ngrid, nao, seed=4100 + nao + ngrid)
        exc_ref, v_ref = oracle.compute_xc(1, dm, ao, w, gr)
        out = _both_variants(name, dm, ao, gr, w, dev, 2, expect_fringe=True)
        _check_oracle(*out[1], exc_ref, v_ref)


@pytest.mark.parametrize("nao", PADDED_NAO)
def test_other_widths_keep_the_padded_kernel(dev, nao):
    for name in ("GGA", "LDA"):
        dm, ao, gr, w = synth_inputs(1000, nao, need_grad=name != "LDA", seed=4200 + nao)
        s = _solver(name, 1)
        exc, v = _run(s, name, dm, ao, gr, w, dev)
        assert s.get_option("used_vxc_fringe") == 0.0
        _check_oracle(exc, v, *oracle.compute_xc(ORACLE_TYPE[name], dm, ao, w, gr))


def test_b3lyp_keeps_the_padded_kernel(dev):
    dm, ao, gr, w = synth_inputs(1000, 114, seed=4300)
    s = _solver("B3LYP", 1)
    exc, v = _run(s, "B3LYP", dm, ao, gr, w, dev)
    assert s.get_option("used_vxc_fringe") == 0.0
    _check_oracle(exc, v, *oracle.compute_xc(2, dm, ao, w, gr))


def test_option_defaults_to_auto(dev):
    assert q.DFTSolverWrapper(q.build_library(), "GGA").get_option("vxc_fringe") == -1.0


@pytest.mark.parametrize("nao", [114, 116, 33])
@pytest.mark.parametrize("only_fringe", [True, False])
def test_fringe_lines_land_where_they_belong(dev, nao, only_fringe):
    """V[a][b] = sum_g Q[g][a] AO[g][b] with Q from AO and its gradients (GGA).  An AO plane that is zero except in the fringe
    columns leaves V non-zero in exactly the fringe COLUMNS (every row: the gradients are dense); one that is zero only
    there leaves exactly those columns zero.  A swapped, shifted or dropped fringe line changes the pattern."""
    ngrid, f0 = 1000, 16 * ((nao - 1) // 16)
    dm, ao, gr, w = synth_inputs(ngrid, nao, seed=4400 + nao)
    ao = ao.copy()
    if only_fringe:
        ao[:, :f0] = 0.0
    else:
        ao[:, f0:] = 0.0
    exc_ref, v_ref = oracle.compute_xc(1, dm, ao, w, gr)
    live = np.zeros((nao, nao), dtype=bool)
    live[:, f0:] = True
    if not only_fringe:
        live = ~live
    assert (v_ref[~live] == 0.0).all() and (np.abs(v_ref[live]) > 0.0).all()      # the case is what it claims to be
    out = _both_variants("GGA", dm, ao, gr, w, dev, 2, expect_fringe=True)
    for exc, v in out.values():
        _check_oracle(exc, v, exc_ref, v_ref)
        assert (v[~live] == 0.0).all() and (np.abs(v[live]) > 0.0).all()
