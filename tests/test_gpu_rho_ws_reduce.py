"""The density kernel of nao <= 128 (k_rho_ws, csrc/xc_ws_kernels.hpp) with its row sums finished on the
matrix waves: loader threads leave 16 partial sums per grid row in LDS, an MFMA wave adds them one step
later and the result ring is flushed one barrier later than before.  What can go wrong is in the seams:
tile counts with an unowned half column group (odd NT), grids with fewer sub-tiles than workgroups or a
partial last one, the burst flush (more than 16 sub-tiles per workgroup) and its drain, and the
independence of a point's density from the step that handled it.

Bounds as in test_gpu_parity.py (fp64 round-off; the 16-term sums are taken in another order than the
oracle's): Exc |rel| <= 1e-12, Vxc |abs| <= 1e-11 max|V| + 1e-13.  tiny = 0 everywhere, so that bases
of at most 32 functions take this kernel too.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import quantum_compute_dft_amd as q  # noqa: E402
from helpers import synth_inputs  # noqa: E402

NAMES = {0: "LDA", 1: "GGA", 2: "B3LYP"}
BENCH_SHAPE = (143556, 114)   # Benzene / def2-SVP: 35 sub-tiles per workgroup on 256 CUs, two burst flushes


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(xc_type, **opts):
    w = q.DFTSolverWrapper(q.build_library(), NAMES[xc_type])
    for k, v in opts.items():
        w.set_option(k, v)
    return w


def _run(w, dm, ao, gr, wts, dev):
    ngrid, nao = ao.shape
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    d_dm, d_ao, d_gr, d_w = t(dm), t(ao), t(gr), t(wts)
    d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=dev)  # must be overwritten
    exc = w.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
    torch.cuda.synchronize()
    return exc, d_v.cpu().numpy()


def _check(exc, v, exc_ref, v_ref):
    assert exc == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    scale = np.abs(v_ref).max()
    assert np.abs(v - v_ref).max() <= 1e-11 * scale + 1e-13


@pytest.mark.parametrize("nao", [1, 7, 16, 17, 33, 48, 63, 80, 97, 112, 114, 127, 128])
@pytest.mark.parametrize("xc_type", [0, 1, 2])
def test_every_tile_count_matches_oracle(dev, xc_type, nao):
    """NT = 1..8; odd nao takes the 8-byte loads.  5003 points: 313 sub-tiles, a partial last one, one or two per workgroup."""
    dm, ao, gr, w = synth_inputs(5003, nao, seed=4100 + nao)
    exc_ref, v_ref = oracle.compute_xc(xc_type, dm, ao, w, gr)
    exc, v = _run(_solver(xc_type, tiny=0), dm, ao, gr if xc_type else None, w, dev)
    _check(exc, v, exc_ref, v_ref)


@pytest.mark.parametrize("ngrid", [1, 15, 16, 17, 16 * 256 - 1, 16 * 256 + 1, 20011])
@pytest.mark.parametrize("nao", [17, 114])
@pytest.mark.parametrize("xc_type", [0, 1, 2])
def test_ragged_and_tiny_grids_match_oracle(dev, xc_type, nao, ngrid):
    """Fewer sub-tiles than workgroups, one each, one more than that, a partial last tile."""
    dm, ao, gr, w = synth_inputs(ngrid, nao, seed=4300 + ngrid % 1000 + nao)
    exc_ref, v_ref = oracle.compute_xc(xc_type, dm, ao, w, gr)
    for order in (0, 3):
        exc, v = _run(_solver(xc_type, tiny=0, sweep_order=order), dm, ao, gr if xc_type else None, w, dev)
        _check(exc, v, exc_ref, v_ref)


@pytest.fixture(scope="module")
def bench_case():
    ngrid, nao = BENCH_SHAPE
    dm, ao, gr, w = synth_inputs(ngrid, nao, seed=4500)
    return dm, ao, gr, w, oracle.compute_xc(1, dm, ao, w, gr, omp=True)


def test_burst_flush_at_the_bench_shape_matches_oracle(dev, bench_case):
    """More than WS_OT = 16 sub-tiles per workgroup: the results leave in bursts while the sweep goes on."""
    dm, ao, gr, w, (exc_ref, v_ref) = bench_case
    exc, v = _run(_solver(1, tiny=0), dm, ao, gr, w, dev)
    _check(exc, v, exc_ref, v_ref)


@pytest.mark.parametrize("shape", [(20011, 114), BENCH_SHAPE], ids=["20011x114", "bench"])
def test_exc_is_bit_identical_across_walking_orders_and_calls(dev, bench_case, shape):
    """rho of a point depends on its row and its place in the 16-row sub-tile only, never on the workgroup, the step
    or the LDS slot that handled it; and nothing in the kernel is left over from the call before."""
    dm, ao, gr, w = bench_case[:4] if shape == BENCH_SHAPE else synth_inputs(*shape, seed=61)
    s0 = _solver(1, tiny=0, sweep_order=0)
    first = _run(s0, dm, ao, gr, w, dev)
    again = _run(s0, dm, ao, gr, w, dev)
    assert again[0] == first[0]
    assert np.array_equal(again[1], first[1])
    for order in (1, 2, 3):
        got = _run(_solver(1, tiny=0, sweep_order=order), dm, ao, gr, w, dev)
        assert got[0] == first[0], order


@pytest.mark.parametrize("ngrid,nao", [(5003, 33), (20011, 114), (4097, 128)])
@pytest.mark.parametrize("xc_type", [0, 1, 2])
def test_plain_valu_validation_path_agrees(dev, xc_type, ngrid, nao):
    """path = 1: the first-generation kernels, no MFMA, no wave roles -- an independent device-side answer."""
    dm, ao, gr, w = synth_inputs(ngrid, nao, seed=4700 + nao)
    ref = _run(_solver(xc_type, path=1), dm, ao, gr if xc_type else None, w, dev)
    got = _run(_solver(xc_type, tiny=0), dm, ao, gr if xc_type else None, w, dev)
    _check(got[0], got[1], ref[0], ref[1])
