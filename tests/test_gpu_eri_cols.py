"""DFT_EriColumns (csrc/eri_cols.hip) -- the ERI columns of a ket shell pair on the device -- against the host engine
(csrc/integrals.c::qc_eri_cols2: the product's own engine in the same McMurchie-Davidson formulation, so this file
shows that the two AGREE, not that either is right; both are compared element by element with an independent
high-precision reference in tests/test_eri_reference_cpu.py (host) and tests/test_gpu_eri_reference.py (device); the
reference takes these integrals from libcint, grid.py:65).  Every angular-momentum class up to (ff|ff), swapped shell
order, Schwarz screening, and the Cholesky factorisation built on it."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from quantum_compute_dft_amd import basis, cholesky, integrals  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _compare(sh, pairs, dev, screen=1e-14, tol=1e-12):
    host = integrals.EriColumns(sh)
    q = integrals.schwarz_bounds(sh, host.diag())
    devc = integrals.DeviceEriColumns(sh, q)
    n = sh.nao
    worst = 0.0
    for C, D in pairs:
        ref = host.cols(C, D, screen, lower_only=True)
        buf = torch.full((ref.shape[0] * n * n,), 7.0, dtype=torch.float64, device=dev)     # must be cleared by the call
        got = devc.cols(C, D, screen, buf).cpu().numpy()
        assert got.shape == ref.shape
        err = np.abs(got - ref).max()
        worst = max(worst, err)
        assert err <= tol * max(1.0, np.abs(ref).max()), (C, D, err)
    host.close(); devc.close()
    return worst


def test_every_class_up_to_ffff_on_a_ch_fragment(dev):
    syms, xyz = ["C", "H"], np.array([[0.10, -0.20, 0.05], [1.25, 0.90, 1.60]])
    sh = basis.build_shells(syms, xyz, "def2-tzvp")                     # C: 5s 3p 2d 1f, H: 3s 1p
    by_l = {l: [i for i, x in enumerate(sh.l) if x == l] for l in range(4)}
    pairs = []
    for lc in range(4):
        for ld in range(4):
            C, D = by_l[lc][0], by_l[ld][-1]
            pairs.append((C, D))
            if C != D:
                pairs.append((D, C))                                    # the swapped order of the same pair
    worst = _compare(sh, pairs, dev)
    assert worst < 1e-12


def test_benzene_def2svp_blocks_and_screening(dev):
    import os
    from quantum_compute_dft_amd import inputs
    syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
    sh = basis.build_shells(syms, xyz, "def2-svp")
    rng = np.random.default_rng(5)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, sh.nshell, size=(8, 2))]
    d = [i for i, l in enumerate(sh.l) if l == 2]
    pairs += [(d[0], d[-1]), (d[3], 0)]
    _compare(sh, pairs, dev, screen=1e-14)
    _compare(sh, pairs[:4], dev, screen=1e-6, tol=1e-12)              # the same quartets are skipped on both sides


def test_cholesky_with_device_columns_matches_host_columns(dev):
    syms, xyz = basis.parse_xyz("O 0 0 0.1173; H 0 0.7572 -0.4692; H 0 -0.7572 -0.4692")
    sh = basis.build_shells(syms, np.asarray(xyz), "def2-svp")
    La = cholesky.cholesky_eri(sh, tol=1e-10, device=dev, device_columns=True)
    Lb = cholesky.cholesky_eri(sh, tol=1e-10, device=dev, device_columns=False)
    # (the vectors themselves may differ: near-degenerate pivots are taken in another order when the columns differ in
    # the last bits; what the factorisation promises is the residual bound)
    assert abs(La.shape[0] - Lb.shape[0]) <= 2
    eri = integrals.int2e(sh)
    for L in (La, Lb):
        approx = torch.einsum("pij,pkl->ijkl", L, L).cpu().numpy()
        assert np.abs(approx - eri).max() <= 1e-9
        assert float((L - L.transpose(1, 2)).abs().max()) == 0.0 or float((L - L.transpose(1, 2)).abs().max()) < 1e-14


def test_many_pairs_in_one_call_equal_the_single_calls(dev):
    """DFT_EriColumnsMany (the Cholesky factorisation's batched steps): blocks of several ket shell pairs written back to back by
    kernels that run side by side, bit-identical to one DFT_EriColumns call per pair; the whole target range is cleared."""
    syms, xyz = ["C", "H", "O"], np.array([[0.10, -0.20, 0.05], [1.25, 0.90, 1.60], [-1.9, 0.7, -0.4]])
    sh = basis.build_shells(syms, xyz, "def2-svp")
    host = integrals.EriColumns(sh)
    devc = integrals.DeviceEriColumns(sh, integrals.schwarz_bounds(sh, host.diag()))
    host.close()
    n, ns = sh.nao, sh.nshell
    pairs = [(ns - 1, 0), (2, 2), (1, 3), (ns - 2, ns - 3), (0, 0), (4, 1)]
    nqs = [(2 * int(sh.l[C]) + 1) * (2 * int(sh.l[D]) + 1) for C, D in pairs]
    buf = torch.full((sum(nqs) * n * n,), -3.0, dtype=torch.float64, device=dev)
    many = devc.cols_many(pairs, 1e-14, buf).clone()
    assert many.shape == (sum(nqs), n, n)
    one = torch.empty((max(nqs) * n * n,), dtype=torch.float64, device=dev)
    o = 0
    for (C, D), nq in zip(pairs, nqs):
        ref = devc.cols(C, D, 1e-14, one)
        assert torch.equal(many[o:o + nq], ref), (C, D)
        o += nq
    devc.close()
