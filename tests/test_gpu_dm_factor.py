"""DFT_FactorDensity and option "dm_factor" on the GPU (csrc/dm_factor.hip): the factor against the acceptance bound
and the numpy restatement (tests/dm_factor_reference.py), everything that must be rejected, the sweep of DFT_ComputeXC
through the factor against the CPU oracle (tolerances of test_gpu_occ.py: Exc rel 1e-12, Vxc 1e-11 max|V|), bit-equal
fallbacks, the entries the option must leave alone, the exchange matrix from the factor, and an SCF run end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import quantum_compute_dft_amd as q  # noqa: E402
from dm_factor_reference import (FACTOR_SHAPES, INCONSISTENT, NOT_PSD, RANK_EXCEEDED, SIZE, consistency_bound,  # noqa: E402
                                 factor_case, occ_inputs, pivoted_cholesky, s_orthonormal_density)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "LDA", 1: "GGA", 2: "B3LYP"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(xc_type=0, **opts):
    s = q.DFTSolverWrapper(q.build_library(), NAMES[xc_type])
    for k, v in opts.items():
        s.set_option(k, v)
    return s


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _assert_factor(dm, got, rank):
    L, r = got
    L = L.cpu().numpy()
    assert r == rank and L.shape == (dm.shape[0], rank)
    err, bound = np.abs(dm - L @ L.T), consistency_bound(dm, L)
    print(f"nao {dm.shape[0]} rank {r}: max |dm - L L^T| / bound = {(err / bound).max():.3e}")
    assert np.all(err <= bound)


# ---- the factor --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nao,nocc", FACTOR_SHAPES)
def test_factor_recovers_the_occupied_rank(dev, nao, nocc):
    _, dm = factor_case(nao, nocc)
    s = _solver()
    d_dm = _t(dm, dev)
    got = s.factor_density(d_dm)
    assert got is not None, s.factor_info
    _assert_factor(dm, got, nocc)
    assert s.factor_info[0] == nocc and s.factor_info[2] == 0 and s.factor_info[3] == np.diag(dm).max()
    assert s.factor_info[1] <= 1e-13
    again = s.factor_density(d_dm)                      # the same bits every run
    assert again[1] == got[1] and torch.equal(again[0], got[0])
    assert pivoted_cholesky(dm)[1]["rank"] == got[1]    # seeded inputs: no ties, the restatement takes the same steps


def test_factor_of_s_orthonormal_orbitals_in_an_ill_conditioned_basis(dev):
    dm, _ = s_orthonormal_density(246, 47, 1e6, seed=31)
    s = _solver()
    got = s.factor_density(_t(dm, dev))
    assert got is not None, s.factor_info
    _assert_factor(dm, got, 47)


def test_damped_mix_of_two_densities(dev):
    c1 = occ_inputs(1, 50, 10, seed=11)[0]
    c2 = occ_inputs(1, 50, 10, seed=12)[0]
    dm = 0.7 * c1 @ c1.T + 0.3 * c2 @ c2.T
    s = _solver()
    got = s.factor_density(_t(dm, dev))
    assert got is not None, s.factor_info
    _assert_factor(dm, got, 20)


def _rejects():
    c, dm, *_ = occ_inputs(1, 50, 10, seed=5)
    nonsym = dm.copy(); nonsym[3, 17] += 1e-6
    c30 = occ_inputs(1, 50, 30, seed=6)[0]
    nan = dm.copy(); nan[7, 9] = nan[9, 7] = np.nan
    return {"non-symmetric": (nonsym, INCONSISTENT), "indefinite": (dm - 1.5 * np.outer(c[:, 0], c[:, 0]), NOT_PSD),
            "rank 30 of 50": (c30 @ c30.T, RANK_EXCEEDED), "zero": (np.zeros((50, 50)), NOT_PSD), "NaN": (nan, None),
            "all NaN": (np.full((50, 50), np.nan), None), "nao 1": (np.ones((1, 1)), SIZE)}


@pytest.mark.parametrize("case", ["non-symmetric", "indefinite", "rank 30 of 50", "zero", "NaN", "all NaN", "nao 1"])
def test_rejections_return_zero_and_terminate(dev, case):
    dm, reason = _rejects()[case]
    s = _solver()
    assert s.factor_density(_t(dm, dev)) is None
    assert s.last_error() == ""
    if reason is not None:
        assert s.factor_info[2] == reason, s.factor_info
    assert s.factor_info[2] == pivoted_cholesky(dm)[1]["reason"] or reason is None
    if case == "rank 30 of 50":                         # ... and with room for it the same matrix factorises
        _assert_factor(dm, s.factor_density(_t(dm, dev), max_rank=30), 30)


def test_bad_arguments_are_errors_not_aborts(dev):
    s = _solver()
    buf = torch.zeros(64, dtype=torch.float64, device=dev)
    assert s.lib.DFT_FactorDensity(s.solver, 8, 0, 0, 0.0, buf.data_ptr(), None) == -1
    assert "bad arguments" in s.last_error()
    assert s.lib.DFT_FactorDensity(s.solver, -3, buf.data_ptr(), 0, 0.0, buf.data_ptr(), None) == -1


# ---- the sweep through the factor ----------------------------------------------------------------------------------
def _run(s, xc_type, dm, ao, gr, w, dev, entry="sync"):
    ngrid, nao = ao.shape
    d_dm, d_ao, d_w = _t(dm, dev), _t(ao, dev), _t(w, dev)
    d_gr = _t(gr, dev) if xc_type else None
    d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=dev)
    if entry == "async":
        d_e = torch.zeros(1, dtype=torch.float64, device=dev)
        assert s.compute_xc_async(ngrid, nao, d_dm, d_ao, d_w, d_v, d_e, d_gr) == 0
        torch.cuda.synchronize()
        return float(d_e.item()), d_v.cpu().numpy()
    exc = s.lib.DFT_ComputeXC(s.solver, ngrid, nao, d_dm.data_ptr(), d_ao.data_ptr(), d_gr.data_ptr() if xc_type else 0,
                              d_w.data_ptr(), d_v.data_ptr())       # the reference's own symbol
    s._check()
    torch.cuda.synchronize()
    return exc, d_v.cpu().numpy()


def _check(exc, v, exc_ref, v_ref):
    assert exc == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    assert np.abs(v - v_ref).max() <= 1e-11 * np.abs(v_ref).max() + 1e-13


@functools.lru_cache(maxsize=None)
def _sweep_inputs(ngrid, nao, nocc):
    return occ_inputs(ngrid, nao, nocc, seed=4000 + ngrid + nao + nocc)


SWEEP_SHAPES = [(257, 13, 3), (2500, 114, 21), (700, 129, 26), (1111, 246, 47), (130, 494, 47), (200, 610, 250)]


@pytest.mark.parametrize("ngrid,nao,nocc", SWEEP_SHAPES)
@pytest.mark.parametrize("xc_type", [0, 1, 2])
def test_sweep_through_the_factor_matches_oracle(dev, xc_type, ngrid, nao, nocc):
    _, dm, ao, gr, w = _sweep_inputs(ngrid, nao, nocc)
    exc_ref, v_ref = oracle.compute_xc(xc_type, dm, ao, w, gr if xc_type else None)
    s = _solver(xc_type, dm_factor=1, occ=1, tiny=0)
    exc, v = _run(s, xc_type, dm, ao, gr, w, dev)
    print(f"Exc rel err {abs(exc - exc_ref) / abs(exc_ref):.2e}, Vxc err / max|V| {np.abs(v - v_ref).max() / np.abs(v_ref).max():.2e}")
    _check(exc, v, exc_ref, v_ref)
    assert s.get_option("used_dm_factor") == 1 and s.get_option("used_occ") == 1 and s.get_option("dm_factor_rank") == nocc


def test_auto_rule_follows_occ_plan(dev):
    """occ = 0: the factor is swept where the occupied form does clearly fewer MFMAs at its rank; occ = 2: never."""
    for (ngrid, nao, nocc), taken in (((800, 246, 47), 1), ((800, 160, 90), 0)):
        _, dm, ao, gr, w = occ_inputs(ngrid, nao, nocc, seed=77 + nao)
        exc0, v0 = _run(_solver(1), 1, dm, ao, gr, w, dev)
        s = _solver(1, dm_factor=1)
        exc, v = _run(s, 1, dm, ao, gr, w, dev)
        assert s.get_option("used_dm_factor") == taken and s.get_option("used_occ") == taken
        assert s.get_option("dm_factor_rank") == (nocc if taken else 0)      # 90 of 160: above nao / 2, rejected
        _check(exc, v, exc0, v0)
        if not taken:
            assert exc == exc0 and np.array_equal(v, v0)
        s = _solver(1, dm_factor=1, occ=2)
        exc, v = _run(s, 1, dm, ao, gr, w, dev)
        assert s.get_option("used_dm_factor") == 0 and s.get_option("used_occ") == 0
        assert exc == exc0 and np.array_equal(v, v0)


@pytest.mark.parametrize("kind", ["non-symmetric", "full rank", "indefinite"])
def test_fallback_is_bit_equal(dev, kind):
    ngrid, nao, nocc = 700, 129, 26
    c, dm, ao, gr, w = occ_inputs(ngrid, nao, nocc, seed=91)
    if kind == "non-symmetric":
        dm = dm.copy(); dm[5, 77] += 1e-6
    elif kind == "full rank":
        a = np.random.default_rng(92).standard_normal((nao, nao))
        dm = a @ a.T / nao
    else:
        dm = dm - 1.5 * np.outer(c[:, 0], c[:, 0])
    for xc_type in (0, 1):
        exc0, v0 = _run(_solver(xc_type, occ=1), xc_type, dm, ao, gr, w, dev)
        s = _solver(xc_type, occ=1, dm_factor=1)
        exc, v = _run(s, xc_type, dm, ao, gr, w, dev)
        assert s.get_option("used_dm_factor") == 0 and s.get_option("dm_factor_rank") == 0
        assert exc == exc0 and np.array_equal(v, v0)


def test_other_entries_and_the_tiny_plan_are_untouched(dev):
    _, dm, ao, gr, w = occ_inputs(2500, 114, 21, seed=93)
    outs = [_run(_solver(1, dm_factor=o, occ=1), 1, dm, ao, gr, w, dev, entry="async") for o in (0, 1)]
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1])
    _, dm, ao, gr, w = occ_inputs(1000, 16, 5, seed=94)                      # the one-pass plan (default "tiny")
    for xc_type in (0, 2):
        exc0, v0 = _run(_solver(xc_type), xc_type, dm, ao, gr, w, dev)
        s = _solver(xc_type, dm_factor=1, occ=1)
        exc, v = _run(s, xc_type, dm, ao, gr, w, dev)
        assert s.get_option("used_dm_factor") == 0 and exc == exc0 and np.array_equal(v, v0)


def test_repeated_calls_and_timings(dev):
    """The same pointers again and again (where option 0 would replay a graph): the same bits, and with "profile" the
    factor kernels in front of the sweep's."""
    ngrid, nao, nocc = 2500, 114, 21
    _, dm, ao, gr, w = _sweep_inputs(ngrid, nao, nocc)
    s = _solver(1, dm_factor=1)
    d_dm, d_ao, d_w, d_gr = _t(dm, dev), _t(ao, dev), _t(w, dev), _t(gr, dev)
    d_v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
    res = []
    for _ in range(4):
        d_v.zero_()
        res.append((s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr), d_v.clone()))
        assert s.get_option("used_dm_factor") == 1
    assert all(r[0] == res[0][0] and torch.equal(r[1], res[0][1]) for r in res)
    s.set_option("profile", 1)
    s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
    names = [n for n, _ in s.timings()]
    assert names[:3] == ["dm_factor", "dm_factor_check", "rho_occ"], names
    s.factor_density(d_dm)
    assert [n for n, _ in s.timings()] == ["dm_factor", "dm_factor_check"]


def test_default_is_off_and_the_environment_turns_it_on():
    assert _solver().get_option("dm_factor") == 0
    code = ("import quantum_compute_dft_amd as q; s = q.DFTSolverWrapper(q.library_path(), 'LDA'); "
            "print('dm_factor', int(s.get_option('dm_factor')))")
    for value, want in (("1", 1), ("0", 0)):
        env = dict(os.environ, QCDFT_DM_FACTOR=value, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert f"dm_factor {want}" in out.stdout


# ---- exchange from the factor --------------------------------------------------------------------------------------
def test_exchange_from_the_factor(dev):
    naux, nao, nocc = 8, 40, 7
    rng = np.random.default_rng(95)
    a = 0.3 * rng.standard_normal((naux, nao, nao))
    chol = 0.5 * (a + a.transpose(0, 2, 1))
    cocc = np.sqrt(2.0) * 0.7 * rng.standard_normal((nao, nocc))
    dm = cocc @ cocc.T
    s = _solver()
    d_chol, d_dm = _t(chol, dev), _t(dm, dev)
    got = s.factor_density(d_dm)
    assert got is not None and got[1] == nocc
    K = []
    for c, n in ((_t(cocc, dev), nocc), got):
        d_K = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
        assert s.compute_jk_factorized(nao, naux, n, d_chol, d_dm, c, None, d_K) == 0
        torch.cuda.synchronize()
        K.append(d_K.cpu().numpy())
    assert np.abs(K[1] - K[0]).max() <= 1e-11 * np.abs(K[0]).max()


# ---- an SCF run ----------------------------------------------------------------------------------------------------
def test_scf_with_the_reference_call_and_the_option(dev):
    """H2O / def2-SVP, the host loop with the reference's DFT_ComputeXC(dm): with the option every cycle's sweep runs
    through the factor of the loop's dm (LDA: 8 against 16 MFMAs per 16 grid rows at 24 functions, 5 occupied)."""
    from quantum_compute_dft_amd import inputs, scf
    inp = inputs.build("H2O", "def2-svp", 3, verbose=False)
    res = {}
    for on in (False, True):
        be = scf.HipBackend(inp, "LDA", xc_occ=False, dm_factor=on)
        be.solver.set_option("tiny", 0)
        res[on] = scf.run_scf(inp, be, "LDA", log=None)
        assert be.solver.get_option("used_dm_factor") == (1 if on else 0)
        assert be.solver.get_option("dm_factor_rank") == (inp.nocc if on else 0)
    assert res[True]["converged"] and res[False]["converged"]
    print("E_tot", res[False]["E_tot"], res[True]["E_tot"], "cycles", res[False]["cycles"], res[True]["cycles"])
    assert abs(res[True]["E_tot"] - res[False]["E_tot"]) <= 1e-9
    assert res[True]["cycles"] == res[False]["cycles"]
