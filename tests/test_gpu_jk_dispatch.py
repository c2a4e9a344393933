"""Every kernel variant and dispatch edge of the dense (jk) and factorised (jk_factorized) Coulomb / exchange builds.

The cases are the tables of tests/jk_cases.py (what each one reaches: `note`, expected_kernels(); the CPU suite checks
the tables against the dispatch rules and the compiler's list of instantiations).  Integer cases are compared with a
plain numpy contraction by np.array_equal -- every intermediate is an integer below 2^53, so there is no tolerance;
real-valued companions are compared with the same contraction in longdouble at the project's J/K bound
|delta| <= 1e-12 max|ref| (header of tests/test_gpu_parity.py).

Notes on the cases:
* n = 102 is chosen for a 256-CU device (jsplit = 1 for K with 11 column blocks, the path of the n = 114 workload);
  with another CU count jsplit may differ and the case is then one more multi-block case.
* n > 512 (KB = 1: one k-segment per column block) cannot be tested: its ERI, 8 n^4 bytes >= 554 GB, does not fit the
  device's memory.
* with QCDFT_JSYM8_CPT unset the library picks the columns per thread of k_j_sym8 from the CU count; the three forced
  values cover every instantiation, the unset run covers the selection itself.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import jk_cases as jc  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd.grid_shard import eri_row_bounds  # noqa: E402

REL = 1e-12      # J/K bound of the real-valued cases, relative to max|ref|
FILL = 7.0       # every output holds this before a call: whatever is not written shows


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield torch.device("cuda:0")
    _DEV.clear(); _FRESH.clear()
    jc.clear_caches()
    torch.cuda.empty_cache()


_DEV = {}      # device copies of the inputs, shared between the fresh-solver tests and the one-solver test
_FRESH = {}    # results of the fresh-solver runs (numpy), by case


def _solver(**opts):
    w = q.DFTSolverWrapper(q.library_path(), "B3LYP")
    for k, v in opts.items():
        w.set_option(k, v)
    return w


def _up(a, dev, aligned=True):
    """Device copy of `a`; aligned = False: a view that starts 8 bytes into its allocation."""
    h = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if aligned:
        d = h.to(dev)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(h.numel() + 1, dtype=torch.float64, device=dev)
    assert buf.data_ptr() % 16 == 0
    d = buf[1:].view(h.shape)
    d.copy_(h)
    assert d.data_ptr() % 16 == 8 and d.is_contiguous()
    return d


def _out(n, dev):
    return torch.full((n, n), FILL, dtype=torch.float64, device=dev)


def _dense_inputs(n, dev, aligned=True):
    key = ("dense", n, aligned)
    if key not in _DEV:
        eri, dm, _, _ = jc.dense_int_case(n)
        _DEV[key] = (_up(eri, dev, aligned), _up(dm, dev))
    return _DEV[key]


def _fact_inputs(c, dev):
    key = ("fact", c.n, c.naux, c.nocc, c.aligned, c.dm_products)
    if key not in _DEV:
        chol, cocc, dm = (jc.fact_mixed_dm_case if c.dm_products == 2 else jc.fact_int_case)(c.n, c.naux, c.nocc)[:3]
        _DEV[key] = (_up(chol, dev, c.aligned), _up(dm, dev), _up(cocc, dev))
    return _DEV[key]


def _run_dense(w, n, d_eri, d_dm, dev):
    """J alone, K alone, J and K in one pass -> numpy J, K, J_joint, K_joint."""
    d_J, d_K, d_J2, d_K2 = (_out(n, dev) for _ in range(4))
    w.compute_coulomb(n, d_eri, d_dm, d_J)
    w.compute_exchange(n, d_eri, d_dm, d_K)
    w.compute_jk(n, d_eri, d_dm, d_J2, d_K2)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (d_J, d_K, d_J2, d_K2))


def _run_fact(w, c, d_L, d_dm, d_c, dev):
    """J and K together (fused dot), J alone, K alone -> numpy J_joint, K_joint, J_alone, K_alone."""
    d_J, d_K, d_J1, d_K1 = (_out(c.n, dev) for _ in range(4))
    assert w.compute_jk_factorized(c.n, c.naux, c.nocc, d_L, d_dm, d_c, d_J, d_K) == 0
    assert w.compute_jk_factorized(c.n, c.naux, c.nocc, d_L, d_dm, None, d_J1, None) == 0
    assert w.compute_jk_factorized(c.n, c.naux, c.nocc, d_L, None, d_c, None, d_K1) == 0
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (d_J, d_K, d_J1, d_K1))


def _fresh_dense(n, dev):
    if ("dense", n) not in _FRESH:
        _FRESH[("dense", n)] = _run_dense(_solver(), n, *_dense_inputs(n, dev), dev)
    return _FRESH[("dense", n)]


def _fresh_fact(c, dev):
    if c not in _FRESH:
        _FRESH[c] = _run_fact(_solver(), c, *_fact_inputs(c, dev), dev)
    return _FRESH[c]


def _check_dense(res, J_ref, K_ref):
    J, K, J2, K2 = res
    assert np.array_equal(J, J_ref), np.abs(J - J_ref).max()
    assert np.array_equal(K, K_ref), np.abs(K - K_ref).max()
    assert np.array_equal(J2, J) and np.array_equal(K2, K)          # the one-pass form, bit for bit


def _check_fact(res, J_ref, K_ref):
    J, K, J1, K1 = res
    assert np.array_equal(K, K_ref), np.abs(K - K_ref).max()
    assert np.array_equal(K1, K)                                    # K alone (DOT = false) = K of the joint call, bit for bit
    assert np.array_equal(J, J_ref), np.abs(J - J_ref).max()
    assert np.array_equal(J1, J_ref), np.abs(J1 - J_ref).max()


def _close(got, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    err = np.abs(got.astype(np.longdouble) - ref).max() / np.abs(ref).max()
    print(f"max|delta| / max|ref| = {float(err):.3e}")
    return err <= REL


# ---------------------------------------------------------------------------------------------------------------------
# dense ERI, general path (k_jk_stream)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", jc.DENSE_CASES, ids=jc.case_id)
def test_dense_jk_integer_exact(dev, c):
    _, _, J_ref, K_ref = jc.dense_int_case(c.n)
    _check_dense(_fresh_dense(c.n, dev), J_ref, K_ref)


@pytest.mark.parametrize("n", jc.DENSE_REAL_N)
def test_dense_jk_real_valued_against_longdouble(dev, n):
    eri, dm, J_ref, K_ref = jc.dense_real_case(n)
    J, K, J2, K2 = _run_dense(_solver(), n, _up(eri, dev), _up(dm, dev), dev)
    assert _close(J, J_ref) and _close(K, K_ref)
    assert np.array_equal(J2, J) and np.array_equal(K2, K)


def test_dense_jk_with_an_eri_that_is_only_8_byte_aligned(dev):
    """Even n with the ERI 8 bytes into its allocation: the 8-byte-load instantiations, same exact result."""
    c = jc.UNALIGNED_DENSE
    _, _, J_ref, K_ref = jc.dense_int_case(c.n)
    d_eri, d_dm = _dense_inputs(c.n, dev, aligned=False)
    _check_dense(_run_dense(_solver(), c.n, d_eri, d_dm, dev), J_ref, K_ref)


@pytest.mark.parametrize("c", jc.ROWS_CASES, ids=jc.case_id)
def test_dense_row_blocks_integer_exact(dev, c):
    """DFT_ComputeJKRows with i0 > 0 and more than one column block: the partial J's and the K row blocks of all ranks
    sum to the whole J and K exactly, K is zero outside a rank's rows, a J-only call gives the J of the joint call."""
    n = c.n
    eri, dm, J_ref, K_ref = jc.dense_int_case(n)
    w = _solver()
    d_dm = _up(dm, dev)
    J_sum, K_sum, covered = np.zeros((n, n)), np.zeros((n, n)), 0
    for r in range(c.world):
        lo, hi = eri_row_bounds(n, c.world, r)
        covered += hi - lo
        if hi == lo:
            continue
        i_lo, i_hi = lo // n, hi // n
        d_rows = _up(eri[lo:hi], dev)
        d_J, d_K, d_J1 = _out(n, dev), _out(n, dev), _out(n, dev)
        assert w.compute_jk_rows(n, i_lo, i_hi, d_rows, d_dm, d_J, d_K) == 0
        assert w.compute_jk_rows(n, i_lo, i_hi, d_rows, d_dm, d_J1, None) == 0
        torch.cuda.synchronize()
        K_r = d_K.cpu().numpy()
        assert np.all(K_r[:i_lo] == 0.0) and np.all(K_r[i_hi:] == 0.0)
        assert np.array_equal(K_r[i_lo:i_hi], K_ref[i_lo:i_hi])
        assert torch.equal(d_J1, d_J)
        J_sum += d_J.cpu().numpy(); K_sum += K_r
    assert covered == n * n
    assert np.array_equal(J_sum, J_ref) and np.array_equal(K_sum, K_ref)


# ---------------------------------------------------------------------------------------------------------------------
# symmetric J (k_j_sym, k_j_sym8)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", jc.SYM_CASES, ids=jc.case_id)
def test_symmetric_coulomb_integer_exact(dev, c, monkeypatch):
    """J from the upper triangle (eri_symmetric = 1) or the unique eighth (= 2; every instantiation through
    QCDFT_JSYM8_CPT, which the library reads on every call): exact, deterministic, symmetric bit for bit in mode 2,
    and nothing outside the region is read."""
    n = c.n
    if c.cpt:
        monkeypatch.setenv("QCDFT_JSYM8_CPT", str(c.cpt))
    else:
        monkeypatch.delenv("QCDFT_JSYM8_CPT", raising=False)
    eri, dm, J_ref = jc.sym_int_case(n, c.sym)
    d_eri, d_dm = _up(eri, dev), _up(dm, dev)
    w = _solver(eri_symmetric=c.sym)
    d_J, d_Jb, d_Jp = _out(n, dev), _out(n, dev), _out(n, dev)
    w.compute_coulomb(n, d_eri, d_dm, d_J)
    w.compute_coulomb(n, d_eri, d_dm, d_Jb)
    keep = torch.from_numpy(jc.sym_read_mask(n, c.sym)).to(dev)
    d_poison = torch.where(keep, d_eri, torch.full_like(d_eri, 1e3)).contiguous()
    w.compute_coulomb(n, d_poison, d_dm, d_Jp)
    torch.cuda.synchronize()
    J = d_J.cpu().numpy()
    assert np.array_equal(J, J_ref), np.abs(J - J_ref).max()
    assert torch.equal(d_Jb, d_J) and torch.equal(d_Jp, d_J)
    if c.sym == 2:
        assert torch.equal(d_J, d_J.T)


# ---------------------------------------------------------------------------------------------------------------------
# factorised J/K (k_gemm_tn)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", jc.FACT_CASES, ids=jc.case_id)
def test_factorised_jk_integer_exact(dev, c):
    J_ref, K_ref = jc.fact_int_case(c.n, c.naux, c.nocc)[3:]
    _check_fact(_fresh_fact(c, dev), J_ref, K_ref)


@pytest.mark.parametrize("nao,naux,nocc", jc.FACT_REAL)
def test_factorised_jk_real_valued_against_longdouble(dev, nao, naux, nocc):
    chol, cocc, dm, J_ref, K_ref = jc.fact_real_case(nao, naux, nocc)
    c = jc.Case("fact", nao, naux, nocc)
    J, K, J1, K1 = _run_fact(_solver(), c, _up(chol, dev), _up(dm, dev), _up(cocc, dev), dev)
    assert _close(J, J_ref) and _close(J1, J_ref) and _close(K, K_ref)
    assert np.array_equal(K1, K)


def test_factorised_j_follows_a_dm_that_is_not_the_orbital_product(dev):
    """dm = c1 c1^T + c2 c2^T with cocc = c1: J is the Coulomb matrix of dm (the fused dots are discarded on the device),
    K the exchange matrix of the orbitals -- all exact."""
    c = jc.FACT_MIXED_DM
    J_ref, K_ref = jc.fact_mixed_dm_case(c.n, c.naux, c.nocc)[3:]
    _check_fact(_run_fact(_solver(), c, *_fact_inputs(c, dev), dev), J_ref, K_ref)


def test_factorised_jk_with_vectors_that_are_only_8_byte_aligned(dev):
    c = jc.UNALIGNED_FACT
    J_ref, K_ref = jc.fact_int_case(c.n, c.naux, c.nocc)[3:]
    _check_fact(_run_fact(_solver(), c, *_fact_inputs(c, dev), dev), J_ref, K_ref)


@pytest.mark.parametrize("c", jc.KSPLIT_CASES, ids=jc.case_id)
def test_factorised_k_with_a_forced_split_of_the_contraction(dev, c):
    """Option ksplit: 8 ksplit chunks of the (P, i) rows of Yt, whatever their number -- empty chunks included."""
    J_ref, K_ref = jc.fact_int_case(c.n, c.naux, c.nocc)[3:]
    _check_fact(_run_fact(_solver(ksplit=c.ksplit), c, *_fact_inputs(c, dev), dev), J_ref, K_ref)


# ---------------------------------------------------------------------------------------------------------------------
# one solver, many shapes: the workspaces (jpart, kpart, cdy, cdc, cdv) grow on demand and are reused
# ---------------------------------------------------------------------------------------------------------------------
def _reuse_order(items):
    """Largest, smallest, then the rest with even and odd nao alternating (largest first within each parity)."""
    items = sorted(items, key=lambda it: it[1].n, reverse=True)
    first, last, rest = items[0], items[-1], items[1:-1]
    even, odd = [it for it in rest if it[1].n % 2 == 0], [it for it in rest if it[1].n % 2 == 1]
    out = [first, last]
    while even or odd:
        if even:
            out.append(even.pop(0))
        if odd:
            out.append(odd.pop(0))
    return out


def test_one_solver_through_every_shape_gives_the_fresh_solver_results(dev):
    """A buffer that is large enough is not reallocated (and the pad column of Yt is cleared only in a fresh buffer):
    results after any history of calls must equal those of a new solver bit for bit."""
    order = _reuse_order([("fact", c) for c in jc.FACT_CASES]) + _reuse_order([("dense", c) for c in jc.DENSE_CASES])
    assert [it[1].n for it in order[:2]] == [259, 5] and len(order) == len(jc.FACT_CASES) + len(jc.DENSE_CASES)
    fresh = {c: (_fresh_fact(c, dev) if kind == "fact" else _fresh_dense(c.n, dev)) for kind, c in order}
    w = _solver()
    for kind, c in order:
        if kind == "fact":
            got = _run_fact(w, c, *_fact_inputs(c, dev), dev)
        else:
            got = _run_dense(w, c.n, *_dense_inputs(c.n, dev), dev)
        for g, f in zip(got, fresh[c]):
            assert np.array_equal(g, f), (jc.case_id(c), np.abs(g - f).max())
    # and the other way round: the factorised list again on the workspaces the dense n = 102 pass left behind
    for kind, c in order[:len(jc.FACT_CASES)]:
        for g, f in zip(_run_fact(w, c, *_fact_inputs(c, dev), dev), fresh[c]):
            assert np.array_equal(g, f), (jc.case_id(c), np.abs(g - f).max())
