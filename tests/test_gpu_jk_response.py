"""DFT_ComputeJKFactorizedResponse: J_k = J[A B_k^T + B_k A^T] and M_k = sum_P (L_P A)(L_P B_k)^T of several trials from
Cholesky vectors, and the dense entry the excitation solver relies on for an antisymmetric dm.

Integer cases (generators and magnitude limits of tests/jk_cases.py: |L| <= 3, |A|, |B| <= 2) are compared bitwise with
int64 numpy arithmetic.  The largest intermediate is J: naux terms v_P L_P with |v_P| <= nao^2 * 3 * (2 * nocc * 4), below
naux * nocc * (6 nao)^2 ~ 1.5e8 at the largest case, far below 2^53, and M's naux * nocc * (6 nao)^2 is the same figure:
every summation order gives the same bits.  The cases sit on both sides of every half-transform tier (nocc 16|17, 32|33,
48|49, 64|65), take both parities of nao (16-byte and 8-byte loads of L) and nvec on both sides of the 8-trial group.
Real-valued cases go against numpy at 1e-12 of max|ref|, the bound of the existing factorised tests.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import jk_cases as jc  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402

FILL = 7.0
INT_CASES = [(17, 5, 3, 1), (33, 7, 16, 3), (34, 6, 17, 8), (64, 5, 32, 2), (65, 4, 33, 9), (96, 6, 48, 4), (97, 6, 49, 2),
             (66, 3, 64, 1), (67, 3, 65, 2)]
REAL_CASES = [(97, 6, 57, 5), (141, 3, 129, 2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    yield torch.device("cuda:0")
    int_case.cache_clear(); real_case.cache_clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def solver(dev):
    return q.DFTSolverWrapper(q.library_path(), "B3LYP")


def reference(chol, A, Bs):
    """J (nvec, nao, nao) and M (nvec, nao, nao) in the dtype of the inputs."""
    AB = np.einsum("mi,kni->kmn", A, Bs)
    D = AB + AB.transpose(0, 2, 1)
    v = np.einsum("pij,kij->kp", chol, D)
    J = np.einsum("kp,pij->kij", v, chol)
    LA = np.einsum("pmn,ni->pmi", chol, A)
    M = np.stack([np.einsum("pmi,pni->mn", LA, np.einsum("pmn,ni->pmi", chol, B)) for B in Bs])
    return J, M


@functools.lru_cache(maxsize=None)
def int_case(nao, naux, nocc, nvec):
    rng = np.random.default_rng(7400 + 1000 * nao + 10 * nocc + nvec)
    chol, A = jc._int_factors(rng, nao, naux, nocc)
    Bs = jc._ints(rng, -jc.C_MAX, jc.C_MAX, (nvec, nao, nocc))
    J, M = reference(chol.astype(np.int64), A.astype(np.int64), Bs.astype(np.int64))
    assert max(np.abs(J).max(), np.abs(M).max()) < 2 ** 53 and naux * nocc * (6 * nao) ** 2 < 2 ** 53
    return chol, A, Bs, J.astype(np.float64), M.astype(np.float64)


@functools.lru_cache(maxsize=None)
def real_case(nao, naux, nocc, nvec):
    rng = np.random.default_rng(300 + nao)
    X = rng.normal(0, 0.3, (naux, nao, nao))
    chol = 0.5 * (X + X.transpose(0, 2, 1))
    A, Bs = rng.normal(0, 0.7, (nao, nocc)), rng.normal(0, 0.7, (nvec, nao, nocc))
    return (chol, A, Bs) + reference(chol, A, Bs)


def up(a, dev, aligned=True):
    h = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    if aligned:
        d = h.to(dev)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(h.numel() + 1, dtype=torch.float64, device=dev)
    d = buf[1:].view(h.shape)
    d.copy_(h)
    assert d.data_ptr() % 16 == 8 and d.is_contiguous()
    return d


class Guarded:
    """An (nvec, nao, nao) output with one guard row of FILL before and after it."""

    def __init__(self, nvec, nao, dev):
        self.buf = torch.full((nvec * nao + 2, nao), FILL, dtype=torch.float64, device=dev)
        self.out = self.buf[1:-1].view(nvec, nao, nao)

    def host(self):
        h = self.buf.cpu().numpy()
        assert np.all(h[0] == FILL) and np.all(h[-1] == FILL), "a guard row was written"
        return h[1:-1].reshape(self.out.shape)


def run(solver, dev, chol, A, Bs, aligned=True):
    """J and M together, J alone, M alone -> numpy J, M, J_alone, M_alone (guard rows checked)."""
    nvec, nao, nocc = Bs.shape
    d_L, d_A, d_B = up(chol, dev, aligned), up(A, dev), up(Bs, dev)
    g = [Guarded(nvec, nao, dev) for _ in range(4)]
    args = (nao, chol.shape[0], nocc, nvec, d_L, d_A, d_B)
    assert solver.compute_jk_factorized_response(*args, g[0].out, g[1].out) == 0
    assert solver.compute_jk_factorized_response(*args, g[2].out, None) == 0
    assert solver.compute_jk_factorized_response(*args, None, g[3].out) == 0
    torch.cuda.synchronize()
    return tuple(x.host() for x in g)


@pytest.mark.parametrize("case", INT_CASES, ids=lambda c: "n%d-naux%d-nocc%d-nvec%d" % c)
def test_integer_cases_are_bitwise_the_int64_contraction(solver, dev, case):
    chol, A, Bs, J, M = int_case(*case)
    got = run(solver, dev, chol, A, Bs)
    for name, g, ref in (("J", got[0], J), ("M", got[1], M), ("J alone", got[2], J), ("M alone", got[3], M)):
        assert np.array_equal(g, ref), (name, case, float(np.abs(g - ref).max()))
    assert not np.array_equal(M, M.transpose(0, 2, 1))            # M is not symmetric: every tile is computed, none mirrored


def test_vectors_eight_bytes_into_their_allocation(solver, dev):
    chol, A, Bs, J, M = int_case(34, 6, 17, 8)
    got = run(solver, dev, chol, A, Bs, aligned=False)
    assert np.array_equal(got[0], J) and np.array_equal(got[1], M) and np.array_equal(got[2], J) and np.array_equal(got[3], M)


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: "n%d-naux%d-nocc%d-nvec%d" % c)
def test_real_cases_match_numpy(solver, dev, case):
    chol, A, Bs, J, M = real_case(*case)
    got = run(solver, dev, chol, A, Bs)
    for name, g, ref in (("J", got[0], J), ("M", got[1], M), ("J alone", got[2], J), ("M alone", got[3], M)):
        err = float(np.abs(g - ref).max() / np.abs(ref).max())
        print(f"{name} {case}: {err:.2e}")
        assert err <= 1e-12, (name, case, err)
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[1], got[3])


def test_a_trial_is_bitwise_the_same_alone_and_in_any_batch(solver, dev):
    nao, naux, nocc = 97, 6, 57
    chol, A, _, _, _ = real_case(nao, naux, nocc, 5)
    Bs = np.random.default_rng(11).normal(0, 0.7, (9, nao, nocc))
    J9, M9, _, _ = run(solver, dev, chol, A, Bs)
    J3, M3, _, _ = run(solver, dev, chol, A, Bs[:3])
    assert np.array_equal(J3, J9[:3]) and np.array_equal(M3, M9[:3])
    for k in (0, 2, 8):                                               # first of a group, inside it, the lone ninth
        J1, M1, _, _ = run(solver, dev, chol, A, Bs[k:k + 1])
        assert np.array_equal(J1[0], J9[k]) and np.array_equal(M1[0], M9[k]), k


def test_bad_arguments_return_an_error_and_nothing_wanted_is_no_work(solver, dev):
    chol, A, Bs, _, _ = int_case(17, 5, 3, 1)
    d_L, d_A, d_B = up(chol, dev), up(A, dev), up(Bs, dev)
    g = Guarded(1, 17, dev)
    good = dict(nao=17, naux=5, nocc=3, nvec=1)
    for key in good:
        for bad in (0, -1):
            a = dict(good, **{key: bad})
            with pytest.raises(RuntimeError, match="bad sizes"):
                solver.compute_jk_factorized_response(a["nao"], a["naux"], a["nocc"], a["nvec"], d_L, d_A, d_B, g.out, None)
    for ptrs in ((None, d_A, d_B), (d_L, None, d_B), (d_L, d_A, None)):
        with pytest.raises(RuntimeError, match="needs the vectors and both factors"):
            solver.compute_jk_factorized_response(17, 5, 3, 1, *ptrs, g.out, None)
    assert solver.compute_jk_factorized_response(17, 5, 3, 1, d_L, d_A, d_B, None, None) == 0
    torch.cuda.synchronize()
    assert np.all(g.host() == FILL) and solver.last_error() == ""


def test_timings_name_the_new_stages(dev):
    w = q.DFTSolverWrapper(q.library_path(), "B3LYP")
    w.set_option("profile", 1)
    chol, A, Bs, _, _ = int_case(33, 7, 16, 3)
    g = [Guarded(3, 33, dev) for _ in range(2)]
    assert w.compute_jk_factorized_response(33, 7, 16, 3, up(chol, dev), up(A, dev), up(Bs, dev), g[0].out, g[1].out) == 0
    torch.cuda.synchronize()
    names = [n for n, _ in w.timings()]
    assert names == ["cdr_half", "cdr_dot", "cdr_j", "cdr_m"], names


@pytest.mark.parametrize("n", [33, 64])
def test_dense_exchange_of_an_antisymmetric_dm_is_the_einsum(solver, dev, n):
    """DFT_ComputeJK's K is the literal einsum for ANY dm: what the dense path of excitation_parts relies on."""
    eri, dm, _, _ = jc.dense_int_case(n)
    dm = dm - dm.T                                                     # |dm| <= 8: K below n^2 * 8 * 8 ~ 2.6e5
    K = np.einsum("ijkl,jl->ik", eri.reshape(n, n, n, n).astype(np.int64), dm.astype(np.int64)).astype(np.float64)
    d_K = torch.full((n, n), FILL, dtype=torch.float64, device=dev)
    solver.compute_jk(n, up(eri, dev), up(dm, dev), None, d_K)
    torch.cuda.synchronize()
    assert np.array_equal(d_K.cpu().numpy(), K) and not np.array_equal(K, K.T)
