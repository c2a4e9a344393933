"""CPU side of the J/K dispatch tests: the case tables of tests/jk_cases.py are what tests/test_gpu_jk_dispatch.py runs.

* every integer case stays below 2^53 in every intermediate, so exact equality is the right GPU assertion;
* the integer references equal the oracle's coulomb / exchange / jk_from_factors exactly (not only self-consistent);
* the edges the tables claim (column blocks, stages, tiers) are the ones the dispatch rules give;
* coverage ledger: every instantiation of k_gemm_tn, k_jk_stream, k_j_sym and k_j_sym8 in the compiler's per-kernel
  report is claimed by at least one case through expected_kernels().
"""
import json

import numpy as np
import pytest

import jk_cases as jc
import oracle

EXACT = 2.0 ** 53
INT_DENSE = jc.DENSE_CASES + jc.ROWS_CASES + [jc.UNALIGNED_DENSE] + jc.SYM_CASES
INT_FACT = jc.FACT_CASES + [jc.FACT_MIXED_DM, jc.UNALIGNED_FACT] + jc.KSPLIT_CASES
# the oracle cross-check runs where it takes well under a second: the dense reference is n^4 work
ORACLE_DENSE_N = sorted({c.n for c in INT_DENSE if c.n <= 65})
ORACLE_FACT = sorted({(c.n, c.naux, c.nocc) for c in INT_FACT})


@pytest.mark.parametrize("c", INT_DENSE, ids=jc.case_id)
def test_dense_integer_cases_stay_exact_in_fp64(c):
    b = jc.dense_bounds(c.n)
    assert set(b) == {"product", "partial", "J", "K", "J_sym8"}
    for name, v in b.items():
        assert v < EXACT, (name, v)
    assert max(b.values()) < 2 ** 31          # in fact not even 32 bits are needed at these sizes


@pytest.mark.parametrize("c", INT_FACT, ids=jc.case_id)
def test_factorised_integer_cases_stay_exact_in_fp64(c):
    b = jc.fact_bounds(c.n, c.naux, c.nocc, dm_products=c.dm_products)
    assert set(b) == {"dm", "Yt", "fused_dot", "dot", "J", "K"}
    for name, v in b.items():
        assert v < EXACT, (name, v)


def test_bounds_hold_for_the_generated_arrays():
    """The bounds are worst cases of the entry ranges: the generated cases must respect both."""
    eri, dm, J, K = jc.dense_int_case(33)
    assert np.abs(eri).max() <= jc.ERI_MAX and np.abs(dm).max() <= jc.DM_MAX
    assert np.array_equal(eri, np.rint(eri)) and not np.array_equal(eri, eri.T)
    b = jc.dense_bounds(33)
    assert np.abs(J).max() <= b["J"] and np.abs(K).max() <= b["K"]
    for sym in (1, 2):
        eri, dm, J = jc.sym_int_case(48, sym)
        assert np.abs(eri).max() <= jc.ERI_MAX and np.abs(dm).max() <= jc.DM_MAX and np.array_equal(eri, eri.T)
        assert np.abs(J).max() <= b["J"] * (48 / 33) ** 2
    e4 = eri.reshape(48, 48, 48, 48)                                       # sym = 2: all eight images, dm symmetric
    assert np.array_equal(e4, e4.transpose(1, 0, 2, 3)) and np.array_equal(e4, e4.transpose(0, 1, 3, 2)) and np.array_equal(dm, dm.T)
    chol, cocc, dm, J, K = jc.fact_int_case(41, 7, 17)
    assert np.abs(chol).max() <= jc.L_MAX and np.abs(cocc).max() <= jc.C_MAX and np.array_equal(chol, chol.transpose(0, 2, 1))
    b = jc.fact_bounds(41, 7, 17)
    assert np.abs(dm).max() <= b["dm"] and np.abs(J).max() <= b["J"] and np.abs(K).max() <= b["K"]
    assert np.abs(np.einsum("ni,pnb->pib", cocc, chol)).max() <= b["Yt"]
    assert np.abs(np.einsum("pij,ij->p", chol, dm)).max() <= min(b["dot"], b["fused_dot"])
    chol, cocc, dm, J, K = jc.fact_mixed_dm_case(41, 7, 17)
    b = jc.fact_bounds(41, 7, 17, dm_products=2)
    assert np.abs(dm).max() <= b["dm"] and np.abs(J).max() <= b["J"] and not np.array_equal(dm, cocc @ cocc.T)


@pytest.mark.parametrize("n", ORACLE_DENSE_N)
def test_dense_integer_reference_equals_the_oracle(n):
    eri, dm, J, K = jc.dense_int_case(n)
    assert np.array_equal(J, oracle.coulomb(eri, dm))
    assert np.array_equal(K, oracle.exchange(eri, dm))


@pytest.mark.parametrize("n,sym", [(48, 1), (49, 1), (48, 2), (49, 2)])
def test_symmetric_integer_reference_equals_the_oracle(n, sym):
    eri, dm, J = jc.sym_int_case(n, sym)
    assert np.array_equal(J, oracle.coulomb(eri, dm))
    # what the kernels may read determines J: the rest of the matrix follows from the symmetry
    keep = jc.sym_read_mask(n, sym)
    assert keep.sum() == (n * n * (n * n + 1) // 2 if sym == 1 else (n * (n + 1) // 2) * (n * (n + 1) // 2 + 1) // 2)


@pytest.mark.parametrize("nao,naux,nocc", ORACLE_FACT)
def test_factorised_integer_reference_equals_the_oracle(nao, naux, nocc):
    chol, cocc, dm, J, K = jc.fact_int_case(nao, naux, nocc)
    Jo, Ko = oracle.jk_from_factors(chol, dm)
    assert np.array_equal(J, Jo) and np.array_equal(K, Ko)
    assert np.array_equal(K, K.T) and np.array_equal(J, J.T)
    if (nao, naux, nocc) == tuple(jc.FACT_MIXED_DM[1:4]):
        chol, cocc, dm, J, K = jc.fact_mixed_dm_case(nao, naux, nocc)
        assert np.array_equal(J, oracle.jk_from_factors(chol, dm)[0])
        assert np.array_equal(K, oracle.jk_from_factors(chol, cocc @ cocc.T)[1])


def test_longdouble_references_agree_with_fp64_to_roundoff():
    """The real-valued references are the same contractions in longdouble: they differ from the fp64 oracle by fp64
    round-off only, far inside the 1e-12 of the GPU comparison."""
    assert np.finfo(np.longdouble).eps < 1e-18
    eri, dm, J, K = jc.dense_real_case(33)
    assert J.dtype == np.longdouble and K.dtype == np.longdouble
    assert np.abs(J - oracle.coulomb(eri, dm)).max() <= 1e-13 * np.abs(J).max()
    assert np.abs(K - oracle.exchange(eri, dm)).max() <= 1e-13 * np.abs(K).max()
    chol, cocc, dm, J, K = jc.fact_real_case(97, 6, 57)
    Jo, Ko = oracle.jk_from_factors(chol, dm)
    assert np.abs(J - Jo).max() <= 1e-13 * np.abs(J).max() and np.abs(K - Ko).max() <= 1e-13 * np.abs(K).max()


def test_tables_reach_the_edges_they_name():
    blocks = {c.n: jc.dense_blocks(c.n) for c in jc.DENSE_CASES}
    assert blocks == {32: (32, 1, 32), 33: (31, 2, 2), 34: (30, 2, 4), 45: (22, 3, 1), 64: (16, 4, 16), 65: (15, 5, 5),
                      102: (10, 11, 2)}
    assert 32 * 32 == jc.JK_COLS and 16 * 64 == jc.JK_COLS and 15 * 65 == 975
    # jsplit = 1 for K at n = 102 on the 256 CUs of an MI355X, as at the n = 114 workload; every smaller n of the table splits j
    assert jc.dense_jsplit(102, 102, 256) == 1 and jc.dense_jsplit(114, 114, 256) == 1
    assert all(jc.dense_jsplit(n, n, 256) > 1 for n in (32, 33, 34, 45, 64, 65)) and jc.dense_jsplit(100, 100, 256) > 1
    # row blocks: more than one column block in every case (the existing row tests stop at n = 24, ncb = 1)
    assert all(jc.dense_blocks(c.n)[1] >= 2 for c in jc.ROWS_CASES)
    assert [jc.half_transform_stages(c.n, c.nocc) for c in jc.FACT_CASES[:3]] == [1, 2, 3]
    # both sides of every tier boundary, and both parities of nao in every tier
    noccs = {c.nocc for c in jc.FACT_CASES}
    assert {16, 17, 32, 33, 48, 49, 64, 65, 128, 129} <= noccs
    for tier in {jc.half_transform_tier(c.nocc) for c in jc.FACT_CASES}:
        assert {c.n % 2 for c in jc.FACT_CASES if jc.half_transform_tier(c.nocc) == tier} == {0, 1}, tier
    assert {jc.half_transform_tier(c.nocc)[1] for c in jc.FACT_CASES if c.nocc <= 64} == {1, 2, 3, 4}
    ids = [jc.case_id(c) for c in jc.ALL_CASES]
    assert len(set(ids)) == len(ids)


def test_every_jk_instantiation_is_claimed_by_a_case():
    """Coverage ledger.  Whoever adds an instantiation of these kernels adds a case that reaches it."""
    import quantum_compute_dft_amd as q
    from quantum_compute_dft_amd import build
    q.build_library()
    res = json.load(open(build.RESOURCES_PATH))
    built = {jc.parse_instantiation(k) for k in res} - {None}
    assert {name for name, _ in built} == set(jc.LEDGER_KERNELS)
    assert len(built) >= 31                                                # 20 + 6 + 2 + 3 at the time of writing
    claimed = {}
    for c in jc.ALL_CASES:
        for k in jc.expected_kernels(c):
            claimed.setdefault(k, []).append(jc.case_id(c))
    unclaimed = sorted(built - set(claimed))
    assert not unclaimed, f"no case of tests/jk_cases.py reaches {unclaimed}"
    phantom = sorted(set(claimed) - built)
    assert not phantom, f"expected_kernels() names instantiations the library does not have: {phantom}"
