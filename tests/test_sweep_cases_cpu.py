"""CPU side of the sweep / AO dispatch tests: the case tables of tests/sweep_cases.py are what
tests/test_gpu_sweep_dispatch.py runs.

* coverage ledger: every instantiation of the sweep and AO kernel families in the compiler's per-kernel report is
  claimed by at least one case through expected_kernels(), and every claim names an instantiation that exists;
* the edges the tables name are the ones the restated dispatch gives;
* every sweep case is an input the oracle can hold: its own response to last-bit perturbations of dm, ao and grad
  stays at or below a tenth of the bound the GPU comparison uses.
"""
import json

import numpy as np
import pytest

import oracle
import sweep_cases as sc


def _built():
    import quantum_compute_dft_amd as q
    from quantum_compute_dft_amd import build
    q.build_library()
    res = json.load(open(build.RESOURCES_PATH))
    return {sc.parse_instantiation(k) for k in res} - {None}


def _claimed(cases):
    claimed = {}
    for c in cases:
        for k in sc.expected_kernels(c):
            claimed.setdefault(k, []).append(sc.case_id(c))
    return claimed


def test_every_sweep_and_ao_instantiation_is_claimed_by_a_case():
    """Coverage ledger.  Whoever adds an instantiation of these kernels adds a case that reaches it; the instantiations
    only tools/occ_time.py's variables reach are not exempt (their cases carry the variables in `env`)."""
    built = _built()
    per_family = {f: sum(1 for name, _ in built if name == f) for f in sc.LEDGER_KERNELS}
    for f, floor in sc.LEDGER_FLOOR.items():
        assert per_family[f] >= floor, f"{f}: {per_family[f]} instantiations parsed from the report, {floor} when the ledger was written"
    claimed = _claimed(sc.ALL_CASES)
    unclaimed = sorted(built - set(claimed))
    assert not unclaimed, f"no case of tests/sweep_cases.py reaches {unclaimed}"
    phantom = sorted(set(claimed) - built)
    assert not phantom, f"expected_kernels() names instantiations the library does not have: {[(k, claimed[k][0]) for k in phantom]}"


@pytest.mark.parametrize("drop", ["xc-B3LYP-g1029-n15-tiny0", "xc-LDA-g1029-n36-tiny0", "xc_occ-LDA-g307-n131-o48-occ1-OCC_RES_KB100",
                                  "xc_occ-GGA-g307-n193-o32-occ1-OCC_NW8", "eval_ao-GGA-g43-huge_odd-ao_pt8"])
def test_deleting_a_case_unclaims_an_instantiation(drop):
    """The ledger is tight where it can be: these cases (one per family of the table) are the only ones that reach some
    instantiation, so the ledger test fails without any one of them.  More than a hundred cases are such sole claimants;
    the others name an edge of the grid, of the options or of the dispatch in a kernel a neighbour already claims."""
    rest = [c for c in sc.ALL_CASES if sc.case_id(c) != drop]
    assert len(rest) == len(sc.ALL_CASES) - 1
    assert _built() - set(_claimed(rest))
    claims = {}
    for c in sc.ALL_CASES:
        for k in sc.expected_kernels(c):
            claims.setdefault(k, []).append(c)
    assert len({v[0] for v in claims.values() if len(v) == 1}) >= 100


def test_env_cases_need_their_variables():
    """occ_plan reads QCDFT_OCC_NW / QCDFT_OCC_RES_KB with getenv at every plan (the GPU test sets them with
    monkeypatch.setenv): without the variable the same shape takes another instantiation, so the cases do need it."""
    env_cases = [c for c in sc.ALL_CASES if c.env]
    assert len(env_cases) >= 24
    for c in env_cases:
        assert sc.expected_kernels(c) != sc.expected_kernels(c._replace(env=())), sc.case_id(c)
    nw8 = {k for c in env_cases for k in sc.expected_kernels(c) if k[0] == "k_rho_occ"}
    assert nw8 == {("k_rho_occ", (nto, 8, g, v, False, 1)) for nto in (1, 2, 3, 4) for g in (False, True) for v in (False, True)}


def test_tables_reach_the_edges_they_name():
    ids = [sc.case_id(c) for c in sc.ALL_CASES]
    assert len(set(ids)) == len(ids)
    ws = [c for c in sc.SWEEP_CASES if any(k[0] == "k_rho_ws" for k in sc.expected_kernels(c))]
    for nt in range(1, 9):                                         # both parities in every NT, for both kernels
        assert {c.nao % 2 for c in ws if sc.nt_of(c.nao) == nt} == {0, 1}, nt
        assert {sc.nt_of(w) for w in sc.WS_PLAIN[nt]} == {nt}
        if nt >= 2:
            fr = [c for c in ws if sc.nt_of(c.nao) == nt and sc.fringe(c, c.nao)]
            assert {c.nao % 2 for c in fr} == {0, 1} and {c.xc for c in fr} >= {"LDA", "GGA"}, nt
    assert {c.nao % 16 for c in ws if sc.fringe(c, c.nao)} == {1, 2, 3, 4}
    assert not any(sc.fringe(c, c.nao) for c in ws if c.xc == "B3LYP" or c.vxc_fringe == 0 or c.nao <= 16)
    naos = {c.nao for c in sc.SWEEP_CASES if c.entry == "xc" and c.path is None}
    assert {16, 17, 32, 33, 128, 129} <= naos
    assert sc.TINY_MAX_NAO == 32 and {c.nao for c in sc.TINY_CASES if sc.takes_tiny(c, c.nao)} >= {16, 17, 32}
    assert not sc.takes_tiny(sc.TINY_CASES[12], 33) and sc.TINY_CASES[12].nao == 33
    # occupied orbitals: both parities in every NTO of both kernels, the resident limit from both sides, nch 4 / 5, npass 1 / 2
    occ = [(c, sc.occ_plan(c.nao, c.nocc, c.xc != "LDA", c.env)) for c in sc.OCC_CASES if sc.uses_occ(c, c.nao)]
    for nto in range(1, 9):
        assert {c.nao % 2 for c, p in occ if p.nto == nto and not p.resident} == {0, 1}, nto
        if nto <= 4:
            assert {c.nao % 2 for c, p in occ if p.nto == nto and p.resident} == {0, 1}, nto
            assert {(c.nao % 2, p.multi) for c, p in occ if p.nto == nto and p.resident} == {(0, False), (1, False), (0, True), (1, True)}, nto
    assert [sc.resident_limit(n) for n in (1, 2, 3, 4)] == [384, 192, 96, 64]
    for nto in (1, 2, 3, 4):
        lim = sc.resident_limit(nto)
        assert any(p.nto == nto and p.resident and c.nao == lim and not c.env for c, p in occ), nto
        assert any(p.nto == nto and not p.resident and c.nao == lim + 1 and not c.env for c, p in occ), nto
    res = {p.nch for c, p in occ if p.resident and not c.env}
    assert {4, 5} <= res and {p.npass for c, p in occ} == {1, 2}
    assert {c.nocc for c, p in occ} >= {16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129}
    auto = [c for c in sc.OCC_CASES if c.occ is None]
    assert {sc.uses_occ(c, c.nao) for c in auto} == {True, False} and any(not c.pass_dm and not sc.uses_occ(c, c.nao) for c in auto)
    # AO tables
    ao = {sc.expected_kernels(c).copy().pop()[1] for c in sc.AO_CASES}
    assert ao == {(g, v, pt, t) for g in (False, True) for v in (False, True) for pt in (8, 16) for t in (False, True)}
    for name, grad in sc.AO_TAB_PAIRS:
        sh = sc.ao_table(name)
        assert [sc.ao_kernel(sh, grad, pt, True)[1][3] for pt in (16, 8)] == [False, True], name
    for name in ("huge_even", "huge_odd"):                         # tile + table crosses the limit for every (GRAD, PT)
        sh = sc.ao_table(name)
        assert sh.nshell >= 300 and set(sh.l) == {0, 1, 2, 3} and sh.nprim.max() == 12
        assert 8 * 8 * (sc.AO_CW | 1) + sc.ao_tab_bytes(sh) > sc.AO_TAB_LIMIT
    assert sc.ao_blocks(sc.ao_table("borrow").l) == ([(0, 24, 0, 120), (24, 28, 120, 10)], 1)
    assert len(sc.ao_blocks(sc.ao_table("t130").l)[0]) == 2
    # direct sweep: chunks that divide the grid, leave a ragged last chunk, exceed the grid; odd planes behind a ragged chunk
    chunks = {sc.case_id(c): sc.direct_chunks(c) for c in sc.DIRECT_CASES}
    assert [256, 256, 256, 256, 5] in chunks.values() and [256] * 4 in chunks.values() and [512, 512, 5] in chunks.values()
    assert [sc.NG] in chunks.values() and {sc.ao_table(c.table).nao for c in sc.DIRECT_CASES} == {37, 83, 130}
    assert any(c.xc == "LDA" for c in sc.DIRECT_CASES)
    for c in sc.DIRECT_CASES:
        assert sc.direct_chunks(c, 32) == sc.direct_chunks(c, 304) and sum(sc.direct_chunks(c)) == c.ngrid


def test_no_shell_table_leaves_a_block_on_an_odd_column():
    """prepare_ao_table starts a block on an odd column only when the block before holds a single shell, which would
    have to be wider than AO_CW minus the widest shell: with l <= 3 every seam on an odd column takes the previous shell
    along.  `even_blocks` is therefore true for every legal table, and 8-byte stores at even nao come from unaligned
    outputs alone (the case table has one)."""
    assert 2 * (2 * sc.AO_MAX_L + 1) <= sc.AO_CW
    rng = np.random.default_rng(3)
    for _ in range(300):
        blocks, _ = sc.ao_blocks(rng.integers(0, sc.AO_MAX_L + 1, int(rng.integers(1, 400))))
        assert all(b[2] % 2 == 0 and b[3] <= sc.AO_CW and b[1] > b[0] for b in blocks)
        assert all(a[1] == b[0] and a[2] + a[3] == b[2] for a, b in zip(blocks, blocks[1:]))


PERTURBATIONS = (lambda d, a, g: (d * (1 + 1e-15), a, g), lambda d, a, g: (d, a * (1 + 1e-15), g),
                 lambda d, a, g: (d, a, g * (1 - 1e-15)), lambda d, a, g: (d * (1 - 2e-15), a * (1 + 1e-15), g))


@pytest.mark.parametrize("c", sc.SWEEP_CASES, ids=sc.case_id)
def test_sweep_inputs_are_ones_the_oracle_can_hold(c):
    """The four last-bit perturbations of test_conditioning_aware_bound_on_ill_conditioned_small_bases move the oracle's
    Vxc by at most 1e-12 max|V|, a tenth of the 1e-11 max|V| the GPU is held to: the comparison measures the kernel, not
    the conditioning of the functional at the synthetic points.  A case that fails gets another seed, not a wider bound."""
    cocc, dm, ao, gr, w = sc.sweep_inputs(c)
    t = sc.oracle_type(c.xc)
    _, v_ref = sc.sweep_reference(c)
    g = gr if t else None
    sens = 0.0
    for pert in PERTURBATIONS:
        d2, a2, g2 = pert(dm, ao, gr)
        sens = max(sens, np.abs(oracle.compute_xc(t, d2, a2, w, g2 if t else None)[1] - v_ref).max())
    assert np.isfinite(v_ref).all() and np.abs(v_ref).max() > 0
    assert sens <= 1e-12 * np.abs(v_ref).max(), (sens / np.abs(v_ref).max())
