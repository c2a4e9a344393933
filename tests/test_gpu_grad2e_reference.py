"""The device two-electron gradient (csrc/grad2e.hip: DFT_Grad2e, DFT_Grad2eSpin) where the other device tests do not
reach.

First part: the device against the 100-digit reference of tests/golden/grad_ref_g{1,2,3}.npz (grad_fixtures; made by
tests/golden/make_grad_reference.py from oracle/eri_reference.py, which shares no formulation with the engines) -- four
shells on four centres, so the quartets with three or four shells of l >= 2 are four-centre quartets, not the one-centre
ones of CH/def2-TZVP: g1 = s p d f (all 16 bra classes x 10 ket classes, the lmax = 3 LDS layout), g2 = d d d d (the
lmax = 2 layout of the def2-SVP production shapes), g3 = f f f f (every chunk of the ff bra, L = 13).  Both orders of the
shells.  Bound: |device - ref| <= 1e-12 max|ref| of the compared (4, 3) array (grad_fixtures.BOUND), against the
reference, not against the host.

Second part: the ket-slice loop.  k_grad2e cuts the ket-pair list into nslice = ceil(32768 / nshell^2) slices; up to 16
shells that is one ket pair per workgroup, and no other device test has more than 15 shells.  C2H4/def2-SVP (24 shells:
5-6 ket pairs per workgroup, d shells on two centres, both k_grad2e<64> and k_grad2e<256>) and C2/def2-TZVP (22 shells:
3-4 ket pairs per workgroup, f shells on two centres) run the loop's second and later iterations: the reuse of the
aliased density-quartet / R-table region, the tables of another ket class, the skip of an exactly-zero quartet between
non-zero ones, the sum carried over the ket pairs.  Device against host with grad2e_helper's yardstick: bar = the host's
own spread between the two orders of the atoms, 10 bar <= 1e-11 and |device - host| <= max(10 bar, 1e-13) max|host|.

Measured on one MI355X (profiles/grad2e_reference_parity.txt, "gpu" lines; QCDFT_WRITE_PROFILES=<dir> rewrites them):
against the reference 1.0e-15 .. 3.3e-15 of max|ref| in every family and order; against the host on the two molecules
1.4e-14 .. 1.1e-13 of max|host|, with reorder bars of 2.4e-14 .. 1.4e-13."""
import numpy as np
import pytest
import torch

import grad2e_helper as gh
import grad_fixtures as G
from quantum_compute_dft_amd import integrals

pytestmark = pytest.mark.gpu

CASES = [(n, r) for n in G.FAMILIES for r in (False, True)]
IDS = [f"{n}{'-reversed' if r else ''}" for n, r in CASES]


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64, order="C"), device="cuda")      # a copy: the shared cases are read-only


# ------------------------------------------------------------------------------------------ device against the reference
@pytest.mark.parametrize("name,reverse", CASES, ids=IDS)
def test_device_against_the_reference(name, reverse):
    f = G.family(name, reverse)
    eng = integrals.DeviceGrad2e(f["sh"])
    try:
        d_D, d_M = _dev(f["D"]), _dev(f["M"])
        got = [(f"grad2e c_hf {c:g}", eng.per_shell(d_D, c).cpu().numpy(), f["g2e"][i]) for i, c in enumerate(f["c_hf"])]
        got += [(f"grad2e_spin c_hf {c:g}", eng.per_shell_spin(d_D, d_M, c).cpu().numpy(), f["g2e_spin"][i]) for i, c in enumerate(f["c_hf"])]
    finally:
        eng.close()
    for what, rows, ref in got:
        G.check("gpu", G.label(f, what), rows, ref)


# ------------------------------------------------------------------------------------------ the ket-slice loop
@pytest.fixture(scope="module", params=list(gh.SLICE_CASES))
def sliced(request):
    """(name, one DeviceGrad2e for the molecule), closed when the molecule's tests are over."""
    eng = integrals.DeviceGrad2e(gh.molecule(gh.SLICE_CASES[request.param])[2])
    yield request.param, eng
    eng.close()


def _against_host(label, got, ref, bar):
    ref = np.asarray(ref)
    G.record("gpu", label + " (ref = host)", float(np.abs(ref).max()), float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max()))
    gh.check(label, got, ref, bar)


def test_the_cases_reach_the_loop(sliced):
    """From the shell count: fewer slices than ket pairs, so every workgroup has several ket pairs; d (f) shells on two
    centres; both launch shapes."""
    name, eng = sliced
    sh = eng.shells
    nslice, nket, least, most = gh.slice_counts(sh.nshell)
    assert -(-32768 // sh.nshell ** 2) < nket and nslice < nket
    want = {"C2H4/def2-SVP": (24, 48, 57, 300, 5, 6, 2), "C2/def2-TZVP": (22, 62, 68, 253, 3, 4, 3)}[name]
    assert (sh.nshell, sh.nao, nslice, nket, least, most, int(np.max(sh.l))) == want
    high = {int(a) for a, l in zip(sh.atom, sh.l) if l == want[6]}
    assert len(high) == 2                                           # the highest shells on two different centres
    assert {int(l) for l in sh.l} >= {0, 1, 2}                      # s/p bras: k_grad2e<64>, d/f bras: k_grad2e<256>


@pytest.mark.parametrize("c_hf", [0.0, 0.25])
def test_several_ket_pairs_per_workgroup(sliced, c_hf):
    name, eng = sliced
    c = gh.slice_case(name, c_hf)
    d_D, d_M = _dev(c["D"]), _dev(c["M"])
    label = f"{name} c_hf {c_hf}"
    _against_host(label + " per shell", eng.per_shell(d_D, c_hf).cpu().numpy(), c["per_shell"], c["bar"])
    _against_host(label + " per atom", eng.grad(np.array(c["D"]), c_hf), c["per_atom"], c["bar"])
    _against_host("spin " + label + " per shell", eng.per_shell_spin(d_D, d_M, c_hf).cpu().numpy(), c["spin_per_shell"], c["bar"])
    _against_host("spin " + label + " per atom", eng.grad_spin(np.array(c["D"]), np.array(c["M"]), c_hf), c["spin_per_atom"], c["bar"])


@pytest.mark.parametrize("c_hf", [0.0, 0.25])
def test_exactly_zero_quartets_between_others_in_a_slice(sliced, c_hf):
    """D and M block-diagonal per atom: the density quartets with an odd mix of centres are exactly zero and are skipped
    in mid-loop, between ket pairs that are not."""
    name, eng = sliced
    c = gh.slice_case(name, c_hf, blocked=True)
    assert 0 < np.count_nonzero(c["D"]) < c["D"].size and 0 < np.count_nonzero(c["M"]) < c["M"].size
    d_D, d_M = _dev(c["D"]), _dev(c["M"])
    label = f"{name} block-diagonal D, M c_hf {c_hf}"
    _against_host(label + " per shell", eng.per_shell(d_D, c_hf).cpu().numpy(), c["per_shell"], c["bar"])
    _against_host(label + " per atom", eng.grad(np.array(c["D"]), c_hf), c["per_atom"], c["bar"])
    _against_host("spin " + label + " per shell", eng.per_shell_spin(d_D, d_M, c_hf).cpu().numpy(), c["spin_per_shell"], c["bar"])
    _against_host("spin " + label + " per atom", eng.grad_spin(np.array(c["D"]), np.array(c["M"]), c_hf), c["spin_per_atom"], c["bar"])


def test_reproducible_and_translationally_invariant(sliced):
    name, eng = sliced
    for c_hf in (0.0, 0.25):
        c = gh.slice_case(name, c_hf)
        d_D, d_M = _dev(c["D"]), _dev(c["M"])
        for kind, run in (("", lambda: eng.per_shell(d_D, c_hf)), ("spin ", lambda: eng.per_shell_spin(d_D, d_M, c_hf))):
            a = run().clone()
            b = run().clone()
            assert torch.equal(a, b), (name, kind, c_hf)
            rows = a.cpu().numpy()
            net = np.abs(rows.sum(axis=0)).max() / np.abs(rows).max()
            print(f"gpu {kind}grad2e {name} c_hf {c_hf}: |sum over shells| / max|row| {net:.2e}")
            assert net <= 1e-10
