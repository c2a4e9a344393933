"""The two-electron term of the nuclear gradient on the device (csrc/grad2e.hip: DFT_Grad2e, integrals.DeviceGrad2e,
HipBackend.grad2e, nuclear_gradient(two_electron="device")) against the host engine (integrals.c::qc_grad2e).

Yardstick (grad2e_helper): bar = the HOST's own spread between the two orders of the atoms, measured in the test; a
comparison passes when 10 bar <= 1e-11 and |device - host| <= max(10 bar, 1e-13) max|host|.  Measured figures:
profiles/grad2e_parity.txt."""
import ctypes

import numpy as np
import pytest
import torch

import grad2e_helper as gh
from quantum_compute_dft_amd import gradients, inputs, integrals, scf

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64, order="C"), device="cuda")      # a copy: the shared cases are read-only


@pytest.fixture(scope="module")
def ch_engines():
    """One DeviceGrad2e per order of the CH fragment's atoms, shared by the tests (both alive at once)."""
    eng = {sw: integrals.DeviceGrad2e(gh.ch_case(0.0, sw)["shells"]) for sw in (False, True)}
    yield eng
    for e in eng.values():
        e.close()


@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("c_hf", [0.0, 0.25])
def test_every_class(ch_engines, c_hf, swapped):
    """CH/def2-TZVP: s-f on bra and ket; with the atoms swapped the (l_a < l_b) classes and the ket pairs C >= D come in
    the other index order.  The d and f shells all sit on the carbon, so every quartet with three or four shells of
    l >= 2 is a ONE-centre quartet here (no centre difference, Boys argument exactly 0), and (ff|ff) from the one f shell
    has a derivative that is zero by parity: the ff bra's largest LDS configuration is launched, its values are not
    tested.  The four-centre classes, (dd|dd) and (ff|ff) at L = 13 among them, are held against the 100-digit reference
    in tests/test_gpu_grad2e_reference.py."""
    c = gh.ch_case(c_hf, swapped)
    eng = ch_engines[swapped]
    rows = eng.per_shell(_dev(c["D"]), c_hf).cpu().numpy()
    label = f"CH/def2-TZVP{' atoms swapped' if swapped else ''} c_hf {c_hf}"
    gh.check(label + " per shell", rows, c["per_shell"], c["bar"])
    gh.check(label + " per atom", eng.grad(c["D"], c_hf), c["per_atom"], c["bar"])


def test_contracted_s_and_p():
    sh = gh.molecule(gh.H2O_STO)[2]
    D = gh.random_density(sh.nao)
    assert sh.nshell == 5
    rows_h, g_h = gh.host_pair(sh, D, 0.25)
    bar = gh.reorder_bar(gh.H2O_STO, D, 0.25, g_h)
    eng = integrals.DeviceGrad2e(sh)
    gh.check("H2O/STO-3G c_hf 0.25 per shell", eng.per_shell(_dev(D), 0.25).cpu().numpy(), rows_h, bar)
    gh.check("H2O/STO-3G c_hf 0.25 per atom", eng.grad(D, 0.25), g_h, bar)
    eng.close()


def test_one_shell():
    sh = gh.molecule(gh.H_ATOM)[2]
    assert sh.nshell == 1
    eng = integrals.DeviceGrad2e(sh)
    rows = eng.per_shell(_dev(np.array([[0.8]])), 0.25).cpu().numpy()
    assert rows.shape == (1, 3) and np.abs(rows).max() <= 1e-14
    eng.close()


def test_exactly_zero_quartets(ch_engines):
    """D block-diagonal per atom: every density quartet with an odd mix of centres is exactly zero and is skipped."""
    c = gh.ch_case(0.25, False, True)
    assert np.count_nonzero(c["D"]) < c["D"].size
    rows = ch_engines[False].per_shell(_dev(c["D"]), 0.25).cpu().numpy()
    gh.check("CH/def2-TZVP block-diagonal D c_hf 0.25 per shell", rows, c["per_shell"], c["bar"])


def test_translational_invariance_on_the_device(ch_engines):
    for c_hf in (0.0, 0.25):
        c = gh.ch_case(c_hf)
        rows = ch_engines[False].per_shell(_dev(c["D"]), c_hf).cpu().numpy()
        net = np.abs(rows.sum(axis=0)).max() / np.abs(rows).max()
        print(f"gpu grad2e CH/def2-TZVP c_hf {c_hf}: |sum over shells| / max|row| {net:.2e}")
        assert net <= 1e-10


def test_reproducible(ch_engines):
    c = gh.ch_case(0.25)
    eng = ch_engines[False]
    d_D, d_other = _dev(c["D"]), _dev(gh.random_density(c["shells"].nao, seed=11))
    a = eng.per_shell(d_D, 0.25).clone()
    b = eng.per_shell(d_D, 0.25).clone()
    eng.per_shell(d_other, 0.0)
    out = torch.full((c["shells"].nshell, 3), 7.0, dtype=torch.float64, device="cuda")
    assert eng.per_shell(d_D, 0.25, out=out) is out
    assert torch.equal(a, b) and torch.equal(a, out)
    assert not torch.equal(a, eng.per_shell(d_other, 0.25))
    # a handle on another molecule, alive at the same time and used in between (the __constant__ tables are shared)
    sh2 = gh.molecule(gh.H2O_SVP)[2]
    D2 = gh.random_density(sh2.nao)
    eng2 = integrals.DeviceGrad2e(sh2)
    r2 = eng2.per_shell(_dev(D2), 0.25).clone()
    assert torch.equal(a, eng.per_shell(d_D, 0.25))
    assert torch.equal(r2, eng2.per_shell(_dev(D2), 0.25))
    rows_h, g_h = gh.host_pair(sh2, D2, 0.25)
    gh.check("H2O/def2-SVP c_hf 0.25 per shell (second handle)", r2.cpu().numpy(), rows_h, gh.reorder_bar(gh.H2O_SVP, D2, 0.25, g_h))
    eng2.close()


def test_refusals(ch_engines):
    c = gh.ch_case(0.0)
    eng = ch_engines[False]
    skew = np.array(c["D"])
    skew[0, 1] += 1e-3
    with pytest.raises(ValueError, match="symmetric"):
        eng.grad(skew, 0.0)
    d_D = _dev(c["D"])
    out = torch.zeros((c["shells"].nshell, 3), dtype=torch.float64, device="cuda")
    u64 = ctypes.c_uint64
    assert eng.lib.DFT_Grad2e(eng._h, u64(0), 0.0, u64(out.data_ptr())) == -1
    assert eng.lib.DFT_Grad2eLastError(eng._h)
    assert eng.lib.DFT_Grad2e(eng._h, u64(d_D.data_ptr()), 0.0, u64(0)) == -1
    assert eng.lib.DFT_Grad2eLastError(eng._h)
    assert eng.lib.DFT_Grad2e(None, u64(d_D.data_ptr()), 0.0, u64(out.data_ptr())) == -1
    assert eng.lib.DFT_Grad2eLastError(None)
    from scf_oracle_backend import OracleBackend
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    be = OracleBackend(inp, "LDA", quirks=False)
    res = scf.run_scf(inp, be, "LDA", log=None)
    with pytest.raises(ValueError, match="device two-electron gradient"):
        gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, two_electron="device")


def test_end_to_end():
    """H2O/def2-SVP B3LYP on HipBackend (dense ERI): the device term against the host term from the same converged state;
    every other term bitwise equal; the default is the host."""
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    be = scf.HipBackend(inp, "B3LYP")
    res = scf.run_scf(inp, be, "B3LYP", log=None, conv_e=1e-10)
    assert res["converged"]
    g_d, t_d = gradients.nuclear_gradient(inp, res, be, two_electron="device")
    g_h, t_h = gradients.nuclear_gradient(inp, res, be, two_electron="host")
    g_0, t_0 = gradients.nuclear_gradient(inp, res, be)
    assert np.array_equal(g_0, g_h) and all(np.array_equal(t_0[k], t_h[k]) for k in t_h)
    assert all(np.array_equal(t_d[k], t_h[k]) for k in t_h if k != "two_electron")
    dm = np.asarray(res["dm"], dtype=np.float64)
    dm = np.ascontiguousarray(0.5 * (dm + dm.T))
    case = (list(inp.symbols), np.asarray(inp.atom_xyz, dtype=np.float64), "def2-svp")
    c_hf = 0.2
    assert np.array_equal(integrals.grad2e(inp.shells, dm, c_hf), t_h["two_electron"])     # B3LYP's exchange weight
    bar = gh.reorder_bar(case, dm, c_hf, t_h["two_electron"])
    gh.check("nuclear_gradient H2O/def2-SVP B3LYP two_electron device vs host", t_d["two_electron"], t_h["two_electron"], bar)
    be.close()
