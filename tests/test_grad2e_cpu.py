"""The host side of the device two-electron gradient: integrals.grad2e(per_shell=True), the refusals that need no device
and the driver's option."""
import ctypes

import numpy as np
import pytest

import grad2e_helper as gh
from quantum_compute_dft_amd import gradients, inputs, integrals, scf


def _parent_grad2e(shells, dm, c_hf):
    """integrals.grad2e as it was before the per_shell keyword: qc_grad2e with the shell table's shell -> atom map."""
    keep, p = integrals._args(shells)
    dm = integrals._sym(dm, "dm")
    owner = np.ascontiguousarray(shells.atom, dtype=np.int32)
    natm = int(owner.max()) + 1
    out = np.zeros((natm, 3))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    assert integrals._load().qc_grad2e(shells.nshell, *p, shells.nao, owner.ctypes.data_as(ip), natm, dm.ctypes.data_as(dp), float(c_hf),
                                       out.ctypes.data_as(dp)) == 0
    return out


@pytest.mark.parametrize("case", ["CH/def2-TZVP", "H2O/def2-SVP"])
@pytest.mark.parametrize("c_hf", [0.0, 0.25])
def test_per_shell_rows_add_up_to_the_atoms(case, c_hf):
    if case.startswith("CH"):
        c = gh.ch_case(c_hf)
        sh, D, rows, g = c["shells"], c["D"], c["per_shell"], c["per_atom"]
    else:
        sh = gh.molecule(gh.H2O_SVP)[2]
        D = gh.random_density(sh.nao)
        rows, g = gh.host_pair(sh, D, c_hf)
    assert rows.shape == (sh.nshell, 3) and g.shape == (int(np.max(sh.atom)) + 1, 3)
    err = np.abs(gh.sum_per_atom(sh, rows) - g).max() / np.abs(g).max()
    print(f"cpu grad2e {case} c_hf {c_hf}: per-shell rows summed against per-atom {err:.2e}")
    assert err <= 1e-13
    # the default return: bitwise the parent's formula, twice, with and without the keyword
    a, b = integrals.grad2e(sh, D, c_hf), integrals.grad2e(sh, D, c_hf, per_shell=False)
    assert np.array_equal(a, b) and np.array_equal(a, g)
    assert np.array_equal(a, _parent_grad2e(sh, D, c_hf))


def test_the_yardstick_is_tight():
    """The host's own spread between the two orders of the atoms, which bounds every device comparison."""
    for c_hf in (0.0, 0.25):
        bar = gh.ch_case(c_hf)["bar"]
        print(f"cpu grad2e CH/def2-TZVP c_hf {c_hf}: reorder bar {bar:.2e}")
        assert 0.0 < 10.0 * bar <= 1e-11
        sw = gh.ch_case(c_hf, swapped=True)
        assert np.abs(sw["per_atom"][::-1] - gh.ch_case(c_hf)["per_atom"]).max() <= bar * np.abs(sw["per_atom"]).max() * (1 + 1e-12)


@pytest.mark.parametrize("name", list(gh.SLICE_CASES))
def test_the_multi_slice_molecules(name):
    """The two molecules of tests/test_gpu_grad2e_reference.py whose workgroups loop over several ket pairs: the shell
    counts that make it so, tied to the constant in DFT_Grad2eOpen; and the host engine the device is compared with there,
    held by translational invariance: d (f) shells on two centres, so an error in a term of the raised bra's recurrence
    that multiplies X_AB -- invisible where all shells of l >= 2 share a centre -- leaves a net force (measured 7e-14 of the largest row; the
    finite-difference projection of test_gradient_integrals_cpu on C2/def2-TZVP would take twice that file's slowest
    case and was left out)."""
    import os
    src = open(os.path.join(os.path.dirname(integrals.__file__), "csrc", "grad2e.hip")).read()
    assert f"std::min(c->nket, ({gh.SLICE_TARGET} + nshell * nshell - 1) / (nshell * nshell))" in src
    sh = gh.molecule(gh.SLICE_CASES[name])[2]
    nslice, nket, least, most = gh.slice_counts(sh.nshell)
    assert (sh.nshell, sh.nao, nslice, nket, least, most) == {"C2H4/def2-SVP": (24, 48, 57, 300, 5, 6), "C2/def2-TZVP": (22, 62, 68, 253, 3, 4)}[name]
    assert gh.slice_counts(15) == (120, 120, 1, 1) and gh.slice_counts(16) == (128, 136, 1, 2)      # every other test: one pair
    rows = integrals.grad2e(sh, gh.random_density(sh.nao), 0.25, per_shell=True)
    net = np.abs(rows.sum(axis=0)).max() / np.abs(rows).max()
    print(f"cpu grad2e {name} c_hf 0.25: |sum over shells| / max|row| {net:.2e}")
    assert net <= 1e-10                              # the bound of every invariance test of the gradient terms


def test_device_engine_without_a_device_says_so():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no GPU device"):
        integrals.DeviceGrad2e(gh.molecule(gh.H_ATOM)[2])


def test_nuclear_gradient_refuses_an_unknown_engine():
    from scf_oracle_backend import OracleBackend
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    be = OracleBackend(inp, "LDA", quirks=False)
    res = scf.run_scf(inp, be, "LDA", log=None)
    with pytest.raises(ValueError, match="two_electron"):
        gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, two_electron="bogus")
    with pytest.raises(ValueError, match="device two-electron gradient"):           # a host backend has no device engine
        gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, two_electron="device")
    g = gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False)[0]
    assert np.array_equal(g, gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, two_electron="host")[0])


def test_driver_option():
    from quantum_compute_dft_amd import dft
    p = dft.build_parser()
    assert p.parse_args(["B3LYP", "H2O", "--gradient"]).grad2e == "host"
    assert p.parse_args(["B3LYP", "H2O", "--gradient", "--grad2e", "device"]).grad2e == "device"
    assert p.parse_args(["B3LYP", "H2O", "--optimize", "--grad2e", "host"]).grad2e == "host"
    with pytest.raises(SystemExit):
        p.parse_args(["B3LYP", "H2O", "--gradient", "--grad2e", "elsewhere"])
