"""gradients.nuclear_gradient_uks on scf.HipBackend -- the XC part by DFT_ComputeXCGradientSpin, the Fock parts from the
device, the two-electron part on the host or by DFT_Grad2eSpin -- against the host assembly from the same densities, and the
driver's --open-shell-gradient.

Bounds as in tests/test_gpu_xc_gradient.py::test_nuclear_gradient_on_the_device: 2e-8 of max|g| for the whole gradient,
Cholesky vectors to 1e-10 so that their share of W stays below it, net force below 1e-3 at grid level 1.  The device
two-electron term is held to the host's by grad2e_helper's yardstick."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import grad2e_helper as gh  # noqa: E402
from quantum_compute_dft_amd import gradients, inputs, integrals, scf  # noqa: E402
from uks_host_backend import UksHostBackend  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_REL = 2e-8
KW = dict(charge=1, spin=1)


@pytest.fixture(scope="module")
def dense():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return inputs.build("H2O", "def2-svp", 1, verbose=False, **KW)


@pytest.mark.parametrize("eri_mode", ["dense", "cholesky"])
def test_uks_gradient_on_the_device(dense, eri_mode):
    """H2O+ B3LYP/def2-SVP, a doublet."""
    inp = dense if eri_mode == "dense" else inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=1e-10, **KW)
    be = scf.HipBackend(inp, "B3LYP", device_resident=False, fused_tail=False, eigensolver="exact")
    res = scf.run_uks(inp, be, "B3LYP", log=None, conv_e=1e-10)
    assert res["converged"] and res["nalpha"] == 5 and res["nbeta"] == 4
    state = {k: res[k] for k in ("dm_a", "dm_b", "nalpha", "nbeta")}
    ref, ref_terms = gradients.nuclear_gradient_uks(dense, state, UksHostBackend(dense, "B3LYP"), "B3LYP")
    scale = float(np.abs(ref).max())
    got = {}
    for engine in ("host", "device"):
        g, terms = gradients.nuclear_gradient_uks(inp, res, be, two_electron=engine)
        got[engine] = (g, terms)
        for k in ref_terms:
            print(f"gpu nuclear_gradient_uks H2O+/def2-SVP B3LYP {eri_mode} two_electron={engine} {k}: {np.abs(terms[k] - ref_terms[k]).max() / scale:.2e}")
        err = float(np.abs(g - ref).max())
        print(f"gpu nuclear_gradient_uks H2O+/def2-SVP B3LYP {eri_mode} two_electron={engine}: max|g| {scale:.3e}  err {err / scale:.2e}")
        assert np.all(np.isfinite(g)) and err <= ERR_REL * scale
        assert g.shape == (3, 3) and np.abs(g.sum(axis=0)).max() < 1e-3      # grid level 1: the fixed quadrature's net force
    (g_h, t_h), (g_d, t_d) = got["host"], got["device"]
    assert all(np.array_equal(t_d[k], t_h[k]) for k in t_h if k != "two_electron")
    assert np.array_equal(gradients.nuclear_gradient_uks(inp, res, be)[0], g_h)          # the default is the host
    dm_a, dm_b = (np.ascontiguousarray(0.5 * (res[k] + res[k].T)) for k in ("dm_a", "dm_b"))
    assert np.array_equal(integrals.grad2e_spin(inp.shells, dm_a + dm_b, dm_a - dm_b, 0.2), t_h["two_electron"])      # B3LYP's exchange weight
    case = (list(inp.symbols), np.asarray(inp.atom_xyz, dtype=np.float64), "def2-svp")
    bar = gh.reorder_bar(case, dm_a + dm_b, 0.2, integrals.grad2e(inp.shells, dm_a + dm_b, 0.2))
    gh.check(f"nuclear_gradient_uks H2O+/def2-SVP B3LYP {eri_mode} two_electron device vs host", t_d["two_electron"], t_h["two_electron"], bar)
    be.close()


def test_backend_gradient_in_slices(dense):
    """HipBackend.xc_gradient_spin: the resident planes whole and in slices of 3000 rows, against the host."""
    be = scf.HipBackend(dense, "B3LYP", device_resident=False, fused_tail=False, eigensolver="exact")
    rng = np.random.default_rng(5)
    ca, cb = 0.4 * rng.standard_normal((dense.shells.nao, 5)), 0.4 * rng.standard_normal((dense.shells.nao, 4))
    dm_a, dm_b = ca @ ca.T, cb @ cb.T
    ao, gr, hs = gradients.ao_planes_host(dense.shells, dense.grids.coords)
    ref = gradients.xc_gradient_spin_host("B3LYP", dm_a, dm_b, ao, dense.grids.weights, gr, hs)
    for rows in (None, 3000):
        G = be.xc_gradient_spin(dm_a, dm_b, slice_rows=rows)
        err = float(np.abs(G - ref).max() / np.abs(ref).max())
        print(f"gpu HipBackend.xc_gradient_spin H2O+/def2-SVP B3LYP slice_rows={rows}: {err:.2e}")
        assert err <= ERR_REL
    be.close()


def test_backend_refusals(dense):
    be = scf.HipBackend(dense, "B3LYP")          # the closed-shell defaults: the fused tail
    z = np.zeros((dense.shells.nao, dense.shells.nao))
    if be.fused or be.device_resident:
        with pytest.raises(ValueError, match="open-shell DFT"):
            be.xc_gradient_spin(z, z)
    be = scf.HipBackend(dense, "LDA", xc_occ=False, dm_factor=True, device_resident=False, fused_tail=False)
    with pytest.raises(ValueError, match="dm_factor"):
        be.xc_gradient_spin(z, z)
    be = scf.HipBackend(dense, "B3LYP", device_resident=False, fused_tail=False)
    be.world = 2
    with pytest.raises(ValueError, match="one rank"):
        be.xc_gradient_spin(z, z)
    with pytest.raises(ValueError, match="device two-electron gradient runs on one rank"):
        be.grad2e_spin(z, z, 0.2)


def test_driver_relaxes_the_cation(tmp_path):
    """--optimize --spin 1 --charge 1 --open-shell-gradient: H2O+/STO-3G LDA at grid level 3 (the driver's defaults), the
    two-electron term on the device."""
    out = tmp_path / "opt.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "LDA", "H2O", "--quirks", "0", "--spin", "1", "--charge", "1",
           "--optimize", "--open-shell-gradient", "--grad2e", "device", "--json", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["uks"] is True and rec["converged"] and rec["grad2e_engine"] == "device"
    assert rec["opt_converged"] and 1 <= rec["opt_steps"] <= 30
    assert rec["opt_energies"][-1] < rec["opt_energies"][0] - 1e-5
    assert set(rec["gradient_terms"]) == {"one_electron", "two_electron", "xc", "nuclear", "external"}
    assert np.abs(np.asarray(rec["gradient"])).max() > 3e-4          # the shipped geometry is the neutral molecule's, not the cation's
    assert (tmp_path / "H2O_opt.xyz").exists()
