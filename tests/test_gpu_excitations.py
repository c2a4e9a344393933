"""excitations.excitations on the device (HipBackend.excitation_parts: DFT_ComputeJKFactorizedResponse or DFT_ComputeJK,
and DFT_FxcApply) for H2O / def2-SVP, grid level 1: 24 functions, 5 x 19 = 95 pairs.

* Three lowest roots, TDA and TDDFT, against the dense solution of matrices built on the HOST: response.HostResponse with
  the backend's own AO planes applied to every unit vector, LAPACK.  For the Cholesky run the host contracts the ERI
  rebuilt from the same vectors, so the truncation cancels.  Bound |dw| <= 1e-7 Ha, |df| <= 1e-6: the device V1 is bounded
  at 2e-8 of max|V1| (test_gpu_fxc.py) and the matrix elements are O(1).
* Cholesky excitation_parts against the dense backend for the same (A, Bs): J and M +- M^T within chol_tol * sum|D+-|,
  |sum_kl R_ijkl D_kl| <= max|R| sum|D| (the relation of test_gpu_response.py).
* The driver's table and JSON record.
"""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import excitation_dense as ed  # noqa: E402
from quantum_compute_dft_amd import excitations as ex  # noqa: E402
from quantum_compute_dft_amd import inputs, response, scf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(log=None, conv_e=1e-11, conv_dm=1e-9)
CHOL_TOL = 1e-10


@pytest.fixture(scope="module")
def dense_inp():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return inputs.build("H2O", "def2-svp", 1, verbose=False)


@pytest.fixture(scope="module")
def chol_inp():
    return inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=CHOL_TOL)


class HostOnDevicePlanes(response.HostResponse):
    """HostResponse on the AO planes of a HipBackend; the ground-state Fock parts come from that backend."""

    def __init__(self, inp, functional, be):
        gr = be.d_gr.cpu().numpy() if be.d_gr is not None else None
        super().__init__(inp, functional, None, be.d_ao.cpu().numpy(), gr, quirks=be.quirks)
        self.be = be

    def ground_state_parts(self, dm, cocc, want_k):
        return self.be.ground_state_parts(dm, cocc, want_k)


def record(label, dw, df, extra=""):
    print(f"{label}: |dw| {dw:.2e} Ha  |df| {df:.2e}  {extra}")
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "excitations_parity.txt"), "a") as fh:
            fh.write(f"gpu  {label:44s} |dw| {dw:9.2e} Ha   |df| {df:9.2e}   {extra}\n")


@pytest.mark.parametrize("functional,eri", [("LDA", "dense"), ("B3LYP", "dense"), ("B3LYP", "cholesky")])
def test_device_roots_against_the_host_built_dense_solution(dense_inp, chol_inp, functional, eri):
    inp = dense_inp if eri == "dense" else chol_inp
    be = scf.HipBackend(inp, functional)
    res = scf.run_scf(inp, be, functional, **KW)
    assert res["converged"]
    host_inp = inp if eri == "dense" else dataclasses.replace(inp, eri=np.einsum("pij,pkl->ijkl", inp.chol, inp.chol))
    ops = ex.ResponseOperators(host_inp, res, HostOnDevicePlanes(host_inp, functional, be), functional)
    ApB, AmB = ed.dense_matrices(ops)
    for tda in (True, False):
        out = ex.excitations(inp, res, be, functional, nroots=3, tda=tda)
        w, f = ed.dense_solution(ops, ApB, AmB, tda)
        dw, df = float(np.abs(out["energies"] - w[:3]).max()), float(np.abs(out["oscillator_strengths"] - f[:3]).max())
        record(f"H2O/def2-SVP {functional} {eri} {'TDA' if tda else 'TDDFT'}", dw, df,
               f"w = {' '.join(f'{x:.6f}' for x in out['energies'])}  iterations {out['iterations']}  trial vectors {out['sigma_builds']}")
        assert out["converged"] and np.all(np.diff(out["energies"]) > 0.0) and np.all(out["oscillator_strengths"] >= 0.0)
        assert dw <= 1e-7 and df <= 1e-6, (dw, df)


def test_cholesky_excitation_parts_against_the_dense_backend(dense_inp, chol_inp):
    be_d, be_f = scf.HipBackend(dense_inp, "B3LYP"), scf.HipBackend(chol_inp, "B3LYP")
    res = scf.run_scf(dense_inp, be_d, "B3LYP", **KW)
    assert res["converged"]
    n, nocc = dense_inp.shells.nao, dense_inp.nocc
    rng = np.random.default_rng(3)
    A, Bs = rng.standard_normal((n, nocc)), rng.standard_normal((9, n, nocc))
    for be in (be_d, be_f):
        be.response_prepare(res["dm"])
    Jd, Md, Vd = be_d.excitation_parts(A, Bs, True)
    Jf, Mf, Vf = be_f.excitation_parts(A, Bs, True)
    assert Jd.shape == Md.shape == Vd.shape == Jf.shape == Mf.shape == (9, n, n)
    for k in range(9):
        AB = A @ Bs[k].T
        for sgn in (1.0, -1.0):
            D = AB + sgn * AB.T
            bound = CHOL_TOL * np.abs(D).sum()
            Kd, Kf = Md[k] + sgn * Md[k].T, Mf[k] + sgn * Mf[k].T
            assert np.abs(Kf - Kd).max() <= bound, (k, sgn)
            ref = np.einsum("ikjl,kl->ij", dense_inp.eri, D)
            assert np.abs(Kd - ref).max() <= 1e-12 * np.abs(ref).max()
        D = AB + AB.T
        assert np.abs(Jf[k] - Jd[k]).max() <= CHOL_TOL * np.abs(D).sum()
        assert np.abs(Jd[k] - np.einsum("ijkl,kl->ij", dense_inp.eri, D)).max() <= 1e-12 * np.abs(Jd[k]).max()
    assert np.array_equal(Vd, Vf)                         # the same DFT_FxcApply on the same planes and table
    assert be_d.excitation_parts(A, Bs[:2], False)[1] is None
    be_f.world = 2
    with pytest.raises(ValueError, match="one rank"):
        be_f.excitation_parts(A, Bs, True)


def test_driver_reports_excitations(tmp_path):
    out = tmp_path / "run.jsonl"
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "H2O", "--basis", "def2-svp", "--grid-level", "1",
           "--excitations", "3", "--json", str(out)]
    for extra, method in (([], "tddft"), (["--tda"], "tda")):
        p = subprocess.run(cmd + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        rec = json.loads(out.read_text().strip().splitlines()[-1])
        w, f = np.array(rec["excitation_energies"]), np.array(rec["oscillator_strengths"])
        assert rec["converged"] and rec["excitation_method"] == method and 1 <= rec["excitation_iterations"] <= 60
        assert w.shape == (3,) and np.all(np.diff(w) > 0.0) and 0.2 < w[0] and w[-1] < 0.6
        assert f.shape == (3,) and np.all(f >= 0.0)
        assert "Singlet excitations" in p.stdout and "largest |X+Y|" in p.stdout
