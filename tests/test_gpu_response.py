"""response.polarizability on the device (HipBackend.response_parts: DFT_ComputeJK / DFT_ComputeJKFactorized and
DFT_FxcPrepare / DFT_FxcApply) for H2O / def2-SVP (24 functions), grid level 1.

* Dense ERI, GGA and B3LYP: the column alpha[:, z] against one finite-field derivative of the dipole moment run on the
  device, by the recipe of test_response_cpu.py: efield = +-F and +-F/2 along z, F = 2e-3, conv_e 1e-12, conv_dm 1e-9,
  value = (4 D(F/2) - D(F)) / 3, bar = |value - D(F/2)|, bound = 10 bar + the CPKS residual carried to alpha.
* Cholesky vectors: J and K of a CPKS trial density (K by linearity from two factorised calls) against the dense
  contraction, bound chol_tol * sum|dm1| -- |sum_kl R_ijkl D_kl| <= max|R| sum|D|, the relation of
  test_gpu_parity.test_factorised_jk_matches_dense_eri_oracle -- and alpha against the dense run.
* The driver's JSON record carries dipole, polarizability and cpks_iterations.
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

from quantum_compute_dft_amd import inputs, properties, response, scf  # noqa: E402

F0 = 2e-3
KW = dict(log=None, conv_e=1e-12, conv_dm=1e-9)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dense():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return inputs.build("H2O", "def2-svp", 1, verbose=False)


def in_field(inp, F):
    _, V_F, E_F = inputs.uniform_field(inp.symbols, inp.atom_xyz, inp.shells, F)
    return dataclasses.replace(inp, Hcore=inp.Hcore + V_F, E_nuc=inp.E_nuc + E_F, efield=np.asarray(F, dtype=np.float64))


def record(label, bar, err, extra=""):
    print(f"{label}: bar {bar:.2e}  error {err:.2e} {extra}")
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "response_parity.txt"), "a") as fh:
            fh.write(f"gpu  {label:40s} bar {bar:9.2e}   error {err:9.2e}   {extra}\n")


@pytest.mark.parametrize("functional", ["GGA", "B3LYP"])
def test_polarizability_against_finite_field_on_the_device(dense, functional):
    be = scf.HipBackend(dense, functional)
    assert not be.fused and not be.device_resident       # the host loop reads Hcore from the inputs: one backend serves every field
    res = scf.run_scf(dense, be, functional, **KW)
    assert res["converged"]
    out = response.polarizability(dense, res, be, functional)
    mu = {}
    for h in (F0, -F0, 0.5 * F0, -0.5 * F0):
        inp = in_field(dense, (0.0, 0.0, h))
        r = scf.run_scf(inp, be, functional, **KW)
        assert r["converged"]
        mu[h] = properties.dipole_moment(inp, r["dm"])
    D = lambda h: (mu[h] - mu[-h]) / (2.0 * h)
    value = (4.0 * D(0.5 * F0) - D(F0)) / 3.0
    bar = float(np.abs(value - D(0.5 * F0)).max())
    err = float(np.abs(out["alpha"][:, 2] - value).max())
    resid = 4.0 * max(np.linalg.norm(out["dipole_integrals"][k]) for k in range(3)) * max(out["residual"])
    record(f"alpha[:, z] H2O/def2-SVP {functional}", bar, err, f"CPKS iterations {out['cpks_iterations']} residual {max(out['residual']):.1e}")
    assert max(out["residual"]) <= 1e-8
    assert err <= 10.0 * bar + resid, (err, bar, resid)
    assert np.abs(out["alpha"] - out["alpha"].T).max() <= 10.0 * bar + resid


def test_cholesky_response_against_dense(dense):
    tol = 1e-8
    fact = inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=tol)
    kw = dict(KW, conv_e=1e-11)
    be_d, be_f = scf.HipBackend(dense, "B3LYP"), scf.HipBackend(fact, "B3LYP")
    r_d, r_f = scf.run_scf(dense, be_d, "B3LYP", **kw), scf.run_scf(fact, be_f, "B3LYP", **kw)
    assert r_d["converged"] and r_f["converged"]
    # the parts of one CPKS step, the same trial density on both backends
    rng = np.random.default_rng(2)
    n, nocc = dense.shells.nao, dense.nocc
    A, B = rng.standard_normal((n, nocc)), rng.standard_normal((n, nocc))
    dm1 = A @ B.T + B @ A.T
    for be, r in ((be_d, r_d), (be_f, r_f)):
        be.response_prepare(r["dm"])
    Jd, Kd, Vd = be_d.response_parts(dm1, True, (A, B))
    Jf, Kf, Vf = be_f.response_parts(dm1, True, (A, B))
    bound = tol * np.abs(dm1).sum()
    print(f"J {np.abs(Jf - Jd).max():.2e}  K {np.abs(Kf - Kd).max():.2e}  bound {bound:.2e}")
    assert np.abs(Jf - Jd).max() <= bound and np.abs(Kf - Kd).max() <= bound
    assert np.abs(Jd - np.einsum("ijkl,kl->ij", dense.eri, dm1)).max() <= 1e-12 * np.abs(Jd).max()
    assert np.abs(Kd - np.einsum("ikjl,kl->ij", dense.eri, dm1)).max() <= 1e-12 * np.abs(Kd).max()
    with pytest.raises(ValueError, match="factors"):
        be_f.response_parts(dm1, True)
    # alpha: a second-order property, stationary in the response -- the residual R of the ERI (max|R| <= tol) enters as
    # (1 + c_hf / 2) |dm1(k) : R : dm1(l)| <= (1 + c_hf / 2) tol sum|dm1(k)| sum|dm1(l)|; ten times that for what the
    # ground state's own shift (orbitals and gaps, first order in tol) adds through the third-order response
    a_d = response.polarizability(dense, r_d, be_d, "B3LYP")
    a_f = response.polarizability(fact, r_f, be_f, "B3LYP")
    s1 = max(np.abs(x).sum() for x in a_d["dm1"])
    bound_a = 10.0 * 1.1 * tol * s1 * s1
    err = float(np.abs(a_f["alpha"] - a_d["alpha"]).max())
    record("alpha Cholesky 1e-8 against dense, B3LYP", bound_a, err, f"CPKS iterations {a_f['cpks_iterations']}")
    assert err <= bound_a


def test_backends_that_cannot_respond_say_so(dense):
    be = scf.HipBackend(dense, "LDA", ao_mode="direct")
    with pytest.raises(ValueError, match="resident AO planes"):
        be.response_prepare(np.eye(dense.shells.nao))
    be = scf.HipBackend(dense, "LDA")
    be.world = 2
    with pytest.raises(ValueError, match="one rank"):
        be.response_parts(np.eye(dense.shells.nao), False)


def test_driver_reports_dipole_and_polarizability(tmp_path):
    out = tmp_path / "run.jsonl"
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "H2O", "--basis", "def2-svp", "--grid-level", "1",
           "--dipole", "--polarizability", "--json", str(out)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["converged"] and len(rec["dipole"]) == 3 and np.array(rec["polarizability"]).shape == (3, 3)
    assert len(rec["cpks_iterations"]) == 3 and all(1 <= n <= 30 for n in rec["cpks_iterations"])
    assert "Dipole moment (e bohr)" in p.stdout and "Static polarizability (a.u.)" in p.stdout
    a = np.array(rec["polarizability"])
    assert np.all(np.linalg.eigvalsh(0.5 * (a + a.T)) > 0.0) and 0.5 < np.linalg.norm(rec["dipole"]) < 1.2    # water: ~0.8 e bohr
