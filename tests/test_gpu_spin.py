"""DFT_ComputeXCSpin -- the spin-resolved sweep on the device (k_xc_points_spin, csrc/xc_spin.hip, between the closed-shell
sweep's density, contraction and reduce kernels) -- against its host counterpart (response.xc_spin_host: the same header
through g++, pinned on the CPU by tests/test_spin_potential_cpu.py), and scf.run_uks on HipBackend.uks_parts.

Shapes (ngrid, nao, nalpha, nbeta), densities cocc_s cocc_s^T of random orbitals:
  (2085, 24, 5, 4)     DFT_ComputeXC would take the one-kernel plan or a recorded graph here
  (2085, 114, 21, 20)  the wave-specialised path, fringe width 114 = 7 x 16 + 2, a ragged last 256-block
  (1100, 130, 9, 7)    the path for nao > 128
  (2085, 50, 3, 0)     fully polarised

Bounds.
* V_s of the device against the host: ERR_REL = 2e-8 of max|V_s|, the bar tests/test_gpu_triplet.py applies to
  DFT_FxcApplyKind against fxc_apply_host.  Exc: rel 1e-12 (+1e-14), the Exc bound of tests/test_gpu_parity.py's sweep
  against the oracle.
* Closed-shell limit (dm/2, dm/2) against DFT_ComputeXC(dm) at quirks 0 and against the oracle: spin_reference.CLOSED_SHELL_BAR,
  what the host test measured (times ten) on the same plane shapes.
* Spin swap: V to 1e-13 of max|V|, Exc to the Exc bound.
* End to end: 2e-8 Ha, the fused-against-host bound of tests/test_gpu_scf_tail.py.

With QCDFT_WRITE_PROFILES set the figures are recorded as "gpu ..." lines of spin_parity.txt in that directory.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fxc_reference as fr  # noqa: E402
import helpers  # noqa: E402
import spin_reference as sr  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import inputs, response, scf  # noqa: E402
from uks_host_backend import UksHostBackend  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2085, 24, 5, 4), (2085, 114, 21, 20), (1100, 130, 9, 7), (2085, 50, 3, 0)]
KW = dict(log=None, conv_e=1e-11, conv_dm=1e-9)
E2E_BAR = 2e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(functional, quirks=0, **opts):
    s = q.DFTSolverWrapper(q.build_library(), functional)
    s.set_option("quirks", quirks)
    for k, v in opts.items():
        s.set_option(k, v)
    return s


def _grad(functional, gr):
    return gr if functional != "LDA" else None


class Planes:
    """The inputs of one shape on the device (copies: the cached host arrays are shared between tests)."""

    def __init__(self, dev, shape, functional):
        self.da, self.db, self.ao, gr, self.w, _, _ = sr.spin_inputs(*shape)
        self.gr = _grad(functional, gr)
        self.ngrid, self.nao, self.dev = shape[0], shape[1], dev
        t = lambda a: torch.as_tensor(np.array(a), device=dev)
        self.d_da, self.d_db, self.d_ao, self.d_w = t(self.da), t(self.db), t(self.ao), t(self.w)
        self.d_gr = t(self.gr) if self.gr is not None else None

    def spin(self, s, d_a=None, d_b=None):
        va, vb = (torch.full((self.nao, self.nao), 7.0, dtype=torch.float64, device=self.dev) for _ in range(2))
        exc = s.compute_xc_spin(self.ngrid, self.nao, self.d_da if d_a is None else d_a, self.d_db if d_b is None else d_b,
                                self.d_ao, self.d_w, va, vb, self.d_gr)
        torch.cuda.synchronize()
        return exc, va.cpu().numpy(), vb.cpu().numpy()

    def closed(self, s, d_dm):
        v = torch.full((self.nao, self.nao), 7.0, dtype=torch.float64, device=self.dev)
        exc = s.compute_xc(self.ngrid, self.nao, d_dm, self.d_ao, self.d_w, v, self.d_gr)
        torch.cuda.synchronize()
        return exc, v.cpu().numpy()


@pytest.fixture(scope="module")
def host():
    """xc_spin_host per (functional, shape), computed once."""
    cache = {}

    def get(functional, shape):
        if (functional, shape) not in cache:
            da, db, ao, gr, w, _, _ = sr.spin_inputs(*shape)
            cache[functional, shape] = response.xc_spin_host(functional, da, db, ao, w, _grad(functional, gr))
        return cache[functional, shape]
    return get


def close(label, got, ref, bar=fr.ERR_REL):
    (e, va, vb), (e0, va0, vb0) = got, ref
    scale = max(float(np.abs(va0).max()), float(np.abs(vb0).max()))
    err = max(float(np.abs(va - va0).max()), float(np.abs(vb - vb0).max())) / scale
    print(f"{label}: Exc {e:.12f} (ref {e0:.12f}, rel {abs(e - e0) / abs(e0):.1e})  max|V| {scale:.3e}  err {err:.2e}")
    sr.record(f"gpu {label}", err, bar)
    assert np.isfinite(e) and np.all(np.isfinite(va)) and np.all(np.isfinite(vb)) and scale > 0.0, label
    assert e == pytest.approx(e0, rel=1e-12, abs=1e-14), label
    assert err <= bar, (label, err)


# ---- 0. what today's code cannot do -------------------------------------------------------------------------------------
def test_the_entry_exists():
    lib = q.load_library(q.build_library())
    assert hasattr(lib, "DFT_ComputeXCSpin")
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5
    assert inputs.build("H2O", "sto-3g", grid_level=1, verbose=False, charge=1, spin=1).nalpha == 5


# ---- 1. device against xc_spin_host -------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_device_against_the_host(dev, host, shape, functional):
    p = Planes(dev, shape, functional)
    got = p.spin(_solver(functional))
    close(f"spin {functional} {shape}", got, host(functional, shape))
    if shape[3] == 0:                     # fully polarised: nothing for the absent spin
        assert np.all(got[2] == 0.0)


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
def test_validation_paths(dev, host, functional, path):
    p = Planes(dev, SHAPES[0], functional)
    close(f"spin {functional} {SHAPES[0]} path={path}", p.spin(_solver(functional, path=path)), host(functional, SHAPES[0]))


# ---- 2. closed-shell limit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_closed_shell_limit_on_the_device(dev, shape, functional):
    p = Planes(dev, shape, functional)
    dm, _, gr, _ = helpers.synth_inputs(shape[0], shape[1])      # the planes of spin_inputs, its own dm
    assert np.array_equal(gr, sr.spin_inputs(*shape)[3])
    d_dm, d_half = torch.as_tensor(dm, device=dev), torch.as_tensor(0.5 * dm, device=dev)
    s = _solver(functional)
    e, va, vb = p.spin(s, d_half, d_half)
    e_c, v_c = p.closed(s, d_dm)
    e_o, v_o = sr.closed_shell_reference(functional, dm, p.ao, p.w, gr)
    worst = 0.0
    for what, e0, v0 in (("DFT_ComputeXC", e_c, v_c), ("oracle", e_o, v_o)):
        de = abs(e - e0) / abs(e0)
        dv = max(float(np.abs(va - v0).max()), float(np.abs(vb - v0).max())) / float(np.abs(v0).max())
        print(f"closed shell {functional} {shape} against {what}: Exc {de:.2e}  V {dv:.2e}")
        sr.record(f"gpu closed shell {functional} {shape} against {what}", max(de, dv), sr.CLOSED_SHELL_BAR)
        worst = max(worst, de, dv)
    assert worst <= sr.CLOSED_SHELL_BAR


# ---- 3. spin swap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_spin_swap(dev, shape, functional):
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    e, va, vb = p.spin(s)
    e2, vb2, va2 = p.spin(s, p.d_db, p.d_da)
    scale = max(float(np.abs(va).max()), float(np.abs(vb).max()))
    err = max(float(np.abs(va - va2).max()), float(np.abs(vb - vb2).max())) / scale
    print(f"swap {functional} {shape}: err {err:.2e}  Exc rel {abs(e - e2) / abs(e):.1e}")
    sr.record(f"gpu swap {functional} {shape}", err, 1e-13)
    assert all(np.all(np.isfinite(x)) for x in (va, vb, va2, vb2)) and np.isfinite(e) and np.isfinite(e2)
    assert e2 == pytest.approx(e, rel=1e-12, abs=1e-14)
    assert err <= 1e-13


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ["GGA", "B3LYP"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_isolation(dev, shape, functional):
    """Two identical spin calls are bitwise equal, and DFT_ComputeXC before and after a spin call is bitwise equal -- at nao 24
    with graph replay on (the third and later calls of a key are replays), at nao 114 as plain launches."""
    p = Planes(dev, shape, functional)
    s = _solver(functional, graph=1 if shape[1] == 24 else 0)
    d_dm = torch.as_tensor(p.da + p.db, device=dev)
    v = torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev)

    def closed():
        e = s.compute_xc(p.ngrid, p.nao, d_dm, p.d_ao, p.d_w, v, p.d_gr)
        torch.cuda.synchronize()
        return e, v.cpu().numpy()

    before = [closed() for _ in range(3)][-1]
    a = p.spin(s)
    b = p.spin(s)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for _ in range(3):
        after = closed()
        assert after[0] == before[0] and np.array_equal(after[1], before[1])
    c = p.spin(s)
    assert a[0] == c[0] and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])


@pytest.mark.parametrize("kind", [0, 1])
def test_a_prepared_response_table_survives(dev, kind):
    shape, functional = SHAPES[1], "B3LYP"
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    d_dm0 = torch.as_tensor(p.da + p.db, device=dev)
    d_dm1 = torch.as_tensor(p.da - p.db, device=dev)

    def apply():
        d_v = torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev)
        assert s.fxc_apply_kind(p.ngrid, p.nao, d_dm1, p.d_ao, d_v, p.d_gr, kind=kind) == 0
        torch.cuda.synchronize()
        return d_v.cpu().numpy()

    if kind:
        s.fxc_prepare_spin(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr, kind=kind)
    else:
        s.fxc_prepare(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr)
    before = apply()
    p.spin(s)
    assert np.array_equal(apply(), before)


# ---- 5. error paths -------------------------------------------------------------------------------------------------------
def test_error_paths(dev):
    shape = SHAPES[0]
    p = Planes(dev, shape, "GGA")
    s = _solver("GGA")
    lib, u64 = s.lib, ctypes.c_uint64
    va, vb = (torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev) for _ in range(2))
    exc = ctypes.c_double(0.0)
    ptr = lambda t: u64(0 if t is None else t.data_ptr())

    def call(solver, da=p.d_da, db=p.d_db, ao=p.d_ao, gr=p.d_gr, w=p.d_w, a=va, b=vb, e=exc, ngrid=p.ngrid):
        rc = lib.DFT_ComputeXCSpin(solver.solver, ngrid, p.nao, ptr(da), ptr(db), ptr(ao), ptr(gr), ptr(w), ptr(a), ptr(b),
                                   ctypes.byref(e) if e is not None else None)
        return rc, solver.last_error()

    assert call(s) == (0, "")
    for kw in (dict(da=None), dict(db=None), dict(ao=None), dict(w=None), dict(a=None), dict(b=None), dict(e=None)):
        rc, msg = call(s, **kw)
        assert rc == -1 and "DFT_ComputeXCSpin needs" in msg, (kw, msg)
    rc, msg = call(s, gr=None)
    assert rc == -1 and "ao_grad pointer is null" in msg
    rc, msg = call(s, ngrid=0)
    assert rc == -1 and "bad sizes" in msg
    for functional, refused in (("GGA", True), ("LDA", True), ("0.5*slater_x+0.1*vwn5_c+b88_x", True), ("B3LYP", False), ("BLYP", False)):
        sq = _solver(functional, quirks=1)
        rc, msg = call(sq)
        assert (rc == -1 and "quirks = 1" in msg and "not the derivatives of their energies" in msg) if refused else (rc, msg) == (0, ""), functional
    with pytest.raises(RuntimeError, match="run with --quirks 0"):       # through the wrapper: an exception, no abort
        p.spin(_solver("GGA", quirks=1))
    assert call(s) == (0, "")


# ---- 6. end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cation():
    """H2O+ doublet, def2-SVP: the inputs with the dense ERI and the host loop's result, once."""
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False, charge=1, spin=1)
    return inp, scf.run_uks(inp, UksHostBackend(inp, "B3LYP"), "B3LYP", **KW)


def _backend(inp, functional):
    return scf.HipBackend(inp, functional, quirks=False, device_resident=False, fused_tail=False, eigensolver="exact")


@pytest.mark.parametrize("eri", ["dense", "cholesky"])
def test_water_cation_on_the_device_against_the_host_loop(dev, cation, eri):
    inp, ref = cation
    if eri == "cholesky":
        inp = inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=1e-10, charge=1, spin=1)
    res = scf.run_uks(inp, _backend(inp, "B3LYP"), "B3LYP", **KW)
    print(f"H2O+ B3LYP/def2-SVP {eri}: device {res['E_tot']:.10f}  host {ref['E_tot']:.10f}  diff {res['E_tot'] - ref['E_tot']:+.2e}  <S^2> {res['s_squared']:.6f}")
    sr.record(f"gpu uks H2O+ B3LYP def2-SVP {eri} against the host loop (Ha)", abs(res["E_tot"] - ref["E_tot"]), E2E_BAR)
    assert ref["converged"] and res["converged"]
    assert abs(res["E_tot"] - ref["E_tot"]) <= E2E_BAR
    assert 0.75 <= res["s_squared"] < 0.80 and abs(res["s_squared"] - ref["s_squared"]) <= 1e-6


def test_spin_zero_on_the_device_against_the_restricted_loop(dev):
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    be = _backend(inp, "B3LYP")
    rks = scf.run_scf(inp, be, "B3LYP", **KW)
    uks = scf.run_uks(inp, be, "B3LYP", **KW)
    print(f"H2O B3LYP/def2-SVP: RKS {rks['E_tot']:.10f}  UKS spin 0 {uks['E_tot']:.10f}  diff {uks['E_tot'] - rks['E_tot']:+.2e}")
    sr.record("gpu uks spin 0 against the device rks H2O B3LYP def2-SVP (Ha)", abs(uks["E_tot"] - rks["E_tot"]), E2E_BAR)
    assert rks["converged"] and uks["converged"]
    assert abs(uks["E_tot"] - rks["E_tot"]) <= E2E_BAR
    assert abs(uks["s_squared"]) <= 1e-8


def test_uks_parts_refuses_what_it_cannot_do(dev):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    z = np.zeros((inp.shells.nao, inp.shells.nao))
    c = np.zeros((inp.shells.nao, 1))
    for kw, text in ((dict(ao_mode="direct"), "--ao direct"), (dict(xc_occ=False, dm_factor=True), "dm_factor"),
                     (dict(device_resident=True), "host loop"), (dict(fused_tail=True, eigensolver="rotate"), "host loop")):
        kw = {**dict(device_resident=False, fused_tail=False), **kw}
        with pytest.raises(ValueError, match=text):
            scf.HipBackend(inp, "B3LYP", quirks=False, **kw).uks_parts(z, z, c, c, True)


def test_driver_flags(dev, tmp_path):
    out = tmp_path / "uks.json"
    base = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "H2O", "--grid-level", "1", "--quirks", "0"]
    r = subprocess.run(base + ["--charge", "1", "--spin", "1", "--json", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["uks"] is True and rec["spin"] == 1 and rec["charge"] == 1 and rec["converged"] and 0.75 <= rec["s_squared"] < 0.80
    r = subprocess.run(base + ["--charge", "1"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--spin" in r.stdout + r.stderr
    for flag in (["--excitations", "2"], ["--polarizability"], ["--dipole"]):
        r = subprocess.run(base + ["--spin", "0"] + flag, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "closed-shell reference" in r.stderr, flag
