"""DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol -- the open-shell response of Vxc on the device (k_fxc_table_pol and
k_fxc_coef_pol, csrc/xc_response_pol.hip, between the sweep's density, contraction and reduce kernels) -- against the host
counterpart (response.fxc_table_pol_host / HostFxcSpin: the same header through g++, pinned on the CPU by
tests/test_spin_response_cpu.py), and the UKS solvers on HipBackend.uks_excitation_parts.

Shapes: test_gpu_spin.SHAPES -- an ngrid that is no multiple of 256, nao on both sides of 128, a ragged width, and the fully
polarised (2085, 50, 3, 0).

Bounds.
* Table, point by point: |device - host| <= HESSIAN_BAR of the plane's largest entry.  The two evaluate the same statements
  and differ in rounding only (contraction into fused multiply-adds, the device's log / exp / cbrt); the host's own distance
  from the 60-digit reference is within HESSIAN_BAR per entry.  Relative to the plane because an entry next to a sign change
  has no relative accuracy in either (a host build with fused multiply-adds moves single entries by 4e-11 of themselves
  and no plane by more than 4e-13 of its maximum at these shapes).  A plane of an absent channel is exactly zero.
* V1_s of the device against fxc_apply_spinpol_host: fxc_reference.ERR_REL = 2e-8 of max|V1_s|.
* Closed-shell limit against DFT_FxcApplyKind kinds 2 and 1 on the device: ERR_REL as well (two device results).
* Spin swap: 1e-13 of max|V1|, the bound of test_gpu_spin.py for the potentials.
* Isolation: bit for bit.
* Roots |dw| <= 1e-7 Ha, |df| <= 1e-6: the bar of tests/test_gpu_excitations.py.  U-CPKS alpha: the device against the host
  on the device's planes, 1e-6 a.u. -- V1 at 2e-8 of O(1) matrix elements through |D_k|^2 / gap ~ 10, plus two GMRES
  residuals of 1e-8 carried the same way.

With QCDFT_WRITE_PROFILES set the figures are recorded as "gpu ..." lines of spin_response_parity.txt in that directory.
"""
import ctypes
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fxc_reference as fr  # noqa: E402
import spin_reference as sr  # noqa: E402
import spin_response_reference as rr  # noqa: E402
import uks_excitation_dense as ued  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import excitations as ex  # noqa: E402
from quantum_compute_dft_amd import inputs, response, scf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2085, 24, 5, 4), (2085, 114, 21, 20), (1100, 130, 9, 7), (2085, 50, 3, 0)]
KW = dict(log=None, conv_e=1e-11, conv_dm=1e-9)


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

    def __init__(self, dev, shape, functional, symmetric=True):
        self.da, self.db, self.d1a, self.d1b, self.ao, gr, self.w = rr.perturbed_inputs(*shape, symmetric=symmetric)
        self.gr = _grad(functional, gr)
        self.functional, self.ngrid, self.nao, self.dev = functional, shape[0], shape[1], dev
        t = lambda a: torch.as_tensor(np.array(a), device=dev)
        self.d_da, self.d_db, self.d_d1a, self.d_d1b = t(self.da), t(self.db), t(self.d1a), t(self.d1b)
        self.d_ao, self.d_w = t(self.ao), t(self.w)
        self.d_gr = t(self.gr) if self.gr is not None else None

    def prepare(self, s, d_a=None, d_b=None):
        assert s.fxc_prepare_spinpol(self.ngrid, self.nao, self.d_da if d_a is None else d_a, self.d_db if d_b is None else d_b,
                                     self.d_ao, self.d_w, self.d_gr) == 0

    def apply(self, s, d_a=None, d_b=None):
        va, vb = (torch.full((self.nao, self.nao), 7.0, dtype=torch.float64, device=self.dev) for _ in range(2))
        assert s.fxc_apply_spinpol(self.ngrid, self.nao, self.d_d1a if d_a is None else d_a, self.d_d1b if d_b is None else d_b,
                                   self.d_ao, va, vb, self.d_gr) == 0
        torch.cuda.synchronize()
        return va.cpu().numpy(), vb.cpu().numpy()

    def host(self):
        return response.fxc_apply_spinpol_host(self.functional, self.da, self.db, self.d1a, self.d1b, self.ao, self.w, self.gr)


def close(label, got, ref, bar=fr.ERR_REL):
    worst = 0.0
    for s, v, r in zip("ab", got, ref):
        scale = float(np.abs(r).max())
        assert np.all(np.isfinite(v)), label
        if scale == 0.0:                                   # the absent spin
            assert np.all(v == 0.0), label
            continue
        err = float(np.abs(v - r).max()) / scale
        print(f"{label} V1_{s}: max|V1| {scale:.3e}  err {err:.2e}")
        worst = max(worst, err)
    rr.record(f"gpu {label}", worst, bar)
    assert worst <= bar, (label, worst)


# ---- 0. what the parent cannot do ---------------------------------------------------------------------------------------
def test_the_entries_exist():
    lib = q.load_library(q.build_library())
    assert hasattr(lib, "DFT_FxcPrepareSpinPol") and hasattr(lib, "DFT_FxcApplySpinPol")
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5


# ---- 1. the table, point by point ---------------------------------------------------------------------------------------
def _host_planes(functional, p):
    """The device's plane layout from the host's (5, 5, n) table: (planes, n)."""
    ra, ga = response._density(p.da, p.ao, p.gr)
    rb, gb = response._density(p.db, p.ao, p.gr)
    H, g = response.fxc_table_pol_host(functional, ra, rb, ga, gb)
    sw = (0.5 if functional == "B3LYP" else 1.0) * p.w
    if p.gr is None:
        return np.stack([H[0, 0], H[0, 1], H[1, 1]]) * sw
    pairs = [(i, j) for i in range(5) for j in range(i, 5)]
    lower = [(j, i) for i in range(4) for j in range(i + 1, 5)]
    return np.stack([H[i, j] for i, j in pairs] + [g[2], g[3], g[4]] + [H[j, i] for j, i in lower]) * sw


@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_device_table_against_the_host_table(dev, shape, functional):
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    p.prepare(s)
    got = s.fxc_spinpol_table(p.ngrid, dev).cpu().numpy()
    ref = _host_planes(functional, p)
    assert got.shape == ref.shape == ((28 if p.gr is not None else 3), p.ngrid)
    assert np.all(np.isfinite(got))
    scale = np.abs(ref).max(axis=1)
    assert np.all(got[scale == 0.0] == 0.0)                 # rows and columns of an absent channel
    live = scale > 0.0
    err = (np.abs(got - ref).max(axis=1)[live] / scale[live])
    print(f"table {functional} {shape}: worst plane {int(np.flatnonzero(live)[np.argmax(err)])}  err {err.max():.2e}")
    rr.record(f"gpu table {functional} {shape}", float(err.max()), rr.HESSIAN_BAR)
    if shape[3] == 0:
        assert (~live).sum() == (2 if p.gr is None else 28 - 5)   # what stays: H_00 (LDA), and H_02, H_20, H_22, g_2 with it
    else:      # all planes but the sigma-sigma ones B88 + LYP leave empty (LYP is linear in the sigmas, B88 is per spin)
        assert live.all() if functional in ("LDA", "GGA", "PBE0") else (~live).sum() == 4 + 3
    assert err.max() <= rr.HESSIAN_BAR


# ---- 2. apply against the host --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_apply_against_the_host(dev, shape, functional):
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    p.prepare(s)
    got = p.apply(s)
    close(f"apply {functional} {shape}", got, p.host())
    if shape[3] == 0:
        assert np.all(got[1] == 0.0)
        again = p.apply(s, None, torch.zeros_like(p.d_d1b))
        assert np.array_equal(again[0], got[0]) and np.all(again[1] == 0.0)       # a beta perturbation changes nothing


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
def test_validation_paths(dev, functional, path):
    p = Planes(dev, SHAPES[0], functional)
    s = _solver(functional, path=path)
    p.prepare(s)
    close(f"apply {functional} {SHAPES[0]} path={path}", p.apply(s), p.host())


@pytest.mark.parametrize("functional", ["GGA", "B3LYP"])
def test_only_the_symmetric_part_of_dm1_counts(dev, functional):
    p = Planes(dev, SHAPES[1], functional, symmetric=False)
    assert np.abs(p.d1a - p.d1a.T).max() > 0.0
    s = _solver(functional)
    p.prepare(s)
    got = p.apply(s)
    close(f"apply {functional} {SHAPES[1]} non-symmetric dm1", got, p.host())
    sym = p.apply(s, torch.as_tensor(0.5 * (p.d1a + p.d1a.T), device=dev), torch.as_tensor(0.5 * (p.d1b + p.d1b.T), device=dev))
    close(f"apply {functional} {SHAPES[1]} dm1 against its symmetric part", got, sym, 1e-13)


# ---- 3. closed-shell limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_closed_shell_limit_on_the_device(dev, shape, functional):
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    d_dm0, d_half = torch.as_tensor(p.da + p.db, device=dev), torch.as_tensor(0.5 * (p.da + p.db), device=dev)
    d_h1 = torch.as_tensor(0.5 * p.d1a, device=dev)
    p.prepare(s, d_half, d_half)
    for kind, sign in ((2, 1.0), (1, -1.0)):
        s.fxc_prepare_spin(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr, kind=kind)
        d_v = torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev)
        assert s.fxc_apply_kind(p.ngrid, p.nao, p.d_d1a, p.d_ao, d_v, p.d_gr, kind=kind) == 0
        torch.cuda.synchronize()
        ref = d_v.cpu().numpy()
        va, vb = p.apply(s, d_h1, sign * d_h1)
        close(f"closed shell {functional} {shape} kind {kind}", (va, sign * vb), (ref, ref))


# ---- 4. spin swap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_spin_swap(dev, shape, functional):
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    p.prepare(s)
    va, vb = p.apply(s)
    p.prepare(s, p.d_db, p.d_da)
    ub, ua = p.apply(s, p.d_d1b, p.d_d1a)
    scale = max(float(np.abs(va).max()), float(np.abs(vb).max()))
    err = max(float(np.abs(va - ua).max()), float(np.abs(vb - ub).max())) / scale
    print(f"swap {functional} {shape}: err {err:.2e}")
    rr.record(f"gpu swap {functional} {shape}", err, 1e-13)
    assert all(np.all(np.isfinite(x)) for x in (va, vb, ua, ub))
    assert err <= 1e-13


# ---- 5. isolation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ["GGA", "B3LYP"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_isolation(dev, shape, functional):
    """The DFT_FxcPrepare table, the kind-1 table and the SpinPol table live side by side: Applies of each are bit-identical
    before and after the others' Prepare / Apply and after DFT_ComputeXC and DFT_ComputeXCSpin calls in between."""
    p = Planes(dev, shape, functional)
    s = _solver(functional)
    d_dm0 = torch.as_tensor(p.da + p.db, device=dev)

    def closed(kind):
        d_v = torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev)
        assert s.fxc_apply_kind(p.ngrid, p.nao, p.d_d1a, p.d_ao, d_v, p.d_gr, kind=kind) == 0
        torch.cuda.synchronize()
        return d_v.cpu().numpy()

    def sweeps():
        v, v2 = (torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev) for _ in range(2))
        s.compute_xc(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, v, p.d_gr)
        s.compute_xc_spin(p.ngrid, p.nao, p.d_da, p.d_db, p.d_ao, p.d_w, v, v2, p.d_gr)
        torch.cuda.synchronize()

    s.fxc_prepare(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr)
    s.fxc_prepare_spin(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr, kind=1)
    before = [closed(0), closed(1)]
    p.prepare(s)
    pol = p.apply(s)
    assert np.array_equal(closed(0), before[0]) and np.array_equal(closed(1), before[1])
    sweeps()
    again = p.apply(s)
    assert np.array_equal(again[0], pol[0]) and np.array_equal(again[1], pol[1])
    s.fxc_prepare(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr)                  # and vice versa
    s.fxc_prepare_spin(p.ngrid, p.nao, d_dm0, p.d_ao, p.d_w, p.d_gr, kind=1)
    assert np.array_equal(closed(0), before[0]) and np.array_equal(closed(1), before[1])
    sweeps()
    again = p.apply(s)
    assert np.array_equal(again[0], pol[0]) and np.array_equal(again[1], pol[1])
    assert np.array_equal(closed(0), before[0]) and np.array_equal(closed(1), before[1])


# ---- 6. error returns and timings -------------------------------------------------------------------------------------------
def test_error_returns(dev):
    p = Planes(dev, SHAPES[0], "GGA")
    s = _solver("GGA")
    lib, u64 = s.lib, ctypes.c_uint64
    va, vb = (torch.zeros((p.nao, p.nao), dtype=torch.float64, device=dev) for _ in range(2))
    ptr = lambda t: u64(0 if t is None else t.data_ptr())

    def prepare(solver, da=p.d_da, db=p.d_db, ao=p.d_ao, gr=p.d_gr, w=p.d_w, ngrid=p.ngrid, nao=p.nao):
        return lib.DFT_FxcPrepareSpinPol(solver.solver, ngrid, nao, ptr(da), ptr(db), ptr(ao), ptr(gr), ptr(w)), solver.last_error()

    def apply(solver, da=p.d_d1a, db=p.d_d1b, ao=p.d_ao, gr=p.d_gr, a=va, b=vb, ngrid=p.ngrid, nao=p.nao):
        return lib.DFT_FxcApplySpinPol(solver.solver, ngrid, nao, ptr(da), ptr(db), ptr(ao), ptr(gr), ptr(a), ptr(b)), solver.last_error()

    rc, msg = apply(s)
    assert rc == -1 and "before DFT_FxcPrepareSpinPol" in msg
    for kw in (dict(da=None), dict(db=None), dict(ao=None), dict(w=None)):
        rc, msg = prepare(s, **kw)
        assert rc == -1 and "DFT_FxcPrepareSpinPol needs" in msg, (kw, msg)
    rc, msg = prepare(s, gr=None)
    assert rc == -1 and "ao_grad pointer is null" in msg
    for kw in (dict(ngrid=0), dict(nao=0)):
        rc, msg = prepare(s, **kw)
        assert rc == -1 and "bad sizes" in msg
    assert prepare(s) == (0, "")
    for kw in (dict(da=None), dict(db=None), dict(ao=None), dict(a=None), dict(b=None)):
        rc, msg = apply(s, **kw)
        assert rc == -1 and "DFT_FxcApplySpinPol needs" in msg, (kw, msg)
    rc, msg = apply(s, gr=None)
    assert rc == -1 and "ao_grad pointer is null" in msg
    for kw in (dict(ngrid=p.ngrid - 1), dict(nao=p.nao - 1)):
        rc, msg = apply(s, **kw)
        assert rc == -1 and "differ from DFT_FxcPrepareSpinPol's" in msg
    assert apply(s) == (0, "")
    rc, msg = prepare(s, ngrid=0)                                  # a failed Prepare leaves nothing to apply
    assert rc == -1 and apply(s)[0] == -1
    for functional, refused in (("GGA", True), ("LDA", True), ("0.5*slater_x+0.1*vwn5_c+b88_x", True), ("B3LYP", False), ("BLYP", False)):
        rc, msg = prepare(_solver(functional, quirks=1))
        assert (rc == -1 and "quirks = 1" in msg and "not the derivatives of their energies" in msg) if refused else (rc, msg) == (0, ""), functional
    with pytest.raises(RuntimeError, match="run with --quirks 0"):       # through the wrapper: an exception, no abort
        p.prepare(_solver("GGA", quirks=1))
    torch.cuda.synchronize()


def test_timings_name_the_new_kernels(dev):
    p = Planes(dev, SHAPES[1], "GGA")
    s = _solver("GGA", profile=1)
    p.prepare(s)
    assert [n for n, _ in s.timings()] == ["rho", "rho", "fxc_table_pol"]
    p.apply(s)
    t = s.timings()
    assert [n for n, _ in t] == ["rho", "rho", "fxc_coef_pol", "fxc_vxc", "fxc_reduce", "fxc_vxc", "fxc_reduce"]
    assert all(ms > 0.0 for _, ms in t)


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def _backend(inp, functional):
    return scf.HipBackend(inp, functional, quirks=False, device_resident=False, fused_tail=False, eigensolver="exact")


class HostOnDevicePlanes(response.HostUksResponse):
    """HostUksResponse on the AO planes of a HipBackend; the ground-state Fock parts come from that backend."""

    def __init__(self, inp, functional, be):
        gr = be.d_gr.cpu().numpy() if be.d_gr is not None else None
        super().__init__(inp, functional, be, be.d_ao.cpu().numpy(), gr)


@pytest.mark.parametrize("eri", ["dense", "cholesky"])
def test_water_cation_roots_and_alpha_against_the_host(dev, eri):
    functional = "B3LYP"
    kw = dict(eri_mode="cholesky", chol_tol=1e-10) if eri == "cholesky" else {}
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False, charge=1, spin=1, **kw)
    be = _backend(inp, functional)
    res = scf.run_uks(inp, be, functional, **KW)
    assert res["converged"]
    host_inp = inp if eri == "dense" else dataclasses.replace(inp, eri=np.einsum("pij,pkl->ijkl", inp.chol, inp.chol))
    hb = HostOnDevicePlanes(host_inp, functional, be)
    ops = ex.UksResponseOperators(host_inp, res, hb, functional)
    assert ops.size == 5 * 19 + 4 * 20
    ApB, AmB = ued.dense_matrices(ops)
    for tda in (True, False):
        out = ex.excitations(inp, res, be, functional, nroots=3, tda=tda)
        w, f = ued.dense_solution(ops, ApB, AmB, tda)
        dw, df = float(np.abs(out["energies"] - w[:3]).max()), float(np.abs(out["oscillator_strengths"] - f[:3]).max())
        print(f"H2O+ {functional} {eri} {'U-TDA' if tda else 'U-TDDFT'}: |dw| {dw:.2e} |df| {df:.2e}  w {out['energies']}  iterations {out['iterations']}")
        rr.record(f"gpu uks H2O+ B3LYP def2-SVP {eri} {'U-TDA' if tda else 'U-TDDFT'} roots against the host-built dense solution (Ha)", dw, 1e-7)
        assert out["converged"] and out["method"] == ("tda-uks" if tda else "tddft-uks") and out["multiplicity"] is None
        assert dw <= 1e-7 and df <= 1e-6, (dw, df)
    a_dev = response.polarizability(inp, res, be, functional)
    a_host = response.polarizability(host_inp, res, hb, functional)
    da = float(np.abs(a_dev["alpha"] - a_host["alpha"]).max())
    print(f"H2O+ {functional} {eri} U-CPKS alpha: |device - host| {da:.2e}  iso {np.trace(a_dev['alpha']) / 3.0:.6f}  iterations {a_dev['cpks_iterations']}")
    rr.record(f"gpu uks H2O+ B3LYP def2-SVP {eri} U-CPKS alpha against the host (a.u.)", da, 1e-6)
    assert max(a_dev["residual"]) <= 1e-8 and da <= 1e-6


def test_backend_refusals_and_an_empty_spin(dev):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    n = inp.shells.nao
    z, c = np.zeros((n, n)), np.zeros((n, 1))
    for kw, text in ((dict(ao_mode="direct"), "--ao direct"), (dict(xc_occ=False, dm_factor=True), "dm_factor")):
        be = scf.HipBackend(inp, "B3LYP", quirks=False, **{**dict(device_resident=False, fused_tail=False), **kw})
        with pytest.raises(ValueError, match=text):
            be.uks_response_prepare(z, z)
        with pytest.raises(ValueError, match=text):
            be.uks_excitation_parts(c, c[None], c, c[None], True)
    be = _backend(inp, "B3LYP")
    rng = np.random.default_rng(2)
    ca = 0.5 * rng.standard_normal((n, 3))
    be.uks_response_prepare(ca @ ca.T, z)
    A, Bs = rng.standard_normal((n, 3)), rng.standard_normal((2, n, 3))
    J, Ma, Mb, Va, Vb = be.uks_excitation_parts(A, Bs, np.zeros((n, 0)), np.zeros((2, n, 0)), True)
    D = np.einsum("mi,kni->kmn", A, Bs)
    assert np.abs(J - np.einsum("ijkl,nkl->nij", inp.eri, D + D.transpose(0, 2, 1))).max() <= 1e-12 * np.abs(J).max()
    assert np.abs(Ma - np.einsum("ikjl,nkl->nij", inp.eri, D)).max() <= 1e-12 * np.abs(Ma).max()
    assert np.all(Mb == 0.0) and np.all(Vb == 0.0) and Va.any() and np.all(np.isfinite(Va))
    be.world = 2
    with pytest.raises(ValueError, match="one rank"):
        be.uks_excitation_parts(A, Bs, np.zeros((n, 0)), np.zeros((2, n, 0)), True)


def test_driver(dev, tmp_path):
    out = tmp_path / "uks.json"
    base = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "H2O", "--grid-level", "1", "--quirks", "0", "--spin", "1", "--charge", "1"]
    flags = ["--dipole", "--polarizability", "--excitations", "2"]
    r = subprocess.run(base + ["--open-shell-response", "--json", str(out)] + flags, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["uks"] is True and rec["converged"] and rec["spin"] == 1
    assert len(rec["dipole"]) == 3 and np.array(rec["polarizability"]).shape == (3, 3) and len(rec["cpks_iterations"]) == 3
    w, f = np.array(rec["excitation_energies"]), np.array(rec["oscillator_strengths"])
    assert w.shape == (2,) and np.all(np.diff(w) >= 0.0) and w[0] > 0.0 and f.shape == (2,) and np.all(f >= 0.0)
    assert rec["excitation_method"] == "tddft-uks" and rec["excitation_multiplicity"] is None and rec["excitation_iterations"] >= 1
    assert "  U1 " in r.stdout and "  U2 " in r.stdout and "Static polarizability" in r.stdout and "Dipole moment" in r.stdout
    r = subprocess.run(base + flags, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "closed-shell reference" in r.stderr and "--open-shell-response" in r.stderr
    r = subprocess.run(base + ["--open-shell-response", "--excitations", "2", "--triplets"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--triplets" in r.stderr
