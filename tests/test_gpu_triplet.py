"""DFT_FxcPrepareSpin / DFT_FxcApplyKind -- the tables of the spin-resolved energy bodies on the device
(k_fxc_table_spin, csrc/xc_response.hip) and the triplet excitations on top of them -- against the host counterpart
(response.fxc_apply_host(kind=...): the same header through g++, pinned on the CPU by tests/test_triplet_cpu.py).

Shapes: the (nao, nocc) of tests/test_gpu_fxc.py's table with a few thousand grid points each, no multiple of 256:
(2057, 24, 6) the one-kernel path, (3333, 114, 21) the wave-specialised path at a ragged nao, (2160, 130, 26) nao > 128.

Bounds.
* V1 of the device against V1 of the host: ERR_REL = 2e-8 of max|V1|, the bound of tests/test_gpu_fxc.py.
* The table, point by point (test_device_table_point_by_point): TABLE_BAR = 2e-11 of the largest entry.  The host table
  is within 6.4e-13 of the 60-digit reference (profiles/triplet_parity.txt); the device runs the same fp64 statements
  with contraction and its own libm (a few ulp), an error of the same kind and size, so device against host is at most
  three times that, 2e-12; times the same factor ten of headroom the host bar has.
* Prepare through the occupied orbitals against Prepare through dm0: 1e-11 (tests/test_gpu_fxc.py, tests/test_gpu_occ.py).
* End to end: |dw| <= 1e-7 Ha, the bound of tests/test_gpu_excitations.py.

With QCDFT_WRITE_PROFILES set every figure printed here is also recorded, one "gpu ..." line per case, in
triplet_parity.txt of that directory (triplet_reference.record): how the gpu lines of profiles/triplet_parity.txt were made.
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

import excitation_dense as ed  # noqa: E402
import fxc_reference as fr  # noqa: E402
import triplet_reference as tr  # noqa: E402
from quantum_compute_dft_amd import excitations as ex  # noqa: E402
from quantum_compute_dft_amd import response, scf  # noqa: E402
from test_gpu_excitations import KW, HostOnDevicePlanes, chol_inp, dense_inp  # noqa: E402,F401
from test_gpu_fxc import Planes, _solver, dev  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2057, 24, 6), (3333, 114, 21), (2160, 130, 26)]
MIX = "0.5*pbe_x+0.3*b88_x+0.7*lyp_c+0.2*pw92_c+0.4*pbe_c+0.1*vwn5_c"
TABLE_BAR = 2e-11
KINDS = {1: "triplet", 2: "singlet-spin"}


def planes(dev, shape, functional, **kw):
    kw.setdefault("seed", 1)
    return Planes(dev, *shape, need_grad=functional != "LDA", **kw)


def prepare_spin(p, s, kind, cocc=None):
    if cocc is None:
        return s.fxc_prepare_spin(p.ngrid, p.nao, p.d_dm0, p.d_ao, p.d_w, p.d_gr, kind=kind)
    d_c = torch.as_tensor(np.ascontiguousarray(cocc), device=p.dev)
    rc = s.fxc_prepare_spin(p.ngrid, p.nao, None, p.d_ao, p.d_w, p.d_gr, d_c, cocc.shape[1], kind=kind)
    torch.cuda.synchronize()
    return rc


def apply_kind(p, s, kind, dm1=None):
    d_dm1 = p.d_dm1 if dm1 is None else torch.as_tensor(np.ascontiguousarray(dm1), device=p.dev)
    d_v = torch.full((p.nao, p.nao), 7.0, dtype=torch.float64, device=p.dev)
    assert s.fxc_apply_kind(p.ngrid, p.nao, d_dm1, p.d_ao, d_v, p.d_gr, kind=kind) == 0
    torch.cuda.synchronize()
    return d_v.cpu().numpy()


def host(p, functional, kind, dm1=None):
    gga = functional != "LDA"
    return response.fxc_apply_host(functional, p.dm0, p.dm1 if dm1 is None else dm1, p.ao, p.w, p.gr if gga else None,
                                   quirks=False, kind=KINDS[kind])


def close(label, v1, ref, bar=fr.ERR_REL):
    scale = float(np.abs(ref).max())
    err = float(np.abs(v1 - ref).max()) / scale
    print(f"{label}: max|V1| {scale:.3e}  err {err:.2e}")
    tr.record(f"gpu {label}", err, bar)
    assert np.all(np.isfinite(v1)) and scale > 0.0, label
    assert err <= bar, (label, err)


# ---- 1. the table, point by point --------------------------------------------------------------------------------------
class PointPlanes:
    """One basis function per grid point (ao the identity, ao_grad diagonal): rho, grad rho and V1[g, g] belong to point g
    alone, V1[g, g] = w (T0 r1 + T1 s1 + (T2 r1 + T3 s1) g.b + T4 g1.b) with b the point's AO gradient -- the device table
    read back through DFT_FxcApplyKind, all five planes at every point.  rho log-spaced over [1e-7, 10], the reduced
    gradient cycling through {0.05, 0.3, 1, 3}; every eleventh point has no density at all."""

    def __init__(self, dev, n):
        rng = np.random.default_rng(n)
        rho = np.logspace(-7, 1, n)
        rho[::11] = 0.0
        s = np.array([0.05, 0.3, 1.0, 3.0])[np.arange(n) % 4]
        b = rng.standard_normal((n, 3))
        b *= (np.cbrt(3.0 * np.pi ** 2 * rho) * s / np.linalg.norm(b, axis=1))[:, None]       # sigma = (2 kF rho s)^2
        self.ngrid = self.nao = n
        self.dm0, self.dm1 = np.diag(rho), np.diag(0.3 * rho * rng.choice([-1.0, 1.0], n))
        self.ao = np.eye(n)
        self.gr = np.stack([np.diag(b[:, k]) for k in range(3)])
        self.w = 0.05 * rng.random(n) + 0.01
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        self.dev = dev
        self.d_dm0, self.d_dm1, self.d_ao, self.d_gr, self.d_w = t(self.dm0), t(self.dm1), t(self.ao), t(self.gr), t(self.w)
        self.empty = rho == 0.0


@pytest.mark.parametrize("kind", [1, 2], ids=["triplet", "singlet"])
@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", MIX])
@pytest.mark.parametrize("n", [24, 114, 130])
def test_device_table_point_by_point(dev, n, functional, kind):
    p = PointPlanes(dev, n)
    if functional == "LDA":
        p.d_gr = None
    s = _solver(functional, 0)
    assert prepare_spin(p, s, kind) == 0
    v1, ref = apply_kind(p, s, kind), host(p, functional, kind)
    assert np.all(np.diag(v1)[p.empty] == 0.0) and np.all(np.diag(ref)[p.empty] == 0.0)      # rows with no density
    assert np.count_nonzero(np.diag(ref)) >= n - np.count_nonzero(p.empty) - 1
    close(f"table {functional[:12]} kind {kind} n={n}", v1, ref, TABLE_BAR)


# ---- 2. DFT_FxcApplyKind against fxc_apply_host ------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", "PBE0"])
@pytest.mark.parametrize("shape", SHAPES)
def test_triplet_response_against_the_host(dev, shape, functional):
    p = planes(dev, shape, functional)
    s = _solver(functional, 0)
    assert prepare_spin(p, s, 1) == 0
    close(f"triplet {functional} {shape}", apply_kind(p, s, 1), host(p, functional, 1))


@pytest.mark.parametrize("functional", ["GGA", "B3LYP"])
def test_singlet_through_the_spin_bodies_is_the_shipped_singlet(dev, functional):
    """kind 2 against DFT_FxcApply at quirks = 0 on the device itself: two tables that agree to 1e-14 on the host."""
    p = planes(dev, SHAPES[1], functional)
    s = _solver(functional, 0)
    assert p.prepare(s) == 0 and prepare_spin(p, s, 2) == 0
    close(f"kind 2 against DFT_FxcApply {functional}", apply_kind(p, s, 2), p.apply(s), 1e-11)


def test_non_symmetric_perturbation(dev):
    p = planes(dev, SHAPES[1], "GGA", symmetric=False)
    assert np.abs(p.dm1 - p.dm1.T).max() > 0.0
    s = _solver("GGA", 0)
    assert prepare_spin(p, s, 1) == 0
    v1 = apply_kind(p, s, 1)
    close("triplet GGA non-symmetric dm1", v1, host(p, "GGA", 1))
    close("triplet GGA, the symmetric part alone", apply_kind(p, s, 1, 0.5 * (p.dm1 + p.dm1.T)), v1, 1e-12)


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP"])
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_prepare_through_occupied_orbitals(dev, shape, functional):
    p = planes(dev, shape, functional)
    lam, V = np.linalg.eigh(p.dm0)
    nocc = shape[2]
    cocc = V[:, -nocc:] * np.sqrt(lam[-nocc:])
    assert np.abs(cocc @ cocc.T - p.dm0).max() <= 1e-13 * np.abs(p.dm0).max()
    s = _solver(functional, 0)
    assert prepare_spin(p, s, 1) == 0
    a = apply_kind(p, s, 1)
    s2 = _solver(functional, 0, occ=1)
    assert prepare_spin(p, s2, 1, cocc) == 0
    assert s2.get_option("used_occ") == 1.0
    close(f"triplet cocc against dm0 {functional} {shape}", apply_kind(p, s2, 1), a, 1e-11)


# ---- 3. interleaving ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_the_two_prepares_and_the_applies_interleave(dev, shape, functional):
    p = planes(dev, shape, functional)
    alone = _solver(functional, 1)
    assert p.prepare(alone) == 0
    singlet = p.apply(alone)
    s = _solver(functional, 1)
    assert p.prepare(s) == 0
    other = planes(dev, (shape[0] + 40, shape[1], shape[2]), functional, seed=3)          # the triplet table at ANOTHER dm0 and grid
    assert prepare_spin(other, s, 1) == 0
    assert np.array_equal(p.apply(s), singlet)                                           # the singlet table was not disturbed
    assert np.array_equal(apply_kind(p, s, 0), singlet)                                  # kind 0 is DFT_FxcApply
    assert prepare_spin(p, s, 1) == 0 and prepare_spin(p, s, 2) == 0
    first = apply_kind(p, s, 1)
    assert np.array_equal(p.apply(s), singlet)
    assert np.array_equal(apply_kind(p, s, 1), first)
    d_v = torch.zeros((shape[1], shape[1]), dtype=torch.float64, device=dev)
    exc = s.compute_xc(other.ngrid, other.nao, other.d_dm0 * 1.3, other.d_ao, other.d_w, d_v, other.d_gr)
    torch.cuda.synchronize()
    assert np.isfinite(exc)
    assert np.array_equal(apply_kind(p, s, 1), first) and np.array_equal(p.apply(s), singlet)
    s.set_option("quirks", 0)                                                            # invalidates the shipped table only
    assert np.array_equal(apply_kind(p, s, 1), first)
    with pytest.raises(RuntimeError, match="invalidated"):
        p.apply(s)
    assert not np.array_equal(first, singlet)


# ---- 4. error returns --------------------------------------------------------------------------------------------------
def test_error_returns(dev):
    p = Planes(dev, 96, 5, 3)
    s = _solver("GGA", 0)
    L, u64 = s.lib, ctypes.c_uint64
    ptr = lambda x: u64(0 if x is None else x.data_ptr())
    d_v = torch.zeros((5, 5), dtype=torch.float64, device=dev)

    def apply(ngrid, nao, gr, kind):
        rc = L.DFT_FxcApplyKind(s.solver, ngrid, nao, ptr(p.d_dm1), ptr(p.d_ao), ptr(gr), ptr(d_v), kind)
        return rc, s.last_error()

    def prepare(gr, kind):
        rc = L.DFT_FxcPrepareSpin(s.solver, p.ngrid, p.nao, 0, u64(0), ptr(p.d_dm0), ptr(p.d_ao), ptr(gr), ptr(p.d_w), kind)
        return rc, s.last_error()

    for kind in (0, 3, -1):
        rc, msg = prepare(p.d_gr, kind)
        assert rc == -1 and "unknown kind" in msg
    rc, msg = apply(p.ngrid, p.nao, p.d_gr, 3)
    assert rc == -1 and "unknown kind" in msg
    rc, msg = apply(p.ngrid, p.nao, p.d_gr, 1)
    assert rc == -1 and "before DFT_FxcPrepareSpin" in msg
    rc, msg = prepare(None, 1)
    assert rc == -1 and "ao_grad pointer is null" in msg
    assert prepare(p.d_gr, 1) == (0, "")
    rc, msg = apply(p.ngrid, p.nao, p.d_gr, 2)                      # the other kind's slot is still empty
    assert rc == -1 and "before DFT_FxcPrepareSpin" in msg
    rc, msg = apply(p.ngrid, p.nao, p.d_gr, 0)                      # and so is DFT_FxcPrepare's
    assert rc == -1 and "before DFT_FxcPrepare" in msg
    rc, msg = apply(p.ngrid + 1, p.nao, p.d_gr, 1)
    assert rc == -1 and "differ from" in msg
    rc, msg = apply(p.ngrid, p.nao - 1, p.d_gr, 1)
    assert rc == -1 and "differ from" in msg
    rc, msg = apply(p.ngrid, p.nao, None, 1)
    assert rc == -1 and "ao_grad pointer is null" in msg
    assert apply(p.ngrid, p.nao, p.d_gr, 1) == (0, "")              # the solver is still usable
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="before DFT_FxcPrepareSpin"):    # through the wrapper: an exception, no abort
        _solver("LDA").fxc_apply_kind(p.ngrid, p.nao, p.d_dm1, p.d_ao, d_v, kind=1)
    with pytest.raises(RuntimeError, match="unknown kind"):
        s.fxc_prepare_spin(p.ngrid, p.nao, p.d_dm0, p.d_ao, p.d_w, p.d_gr, kind=7)
    assert np.isfinite(apply_kind(p, s, 1)).all()


def test_backends_that_cannot_respond_say_so(dense_inp):
    be = scf.HipBackend(dense_inp, "B3LYP")
    dm = np.eye(dense_inp.shells.nao)
    for attr, value, text in (("world", 2, "one rank"), ("ao_mode", "direct", "resident AO planes")):
        old = getattr(be, attr)
        setattr(be, attr, value)
        with pytest.raises(ValueError, match=text):
            be.response_prepare(dm, kind="triplet")
        setattr(be, attr, old)


# ---- 5. timings --------------------------------------------------------------------------------------------------------
def test_timings_name_the_spin_table_kernel(dev):
    p = planes(dev, SHAPES[0], "GGA")
    s = _solver("GGA", 0, profile=1)
    assert prepare_spin(p, s, 1) == 0
    assert [n for n, _ in s.timings()] == ["rho", "fxc_table_spin"]
    apply_kind(p, s, 1)
    assert [n for n, _ in s.timings()] == ["rho", "fxc_coef", "fxc_vxc", "fxc_reduce"]


# ---- 6. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional,eri", [("LDA", "dense"), ("B3LYP", "dense"), ("B3LYP", "cholesky")])
def test_device_triplets_against_the_host_built_dense_solution(dense_inp, chol_inp, functional, eri):
    inp = dense_inp if eri == "dense" else chol_inp
    be = scf.HipBackend(inp, functional, quirks=False)
    res = scf.run_scf(inp, be, functional, **KW)
    assert res["converged"]
    host_inp = inp if eri == "dense" else dataclasses.replace(inp, eri=np.einsum("pij,pkl->ijkl", inp.chol, inp.chol))
    ops = ex.ResponseOperators(host_inp, res, HostOnDevicePlanes(host_inp, functional, be), functional, triplet=True)
    ApB, AmB = ed.dense_matrices(ops)
    for tda in (True, False):
        out = ex.excitations(inp, res, be, functional, nroots=3, tda=tda, triplet=True)
        w, _ = ed.dense_solution(ops, ApB, AmB, tda)
        dw = float(np.abs(out["energies"] - w[:3]).max())
        singlet = ex.excitations(inp, res, be, functional, nroots=1, tda=tda)["energies"][0]
        print(f"H2O/def2-SVP {functional} {eri} triplet {'TDA' if tda else 'TDDFT'}: |dw| {dw:.2e} Ha  w = "
              f"{' '.join(f'{x:.6f}' for x in out['energies'])}  lowest singlet {singlet:.6f}  iterations {out['iterations']}")
        tr.record(f"gpu H2O/def2-SVP {functional} {eri} triplet {'TDA' if tda else 'TDDFT'}, three roots against dense (Ha)", dw, 1e-7)
        assert out["converged"] and out["method"] == ("tda-triplet" if tda else "tddft-triplet")
        assert np.all(np.diff(out["energies"]) > 0.0) and np.all(out["oscillator_strengths"] == 0.0)
        assert dw <= 1e-7, dw
        assert 0.0 < out["energies"][0] < singlet


def test_triplet_parts_request_no_coulomb_and_share_the_exchange(dense_inp):
    be = scf.HipBackend(dense_inp, "B3LYP", quirks=False)
    res = scf.run_scf(dense_inp, be, "B3LYP", **KW)
    n, nocc = dense_inp.shells.nao, dense_inp.nocc
    rng = np.random.default_rng(3)
    A, Bs = rng.standard_normal((n, nocc)), rng.standard_normal((3, n, nocc))
    be.response_prepare(res["dm"])
    be.response_prepare(res["dm"], kind="triplet")
    Js, Ms, Vs = be.excitation_parts(A, Bs, True)
    Jt, Mt, Vt = be.excitation_parts(A, Bs, True, kind="triplet")
    assert Jt is None and Js is not None and np.array_equal(Ms, Mt) and not np.array_equal(Vs, Vt)
    assert np.array_equal(be.excitation_parts(A, Bs, True)[2], Vs)


def test_driver_reports_triplets(tmp_path):
    out = tmp_path / "run.jsonl"
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "H2O", "--basis", "def2-svp", "--grid-level", "1",
           "--quirks", "0", "--excitations", "3", "--json", str(out)]
    recs = []
    for extra in (["--triplets"], []):
        p = subprocess.run(cmd + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        recs.append((json.loads(out.read_text().strip().splitlines()[-1]), p.stdout))
    (t, t_out), (s, s_out) = recs
    assert t["excitation_method"] == "tddft-triplet" and t["excitation_multiplicity"] == 3 and "Triplet excitations" in t_out and "  T1 " in t_out
    assert s["excitation_method"] == "tddft" and s["excitation_multiplicity"] == 1 and "Singlet excitations" in s_out and "  S1 " in s_out
    w = np.array(t["excitation_energies"])
    assert w.shape == (3,) and np.all(np.diff(w) > 0.0) and np.all(np.array(t["oscillator_strengths"]) == 0.0)
    ws = np.array(s["excitation_energies"])
    # every triplet below the singlet of the same rank (the singlet has the Coulomb term 2 (ia|jb) on top, positive
    # semidefinite), the lowest triplet below everything; in H2O only that one lies under the first singlet
    assert 0.0 < w[0] < ws[0] and np.all(w < ws)
