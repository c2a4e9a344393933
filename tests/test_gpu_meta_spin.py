"""DFT_ComputeTauSpin and DFT_ComputeXCMetaSpin -- the spin-resolved meta-GGA sweep on the device (k_tau_spin and
k_xc_points_meta_spin of csrc/xc_meta_spin.hip between the closed-shell sweep's density, contraction and reduce kernels and
the tau kernels of csrc/xc_meta.hip) -- against their host counterparts (metagga.tau_host / xc_meta_spin_host: the same
header through g++, pinned on the CPU by tests/test_meta_spin_cpu.py), and scf.run_uks(meta=True) on HipBackend.

Shapes: meta_spin_reference.SHAPES (the sweep and tau) and TAU_SHAPES (tau only: k_tau's K chunks).

Bounds.
* tau per spin: 1e-12 of max tau (tests/test_gpu_meta.py); tau_spin_fused 1 against 0: 1e-13 of max tau; each form twice: bitwise.
* V_s of the device against the host: fxc_reference.ERR_REL = 2e-8 of max|V| and Exc rel 1e-12 (+1e-14).
* meta_fused 1 against 0: 1e-13 of max|V|; the same call twice: bitwise.
* (dm/2, dm/2) against DFT_ComputeXCMeta(dm): meta_spin_reference.CLOSED_SHELL_BAR; zero meta weights against
  DFT_ComputeXCSpin: spin_reference.CLOSED_SHELL_BAR.
* End to end: 2e-8 Ha (E2E_BAR).

With QCDFT_WRITE_PROFILES set the figures are recorded as "gpu ..." lines of meta_spin_parity.txt in that directory.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fxc_reference as fr  # noqa: E402
import meta_spin_reference as ms  # noqa: E402
import spin_reference as sr  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import functionals, inputs, metagga, scf  # noqa: E402
from uks_meta_host_backend import UksMetaHostBackend  # noqa: E402

KW = dict(log=None, conv_e=1e-11, conv_dm=1e-9)
SENTINEL = 7.0


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


class Planes:
    """The inputs of one shape on the device (copies: the cached host arrays are shared between tests)."""

    def __init__(self, dev, shape, dms=None):
        self.dm_a, self.dm_b, self.ao, self.gr, self.w = ms.inputs(shape)
        if dms is not None:
            self.dm_a, self.dm_b = dms
        self.ngrid, self.nao, self.dev = shape[0], shape[1], dev
        t = lambda a: torch.as_tensor(np.array(a), device=dev)
        self.d_a, self.d_b, self.d_ao, self.d_gr, self.d_w = t(self.dm_a), t(self.dm_b), t(self.ao), t(self.gr), t(self.w)

    def _out(self, n=1):
        return [torch.full((self.nao, self.nao), SENTINEL, dtype=torch.float64, device=self.dev) for _ in range(n)]

    def meta_spin(self, s):
        va, vb = self._out(2)
        exc = s.compute_xc_meta_spin(self.ngrid, self.nao, self.d_a, self.d_b, self.d_ao, self.d_w, va, vb, self.d_gr)
        torch.cuda.synchronize()
        return exc, va.cpu().numpy(), vb.cpu().numpy()

    def spin(self, s):
        va, vb = self._out(2)
        exc = s.compute_xc_spin(self.ngrid, self.nao, self.d_a, self.d_b, self.d_ao, self.d_w, va, vb, self.d_gr)
        torch.cuda.synchronize()
        return exc, va.cpu().numpy(), vb.cpu().numpy()

    def meta(self, s, d_dm):
        v, = self._out()
        exc = s.compute_xc_meta(self.ngrid, self.nao, d_dm, self.d_ao, self.d_w, v, self.d_gr)
        torch.cuda.synchronize()
        return exc, v.cpu().numpy()

    def closed(self, s, d_dm):
        v, = self._out()
        exc = s.compute_xc(self.ngrid, self.nao, d_dm, self.d_ao, self.d_w, v, self.d_gr)
        torch.cuda.synchronize()
        return exc, v.cpu().numpy()

    def tau_spin(self, s):
        ta, tb = (torch.full((self.ngrid,), -3.0, dtype=torch.float64, device=self.dev) for _ in range(2))
        assert s.compute_tau_spin(self.ngrid, self.nao, self.d_a, self.d_b, self.d_gr, ta, tb) == 0
        torch.cuda.synchronize()
        return ta.cpu().numpy(), tb.cpu().numpy()

    def tau(self, s, d_dm):
        t = torch.full((self.ngrid,), -3.0, dtype=torch.float64, device=self.dev)
        assert s.compute_tau(self.ngrid, self.nao, d_dm, self.d_gr, t) == 0
        torch.cuda.synchronize()
        return t.cpu().numpy()


def same(x, y):
    return x[0] == y[0] and all(np.array_equal(a, b) for a, b in zip(x[1:], y[1:]))


def close(label, got, ref, bar=fr.ERR_REL):
    (e, va, vb), (e0, va0, vb0) = got, ref
    scale = float(max(np.abs(va0).max(), np.abs(vb0).max()))
    err = max(float(np.abs(va - va0).max()), float(np.abs(vb - vb0).max())) / scale
    print(f"{label}: Exc {e:.12f} (ref {e0:.12f}, rel {abs(e - e0) / abs(e0):.1e})  max|V| {scale:.3e}  err {err:.2e}")
    ms.record(f"gpu {label}", err, bar)
    assert np.isfinite(e) and np.all(np.isfinite(va)) and np.all(np.isfinite(vb)) and scale > 0.0, label
    assert e == pytest.approx(e0, rel=1e-12, abs=1e-14), label
    assert err <= bar, (label, err)


# ---- 0. what the code before this feature cannot do -----------------------------------------------------------------------
def test_the_entries_exist():
    lib = q.load_library(q.build_library())
    for name in ("DFT_ComputeTauSpin", "DFT_ComputeXCMetaSpin"):
        assert hasattr(lib, name), name
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5
    assert callable(getattr(scf.HipBackend, "uks_meta_parts", None))
    import inspect
    assert inspect.signature(scf.run_uks).parameters["meta"].default is False
    s = _solver("TPSS")
    assert callable(s.compute_tau_spin) and callable(s.compute_xc_meta_spin)
    assert s.get_option("tau_spin_fused") == 1.0                # the default is the form that measured faster (profiles/meta_spin_time.txt)


# ---- a. tau of both spins -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ms.SHAPES + ms.TAU_SHAPES, ids=str)
def test_tau_spin_against_the_host(dev, shape):
    p = Planes(dev, shape)
    want = ms.tau(shape)
    top = float(max(want[0].max(), want[1].max()))
    s = _solver("GGA")                                           # any solver
    before = p.tau(s, p.d_a)
    out = {}
    for fused in (0, 1):
        s.set_option("tau_spin_fused", fused)
        out[fused] = p.tau_spin(s)
        again = p.tau_spin(s)
        assert all(np.array_equal(x, y) for x, y in zip(out[fused], again))          # no atomics: bitwise reproducible
        err = max(float(np.abs(g - h).max()) for g, h in zip(out[fused], want)) / top
        print(f"tau spin {shape} fused={fused}: max tau {top:.3e}  err {err:.2e}")
        ms.record(f"gpu tau spin {shape} tau_spin_fused={fused}", err, 1e-12)
        assert all(np.all(np.isfinite(g)) for g in out[fused])
        assert err <= 1e-12
    both = max(float(np.abs(x - y).max()) for x, y in zip(out[0], out[1])) / top
    ms.record(f"gpu tau spin {shape} fused against plain", both, 1e-13)
    assert both <= 1e-13
    if shape[3] == 0:
        assert np.all(out[0][1] == 0.0) and np.all(out[1][1] == 0.0)
    assert np.array_equal(out[0][0], before)                     # the plain form is k_tau per spin
    assert np.array_equal(p.tau(s, p.d_a), before)               # DFT_ComputeTau is what it was


# ---- b. the sweep against the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ms.FUNCTIONALS)
@pytest.mark.parametrize("shape", ms.SHAPES, ids=str)
def test_device_against_the_host(dev, shape, functional):
    p = Planes(dev, shape)
    s = _solver(functional)
    assert s.get_option("meta_fused") == 0.0
    ref = ms.host(functional, shape)
    a = p.meta_spin(s)
    close(f"meta spin {functional} {shape}", a, ref)
    assert same(a, p.meta_spin(s))                               # the same call twice: bitwise
    s.set_option("tau_spin_fused", 0)
    close(f"meta spin {functional} {shape} tau_spin_fused=0", p.meta_spin(s), ref)
    s.set_option("tau_spin_fused", 1)
    s.set_option("meta_fused", 1)
    b = p.meta_spin(s)
    assert same(b, p.meta_spin(s))
    close(f"meta spin {functional} {shape} meta_fused=1", b, ref)
    scale = float(max(np.abs(a[1]).max(), np.abs(a[2]).max()))
    err = max(float(np.abs(a[1] - b[1]).max()), float(np.abs(a[2] - b[2]).max())) / scale
    ms.record(f"gpu meta spin {functional} {shape} meta_fused 1 against 0", err, 1e-13)
    assert a[0] == b[0] and err <= 1e-13
    if shape[3] == 0:
        assert np.all(a[2] == 0.0) and np.all(b[2] == 0.0)       # an empty channel: exactly zero, the sentinel overwritten


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("functional", ms.FUNCTIONALS)
@pytest.mark.parametrize("shape", ms.SHAPES, ids=str)
def test_validation_paths(dev, shape, functional, path):
    """The rho / sigma stage honours "path" (the VALU and the generic MFMA kernels); the tau kernels are the same."""
    close(f"meta spin {functional} {shape} path={path}", Planes(dev, shape).meta_spin(_solver(functional, path=path)), ms.host(functional, shape))


# ---- c. density matrices that are not positive semidefinite ----------------------------------------------------------------
@pytest.mark.parametrize("functional", ms.FUNCTIONALS)
@pytest.mark.parametrize("shape", [ms.SHAPES[0], ms.SHAPES[3], ms.SHAPES[4], ms.SHAPES[5]], ids=str)
def test_indefinite_density_matrices(dev, shape, functional):
    """dm_s - 0.3 I / 2.  At (2085, 24, 5, 4) 38 / 91 points of alpha / beta fall below the density cut-off and 47 more alpha
    points have tau < tau_W (z clamped); at nao = 50 hundreds do, and 9 to 56 live points have tau_s <= 0; the empty beta
    channels turn negative everywhere and stay absent."""
    dm_a, dm_b, ao, gr, w = ms.inputs(shape)
    shift = 0.15 * np.eye(shape[1])
    dms = (dm_a - shift, dm_b - shift)
    ra, ga, ta, rb, gb, tb = metagga.density_spin_host(*dms, ao, gr)
    live = ra >= 1e-12
    assert (~live).any() and (rb < 1e-12).any() and (live & (ta < np.sum(ga * ga, axis=1) / (8.0 * np.where(live, ra, 1.0)))).any()
    if shape[1] == 50:
        assert (live & (ta <= 0.0)).any()
    if shape[3] == 0:
        assert np.all(rb < 1e-12)
    got = Planes(dev, shape, dms).meta_spin(_solver(functional))
    close(f"meta spin indefinite {functional} {shape}", got, metagga.xc_meta_spin_host(functional, *dms, ao, w, gr))


# ---- d. closed-shell limits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ms.FUNCTIONALS)
@pytest.mark.parametrize("shape", ms.SHAPES[:3], ids=str)
def test_closed_shell_limit(dev, shape, functional):
    dm_a = ms.inputs(shape)[0]
    p = Planes(dev, shape, (dm_a, dm_a))
    s = _solver(functional)
    e, va, vb = p.meta_spin(s)
    e0, v0 = p.meta(s, torch.as_tensor(2.0 * dm_a, device=dev))
    fig = max(abs(e - e0) / abs(e0), float(np.abs(va - v0).max()) / float(np.abs(v0).max()), float(np.abs(vb - v0).max()) / float(np.abs(v0).max()))
    print(f"closed shell {functional} {shape}: {fig:.2e}")
    ms.record(f"gpu closed shell {functional} {shape} against DFT_ComputeXCMeta", fig, ms.CLOSED_SHELL_BAR)
    assert fig <= ms.CLOSED_SHELL_BAR


def _raw_meta_solver(lib, w8, w2):
    lib.DFT_CreateSolverMeta.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.DFT_CreateSolverMeta.restype = ctypes.c_void_p
    return lib.DFT_CreateSolverMeta((ctypes.c_double * len(w8))(*w8), len(w8), (ctypes.c_double * len(w2))(*w2), len(w2))


@pytest.mark.parametrize("mix", ["PBE0", "BLYP", "slater_x + pw92_c"])
@pytest.mark.parametrize("shape", ms.SHAPES[:4], ids=str)
def test_zero_meta_weights_give_the_spin_sweep(dev, shape, mix):
    p = Planes(dev, shape)
    f = functionals.resolve(mix)
    s = _solver(mix)
    lib = s.lib
    h = _raw_meta_solver(lib, f.weight_vector(), [0.0, 0.0])
    assert h
    try:
        zero = _solver(mix)
        lib.DFT_DestroySolver(ctypes.c_void_p(zero.solver))
        zero.solver = h                                           # the wrapper's calls on the meta solver with zero meta weights
        zero.set_option("quirks", 0)
        got = p.meta_spin(zero)
        ref = p.spin(s)
    finally:
        zero.solver = None
        lib.DFT_DestroySolver(ctypes.c_void_p(h))
    scale = float(max(np.abs(ref[1]).max(), np.abs(ref[2]).max()))
    fig = max(abs(got[0] - ref[0]) / abs(ref[0]), float(np.abs(got[1] - ref[1]).max()) / scale, float(np.abs(got[2] - ref[2]).max()) / scale)
    print(f"zero meta weights {mix} {shape}: {fig:.2e}")
    ms.record(f"gpu zero meta weights {mix} {shape} against DFT_ComputeXCSpin", fig, sr.CLOSED_SHELL_BAR)
    assert fig <= sr.CLOSED_SHELL_BAR


# ---- e. isolation and refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ms.SHAPES[:2], ids=str)
def test_other_entries_are_not_disturbed(dev, shape):
    """DFT_ComputeXCMeta, DFT_ComputeXCSpin and DFT_ComputeXC of a GGA solver before and after spin-meta calls in the same
    process: bitwise equal (at nao 24 with graph replay on, at nao 114 as plain launches)."""
    p = Planes(dev, shape)
    d_dm = torch.as_tensor(p.dm_a + p.dm_b, device=dev)
    g = _solver("GGA", graph=1 if shape[1] == 24 else 0)
    m = _solver("TPSS")
    before = ([p.closed(g, d_dm) for _ in range(3)][-1], p.spin(g), p.meta(m, d_dm))
    a = p.meta_spin(m)
    for fused in (1, 0):
        g.set_option("tau_spin_fused", fused)
        p.tau_spin(g)                                            # on the GGA solver itself
    g.set_option("graph", 1 if shape[1] == 24 else 0)
    for _ in range(3):
        assert same(p.closed(g, d_dm), before[0])
    assert same(p.spin(g), before[1]) and same(p.meta(m, d_dm), before[2])
    assert same(p.meta_spin(m), a)


def test_the_shared_workspace_carries_nothing_between_users(dev):
    """DFT_ComputeXCMeta, DFT_ComputeXCMetaSpin (meta_fused 0 and 1), DFT_ComputeTau and DFT_ComputeTauSpin on one TPSS solver,
    DFT_ComputeXCSpin, DFT_FxcPrepareSpinPol + DFT_FxcApplySpinPol and the two tau entries on one GGA solver: the entries of a
    solver work in one set of buffers, whose planes move as the sizes shrink and grow from call to call.  Each result is
    bitwise what the same call gives on a fresh solver that has run nothing else."""
    def calls(p, d_dm):
        def response(s):
            va, vb = p._out(2)
            assert s.fxc_prepare_spinpol(p.ngrid, p.nao, p.d_a, p.d_b, p.d_ao, p.d_w, p.d_gr) == 0
            assert s.fxc_apply_spinpol(p.ngrid, p.nao, p.d_b, p.d_a, p.d_ao, va, vb, p.d_gr) == 0
            torch.cuda.synchronize()
            return 0.0, va.cpu().numpy(), vb.cpu().numpy()
        tau = lambda s: (0.0, p.tau(s, d_dm))
        tau_spin = lambda s: (0.0,) + p.tau_spin(s)
        return [("TPSS", "meta", {}, lambda s: p.meta(s, d_dm)), ("TPSS", "meta spin", dict(meta_fused=0), p.meta_spin),
                ("TPSS", "meta spin fused", dict(meta_fused=1), p.meta_spin), ("GGA", "spin", {}, p.spin), ("GGA", "response", {}, response),
                ("TPSS", "tau", {}, tau), ("GGA", "tau", {}, tau), ("TPSS", "tau spin", dict(tau_spin_fused=1), tau_spin),
                ("GGA", "tau spin plain", dict(tau_spin_fused=0), tau_spin)]

    used = {"TPSS": _solver("TPSS"), "GGA": _solver("GGA")}
    order = (ms.SHAPES[0], ms.SHAPES[1], ms.SHAPES[0], ms.TAU_SHAPES[1])
    assert [(s[0], s[1]) for s in order] == [(2085, 24), (2085, 114), (2085, 24), (400, 385)]
    for shape in order:
        p = Planes(dev, shape)
        d_dm = torch.as_tensor(p.dm_a + p.dm_b, device=dev)
        for functional, label, opts, run in calls(p, d_dm):
            if shape == ms.TAU_SHAPES[1] and "tau" not in label:
                continue                                             # the two-chunk shape: tau alone
            opts = dict(dict(meta_fused=0, tau_spin_fused=1), **opts)    # the options are the solver's: the same on both
            fresh = _solver(functional, **opts)
            for k, v in opts.items():
                used[functional].set_option(k, v)
            assert same(run(used[functional]), run(fresh)), (shape, functional, label)


def test_refusals(dev):
    shape = ms.SHAPES[0]
    p = Planes(dev, shape)
    s = _solver("TPSS")
    s._declare_meta_spin()
    lib, u64 = s.lib, ctypes.c_uint64
    va, vb = p._out(2)
    exc = ctypes.c_double(0.0)
    ptr = lambda t: u64(0 if t is None else t.data_ptr())

    def call(solver, a=p.d_a, b=p.d_b, ao=p.d_ao, w=p.d_w, gr=p.d_gr, oa=va, ob=vb, e=exc, ngrid=p.ngrid, nao=p.nao):
        rc = lib.DFT_ComputeXCMetaSpin(solver.solver, ngrid, nao, ptr(a), ptr(b), ptr(ao), ptr(w), ptr(gr), ptr(oa), ptr(ob),
                                       ctypes.byref(e) if e is not None else None)
        return rc, solver.last_error()

    assert call(s) == (0, "")
    good = p.meta_spin(s)
    for kw in (dict(a=None), dict(b=None), dict(ao=None), dict(w=None), dict(gr=None), dict(oa=None), dict(ob=None), dict(e=None)):
        va.fill_(SENTINEL)
        rc, msg = call(s, **kw)
        assert rc == -1 and "DFT_ComputeXCMetaSpin needs" in msg and "ao_grad" in msg, (kw, msg)
        torch.cuda.synchronize()
        if "oa" not in kw:
            assert bool((va == SENTINEL).all()), kw                 # no kernel launched
    for kw in (dict(ngrid=0), dict(nao=0), dict(ngrid=-5)):
        rc, msg = call(s, **kw)
        assert rc == -1 and "bad sizes" in msg, kw
    assert same(p.meta_spin(s), good)                            # ... and the solver is still usable
    # a solver without meta weights
    g = _solver("GGA")
    g._declare_meta_spin()
    rc, msg = call(g)
    assert rc == -1 and "DFT_CreateSolverMeta" in msg and "no meta-GGA weights" in msg
    assert np.isfinite(p.spin(g)[0])
    # quirks = 1 with vwn5_c / pbe_c
    for functional, refused in (("tpss_x + pbe_c", True), ("tpss_c + slater_x + 0.2*vwn5_c", True), ("TPSS", False)):
        sq = _solver(functional, quirks=1)
        sq._declare_meta_spin()
        rc, msg = call(sq)
        assert (rc == -1 and "quirks = 1" in msg and "DFT_ComputeXCMetaSpin" in msg) if refused else (rc, msg) == (0, ""), functional
        sq.set_option("quirks", 0)
        assert call(sq) == (0, "")
    # every entry that refused a meta solver still does
    with pytest.raises(RuntimeError, match="meta-GGA"):
        s.compute_xc_spin(p.ngrid, p.nao, p.d_a, p.d_b, p.d_ao, p.d_w, va, vb, p.d_gr)
    with pytest.raises(RuntimeError, match="meta-GGA"):
        s.compute_xc(p.ngrid, p.nao, p.d_a, p.d_ao, p.d_w, va, p.d_gr)
    torch.cuda.synchronize()
    assert same(p.meta_spin(s), good)
    # DFT_ComputeTauSpin
    s.compute_tau_spin  # declared above
    t = torch.zeros(p.ngrid, dtype=torch.float64, device=dev)
    for args in ((0, p.nao, ptr(p.d_a), ptr(p.d_b), ptr(p.d_gr), ptr(t), ptr(t)), (p.ngrid, p.nao, ptr(None), ptr(p.d_b), ptr(p.d_gr), ptr(t), ptr(t)),
                 (p.ngrid, p.nao, ptr(p.d_a), ptr(p.d_b), ptr(None), ptr(t), ptr(t)), (p.ngrid, p.nao, ptr(p.d_a), ptr(p.d_b), ptr(p.d_gr), ptr(t), ptr(None))):
        assert lib.DFT_ComputeTauSpin(s.solver, *args) == -1 and s.last_error() != ""


def test_backend_refusals(dev):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, charge=1, spin=1)
    n = inp.shells.nao
    z, c = np.zeros((n, n)), np.zeros((n, 1))
    be = scf.HipBackend(inp, "TPSS", quirks=False)
    with pytest.raises(ValueError, match="meta-GGA") as e:
        be.uks_parts(z, z, c, c, False)
    assert "not built" in str(e.value) and "uks_meta_parts" in str(e.value)
    for f in (lambda: be.uks_response_prepare(z, z), lambda: be.xc_gradient(z), lambda: be.xc_grid_response(z)):
        with pytest.raises(ValueError, match="meta-GGA"):
            f()
    gga = scf.HipBackend(inp, "PBE0", quirks=False, fused_tail=False, device_resident=False)
    with pytest.raises(ValueError, match="uks_meta_parts") as e:
        gga.uks_meta_parts(z, z, c, c, False)
    assert "not" in str(e.value) and "PBE0" in str(e.value)
    with pytest.raises(ValueError, match="meta=False"):
        scf.run_uks(inp, gga, "PBE0", log=None, meta=True)


# ---- f. end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cation():
    """H2O+ doublet / def2-SVP with the dense ERI and the host loop's results per functional, once."""
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False, charge=1, spin=1)
    cache = {}

    def ref(functional):
        if functional not in cache:
            cache[functional] = scf.run_uks(inp, UksMetaHostBackend(inp, functional), functional, meta=True, **KW)
        return cache[functional]
    return inp, ref


@pytest.mark.parametrize("eri", ["dense", "cholesky"])
@pytest.mark.parametrize("functional", ["TPSS", "TPSSh"])
def test_water_cation_on_the_device_against_the_host_loop(dev, cation, functional, eri):
    inp, ref = cation
    ref = ref(functional)
    if eri == "cholesky":
        inp = inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=1e-10, charge=1, spin=1)
    be = scf.HipBackend(inp, functional, quirks=False, fused_tail=False, device_resident=False, eigensolver="exact")
    assert be.meta and not be.xc_occ
    res = scf.run_uks(inp, be, functional, meta=True, **KW)
    print(f"H2O+ {functional}/def2-SVP {eri}: device {res['E_tot']:.10f}  host {ref['E_tot']:.10f}  diff {res['E_tot'] - ref['E_tot']:+.2e}  "
          f"<S^2> {res['s_squared']:.6f} (host {ref['s_squared']:.6f})")
    ms.record(f"gpu uks H2O+ {functional} def2-SVP {eri} against the host loop (Ha)", abs(res["E_tot"] - ref["E_tot"]), ms.E2E_BAR)
    assert ref["converged"] and res["converged"] and (res["nalpha"], res["nbeta"]) == (5, 4)
    assert abs(res["E_tot"] - ref["E_tot"]) <= ms.E2E_BAR
    assert 0.75 <= res["s_squared"] < 0.80
