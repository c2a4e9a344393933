"""DFT_ComputeXCGradientMetaSpin / DFT_ComputeXCEnergyDensityMetaSpin (csrc/xc_grad_meta_spin.hip) against their host
counterparts (gradients.xc_gradient_meta_spin_host / xc_energy_density_meta_spin_host), which
tests/test_uks_meta_gradient_cpu.py holds against finite differences of metagga.xc_meta_spin_host's Exc.

* Device against host: 2e-8 of max|G| (tests/test_gpu_xc_gradient.py's ERR_REL), for TPSS, TPSSh and a mix with one meta
  component, in both forms of option xcg_meta_spin_fused.  Shapes (ngrid, nao, n_alpha, n_beta) on
  tests/uks_meta_gradient_reference.py's planes: (2085, 24, 5, 4), (2085, 114, 9, 7) seven whole column tiles and two columns,
  a ragged last tile of rows, more tiles than one round of workgroups; (1100, 130, 9, 7) past 128, nine column tiles: three
  rounds of the four waves; (37, 50, 6, 5) one ragged tile of rows after two whole ones, ragged columns; (2085, 50, 3, 0)
  fully polarised, D_b = 0; (333, 50, 1, 1) and (333, 50, 1, 0) one orbital (z = 1 to rounding).  K chunks at 37 rows, the
  caps read from the headers: the six-tile cap of k_xc_grad_meta_spin, one column above it, three chunks with a ragged last
  one, and the same for the two caps of the plain form (k_xc_grad's and k_xc_grad_meta<false>'s).  path 1 and 2.
* Fused against plain 1e-13 of max|G|; each form twice bitwise; two ragged grid slices against the whole 1e-12.
* dm_s - 0.15 I and dm_s - 0.3 I (indefinite: channels below the cut-off, z clamped; tau <= 0 at the second): finite, and
  the host's to the same 2e-8.
* (dm/2, dm/2) against DFT_ComputeXCGradientMeta(dm) 4e-14; zero meta weights against DFT_ComputeXCGradientSpin 4e-14.
* DFT_ComputeXCEnergyDensityMetaSpin against the host 1e-12 of max|e|; sum w e against DFT_ComputeXCMetaSpin's Exc 1e-12.
* The eight gradient-side entries and the synchronous sweeps interleaved on one solver through shapes that grow and shrink
  the shared buffers: each result bitwise a fresh solver's; DFT_ComputeXC of a GGA solver bitwise the same before and after.
* The refusals, each with its sentence; of two faults in one call, the first in the order include/dft_solver.h states.
* nuclear_gradient_uks(meta=True) on HipBackend, H2O+ TPSS/def2-SVP, against the host assembly from the same matrices: 2e-8
  of max|g|; dense ERI, Cholesky vectors to 1e-10, grid_response=True, two_electron="device".
* The driver: --optimize with the new flags relaxes H2O+/STO-3G TPSS.

With QCDFT_WRITE_PROFILES set the figures are recorded as "gpu ..." lines of uks_meta_gradient_parity.txt in that directory.
"""
import ctypes
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import uks_meta_gradient_reference as um  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import functionals, gradients, inputs, metagga, scf  # noqa: E402

ERR_REL = 2e-8
_CSRC = os.path.join(os.path.dirname(q.__file__), "csrc")
_HEADERS = "".join(open(os.path.join(_CSRC, f)).read() if os.path.exists(os.path.join(_CSRC, f)) else ""
                   for f in ("xc_grad_launch.hpp", "xc_grad_meta_launch.hpp", "xc_grad_meta_spin_launch.hpp"))


def _cap(name):
    m = re.search(rf"constexpr int {name} = (\d+);", _HEADERS)
    return int(m.group(1)) if m else 0       # 0: a tree without the kernel -- test_the_entries_exist says so


CAP6, CAP2, CAP3 = _cap("XCGMS_KC_MAX"), _cap("XCG_KC_MAX"), _cap("XCGT_KC_MAX")
SHAPES = [(2085, 24, 5, 4), (2085, 114, 9, 7), (1100, 130, 9, 7), (37, 50, 6, 5), (2085, 50, 3, 0), (333, 50, 1, 1), (333, 50, 1, 0)]
# at the cap: one chunk; one column above: two, the second a single tile; three chunks, the last ragged (2 cap + 40 -> 48 padded)
CHUNK_SHAPES = [(37, n, 6, 5) for cap in (CAP6, CAP3, CAP2) for n in (cap, cap + 1, 2 * cap + 40)]


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


@functools.lru_cache(maxsize=None)
def _host_inputs(shape, shift=0.0):
    """(dm_a, dm_b, ao, ao_grad, w, ao_hess) of a shape; shift: dm_s - shift I."""
    dm_a, dm_b, ao, gr, w, hs = um.inputs(*shape)
    if shift:
        dm_a, dm_b = dm_a - shift * np.eye(shape[1]), dm_b - shift * np.eye(shape[1])
        dm_a.setflags(write=False); dm_b.setflags(write=False)
    return dm_a, dm_b, ao, gr, w, hs


class Planes:
    """The inputs of one shape on the device (copies: the cached host arrays are shared between tests)."""

    def __init__(self, dev, shape, shift=0.0):
        self.host = _host_inputs(shape, shift)
        self.ngrid, self.nao, self.dev = shape[0], shape[1], dev
        self.d_a, self.d_b, self.d_ao, self.d_gr, self.d_w, self.d_hs = (torch.as_tensor(np.array(a), device=dev) for a in self.host)
        self.d_dm = (self.d_a + self.d_b).contiguous()

    def _gradient(self, s, entry, dms, lo=0, hi=None):
        hi = self.ngrid if hi is None else hi
        d_out = torch.full((self.nao, 3), 7.0, dtype=torch.float64, device=self.dev)
        gr, hs = self.d_gr[:, lo:hi].contiguous(), self.d_hs[:, lo:hi].contiguous()
        assert getattr(s, entry)(hi - lo, self.nao, *dms, self.d_ao[lo:hi], self.d_w[lo:hi], d_out, gr, hs) == 0
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    def gradient(self, s, lo=0, hi=None):
        return self._gradient(s, "compute_xc_gradient_meta_spin", (self.d_a, self.d_b), lo, hi)

    def gradient_spin(self, s):
        return self._gradient(s, "compute_xc_gradient_spin", (self.d_a, self.d_b))

    def gradient_meta(self, s):
        return self._gradient(s, "compute_xc_gradient_meta", (self.d_dm,))

    def gradient_closed(self, s):
        return self._gradient(s, "compute_xc_gradient", (self.d_dm,))

    def _edens(self, s, entry, dms):
        d_e = torch.full((self.ngrid,), 7.0, dtype=torch.float64, device=self.dev)
        assert getattr(s, entry)(self.ngrid, self.nao, *dms, self.d_ao, d_e, self.d_gr) == 0
        torch.cuda.synchronize()
        return d_e.cpu().numpy()

    def edens(self, s):
        return self._edens(s, "compute_xc_energy_density_meta_spin", (self.d_a, self.d_b))

    def meta_spin(self, s):
        va, vb = (torch.full((self.nao, self.nao), 7.0, dtype=torch.float64, device=self.dev) for _ in range(2))
        exc = s.compute_xc_meta_spin(self.ngrid, self.nao, self.d_a, self.d_b, self.d_ao, self.d_w, va, vb, self.d_gr)
        torch.cuda.synchronize()
        return np.array([exc]), va.cpu().numpy(), vb.cpu().numpy()

    def meta(self, s):
        v = torch.full((self.nao, self.nao), 7.0, dtype=torch.float64, device=self.dev)
        exc = s.compute_xc_meta(self.ngrid, self.nao, self.d_dm, self.d_ao, self.d_w, v, self.d_gr)
        torch.cuda.synchronize()
        return np.array([exc]), v.cpu().numpy()

    def closed(self, s):
        v = torch.full((self.nao, self.nao), 7.0, dtype=torch.float64, device=self.dev)
        exc = s.compute_xc(self.ngrid, self.nao, self.d_dm, self.d_ao, self.d_w, v, self.d_gr)
        torch.cuda.synchronize()
        return np.array([exc]), v.cpu().numpy()


def _check(label, G, ref, bound=ERR_REL):
    scale = float(np.abs(ref).max())
    err = float(np.abs(G - ref).max())
    print(f"gpu {label}: max {scale:.3e}  err {err / scale:.2e}")
    um.record("gpu", label, None, err / scale)
    assert np.all(np.isfinite(G)) and scale > 0.0, label
    assert err <= bound * scale, (label, err / scale)


# ---- 0. what the code before this feature cannot do ---------------------------------------------------------------------
def test_the_entries_exist():
    lib = q.load_library(q.build_library())
    for name in ("DFT_ComputeXCGradientMetaSpin", "DFT_ComputeXCEnergyDensityMetaSpin"):
        assert hasattr(lib, name), name
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5
    s = _solver("TPSS")
    assert s.get_option("xcg_meta_spin_fused") in (0.0, 1.0)
    assert CAP6 > 0 and CAP6 % 16 == 0


# ---- a. device against host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("functional", um.FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES + CHUNK_SHAPES, ids=str)
def test_gradient_matches_the_host(dev, shape, functional, fused):
    p = Planes(dev, shape)
    G = p.gradient(_solver(functional, xcg_meta_spin_fused=fused))
    _check(f"DFT_ComputeXCGradientMetaSpin {functional} {shape} fused={fused}", G, um.host_gradient(functional, shape))


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("functional", um.FUNCTIONALS)
def test_validation_paths(dev, functional, path, fused):
    shape = (2085, 24, 5, 4)
    p = Planes(dev, shape)
    G = p.gradient(_solver(functional, xcg_meta_spin_fused=fused, path=path))
    _check(f"DFT_ComputeXCGradientMetaSpin {functional} {shape} fused={fused} path={path}", G, um.host_gradient(functional, shape))


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("shift", [0.15, 0.3])
@pytest.mark.parametrize("functional", um.FUNCTIONALS)
def test_indefinite_matrices_are_served(dev, functional, shift, fused):
    """dm_s - 0.15 I: negative densities in either channel (below the cut-off: that channel is absent), points where one
    channel lives and the other does not, z > 1 (clamped).  These planes have no live point with tau <= 0 at that shift;
    dm_s - 0.3 I has some in either channel, and points where both channels are absent."""
    shape = (2085, 24, 5, 4)
    dm_a, dm_b, ao, gr, w, hs = _host_inputs(shape, shift)
    ra, ga, ta, rb, gb, tb = metagga.density_spin_host(dm_a, dm_b, ao, gr)
    la, lb = ra > 1e-12, rb > 1e-12
    assert (la & ~lb).any() and (lb & ~la).any() and (la & lb).sum() > 500           # the inputs are what the case is about
    assert (np.einsum("gk,gk->g", ga, ga)[la & (ta > 0)] > (8.0 * ra * ta)[la & (ta > 0)]).any()
    assert ((ta[la] <= 0.0).any() and (tb[lb] <= 0.0).any() and (~la & ~lb).any()) == (shift == 0.3)
    p = Planes(dev, shape, shift)
    G = p.gradient(_solver(functional, xcg_meta_spin_fused=fused))
    _check(f"DFT_ComputeXCGradientMetaSpin {functional} {shape} dm_s - {shift} I fused={fused}", G, um.host_gradient(functional, shape, shift))


# ---- b. the two forms, reproducibility, slices --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2085, 114, 9, 7), (1100, 130, 9, 7), (37, 2 * CAP6 + 40, 6, 5)], ids=str)
def test_fused_against_plain_bitwise_repeats_and_slices(dev, shape):
    p = Planes(dev, shape)
    G = {}
    for fused in (0, 1):
        s = _solver("TPSSh", xcg_meta_spin_fused=fused)
        G[fused] = p.gradient(s)
        assert np.array_equal(G[fused], p.gradient(s)), fused
        cut = min(16 * 41 + 3, shape[0] - 5)      # not a multiple of the row tile: both slices end ragged
        two = p.gradient(s, 0, cut) + p.gradient(s, cut, shape[0])
        err = float(np.abs(two - G[fused]).max() / np.abs(G[fused]).max())
        print(f"gpu two slices against the whole grid {shape} fused={fused}: {err:.2e}")
        um.record("gpu", f"two slices against the whole grid TPSSh {shape} fused={fused}", None, err)
        assert err <= 1e-12
    err = float(np.abs(G[1] - G[0]).max() / np.abs(G[0]).max())
    print(f"gpu fused against plain {shape}: {err:.2e}")
    um.record("gpu", f"fused against plain TPSSh {shape}", None, err)
    assert err <= 1e-13


# ---- c. limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("functional", ["TPSS", "TPSSh"])
@pytest.mark.parametrize("shape", [(2085, 24, 5, 4), (2085, 114, 9, 7), (1100, 130, 9, 7)], ids=str)
def test_closed_shell_limit(dev, shape, functional, fused):
    p = Planes(dev, shape)
    half = (0.5 * p.d_dm).contiguous()
    G = p._gradient(_solver(functional, xcg_meta_spin_fused=fused), "compute_xc_gradient_meta_spin", (half, half))
    G0 = p.gradient_meta(_solver(functional))
    _check(f"(dm/2, dm/2) {functional} {shape} fused={fused} against DFT_ComputeXCGradientMeta(dm)", G, G0, 4e-14)


def _zero_meta_solver(mix):
    """A DFT_CreateSolverMeta solver with the mix's eight weights and zero meta weights."""
    f = functionals.resolve(mix)
    z = _solver(mix)
    lib = z.lib
    lib.DFT_CreateSolverMeta.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    lib.DFT_CreateSolverMeta.restype = ctypes.c_void_p
    h = lib.DFT_CreateSolverMeta((ctypes.c_double * 8)(*f.weight_vector()), 8, (ctypes.c_double * 2)(0.0, 0.0), 2)
    assert h
    lib.DFT_DestroySolver(ctypes.c_void_p(z.solver))
    z.solver = h
    z.set_option("quirks", 0)
    return z


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("mix", ["PBE0", "BLYP"])
@pytest.mark.parametrize("shape", [(2085, 24, 5, 4), (2085, 114, 9, 7), (1100, 130, 9, 7)], ids=str)
def test_zero_meta_weights_give_the_mix(dev, shape, mix, fused):
    """With both meta weights zero the contraction is DFT_ComputeXCGradientSpin's, honouring xcg_spin_fused."""
    p = Planes(dev, shape)
    z = _zero_meta_solver(mix)
    z.set_option("xcg_spin_fused", fused)
    G = p.gradient(z)
    G0 = p.gradient_spin(_solver(mix, xcg_spin_fused=fused))
    _check(f"zero meta weights {mix} {shape} xcg_spin_fused={fused} against DFT_ComputeXCGradientSpin", G, G0, 4e-14)
    z.set_option("xcg_meta_spin_fused", 1 - int(z.get_option("xcg_meta_spin_fused")))      # no tau term: the option has no say
    assert np.array_equal(G, p.gradient(z))


# ---- d. the energy density ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", um.FUNCTIONALS)
@pytest.mark.parametrize("shape", [(2085, 24, 5, 4), (2085, 114, 9, 7), (1100, 130, 9, 7), (2085, 50, 3, 0), (333, 50, 1, 1)], ids=str)
def test_energy_density(dev, shape, functional):
    p = Planes(dev, shape)
    s = _solver(functional)
    dm_a, dm_b, ao, gr, w, _ = p.host
    e = p.edens(s)
    _check(f"DFT_ComputeXCEnergyDensityMetaSpin {functional} {shape}", e, gradients.xc_energy_density_meta_spin_host(functional, dm_a, dm_b, ao, gr), 1e-12)
    exc = float(p.meta_spin(s)[0][0])
    err = abs(float(np.sum(w * e)) - exc) / abs(exc)
    print(f"gpu sum w e against DFT_ComputeXCMetaSpin's Exc {functional} {shape}: {err:.2e}")
    um.record("gpu", f"sum w e against DFT_ComputeXCMetaSpin's Exc {functional} {shape}", None, err, "Exc")
    assert err <= 1e-12


def test_energy_density_of_indefinite_matrices(dev):
    shape, shift = (2085, 24, 5, 4), 0.15
    p = Planes(dev, shape, shift)
    dm_a, dm_b, ao, gr, _, _ = p.host
    for functional in um.FUNCTIONALS:
        e = p.edens(_solver(functional))
        _check(f"DFT_ComputeXCEnergyDensityMetaSpin {functional} {shape} dm_s - {shift} I", e,
               gradients.xc_energy_density_meta_spin_host(functional, dm_a, dm_b, ao, gr), 1e-12)


# ---- e. nothing else is disturbed ---------------------------------------------------------------------------------------
def test_the_shared_gradient_set_carries_nothing_between_users(dev):
    """The eight gradient-side entries work in one set of buffers of the solver.  A DFT_CreateSolverMeta solver with zero meta
    weights (PBE0 at quirks = 0: the one kind that may call all eight) runs them and the two synchronous meta sweeps
    interleaved, in another order on every pass, over shapes that reserve the buffers small, grow them and come back; a TPSS
    solver runs its four entries and the two sweeps in the same way, in both settings of the fused options.  Each result is
    bitwise what the same call gives on a fresh solver that has run nothing else.  DFT_ComputeXC of a GGA solver is bitwise
    the same before and after."""
    def same(x, y):
        x, y = (a if isinstance(a, tuple) else (a,) for a in (x, y))
        return len(x) == len(y) and all(np.array_equal(a, b) and np.all(np.isfinite(a)) for a, b in zip(x, y))

    def calls(p):
        four = {"gradient_meta_spin": p.gradient, "edens_meta_spin": p.edens, "gradient_meta": p.gradient_meta,
                "edens_meta": lambda s: p._edens(s, "compute_xc_energy_density_meta", (p.d_dm,)),
                "meta_spin": p.meta_spin, "meta": p.meta}
        eight = dict(four, gradient=p.gradient_closed, gradient_spin=p.gradient_spin,
                     edens=lambda s: p._edens(s, "compute_xc_energy_density", (p.d_dm,)),
                     edens_spin=lambda s: p._edens(s, "compute_xc_energy_density_spin", (p.d_a, p.d_b)))
        return eight, four

    gga = _solver("GGA")
    p0 = Planes(dev, (2085, 114, 9, 7))
    before = p0.closed(gga)
    used = {"zero": _zero_meta_solver("PBE0"), "TPSS": _solver("TPSS")}
    fresh = {"zero": lambda: _zero_meta_solver("PBE0"), "TPSS": lambda: _solver("TPSS")}
    rng = np.random.default_rng(11)
    for shape in ((37, 50, 6, 5), (2085, 114, 9, 7), (1100, 130, 9, 7), (37, 50, 6, 5)):
        p = Planes(dev, shape)
        eight, four = calls(p)
        for fused in (1, 0):
            opts = dict(xcg_spin_fused=fused, xcg_meta_fused=fused, xcg_meta_spin_fused=fused)
            for kind, table in (("zero", eight), ("TPSS", four)):
                for name in rng.permutation(sorted(table)):
                    f = fresh[kind]()
                    for s in (used[kind], f):
                        for k, v in opts.items():
                            s.set_option(k, v)
                    assert same(table[name](used[kind]), table[name](f)), (shape, fused, kind, name)
    assert same(before, p0.closed(gga))


# ---- f. refusals --------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    p = Planes(dev, (37, 50, 6, 5))
    n, ng = p.nao, p.ngrid
    out, e = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev), torch.full((ng,), 7.0, dtype=torch.float64, device=dev)
    s = _solver("TPSS")
    grad = lambda s, ng=ng, n=n, a=p.d_a, b=p.d_b, ao=p.d_ao, w=p.d_w, gr=p.d_gr, hs=p.d_hs, out=out: \
        s.compute_xc_gradient_meta_spin(ng, n, a, b, ao, w, out, gr, hs)
    dens = lambda s, ng=ng, n=n, a=p.d_a, b=p.d_b, ao=p.d_ao, gr=p.d_gr, e=e: s.compute_xc_energy_density_meta_spin(ng, n, a, b, ao, e, gr)
    for entry, name in ((grad, "DFT_ComputeXCGradientMetaSpin"), (dens, "DFT_ComputeXCEnergyDensityMetaSpin")):
        with pytest.raises(RuntimeError, match=f"{name} needs a solver made by DFT_CreateSolverMeta"):
            entry(_solver("GGA"))
        for kw in ({"a": None}, {"b": None}, {"ao": None}, {"gr": None}):
            with pytest.raises(RuntimeError, match=f"{name} needs .*a pointer is null"):
                entry(s, **kw)
        for kw in ({"ng": 0}, {"n": 0}, {"ng": -3}):
            with pytest.raises(RuntimeError, match="bad sizes"):
                entry(s, **kw)
        for functional in ("tpss_x + pbe_c", "tpss_x + tpss_c + 0.1*vwn5_c"):
            with pytest.raises(RuntimeError, match="quirks = 1.*not the derivatives of their energies"):
                entry(_solver(functional, quirks=1))
        assert entry(_solver("tpss_x + pbe_c", quirks=0)) == 0
        assert entry(_solver("TPSS", quirks=1)) == 0          # TPSS itself runs at either setting
        # two faults in one call: the first in the order include/dft_solver.h states for the gradient-side entries
        with pytest.raises(RuntimeError, match=f"{name} needs a solver made by DFT_CreateSolverMeta"):     # the kind, a null pointer
            entry(_solver("GGA"), a=None)
        with pytest.raises(RuntimeError, match=f"{name} needs .*a pointer is null"):                       # a null pointer, the sizes
            entry(s, gr=None, ng=0)
        with pytest.raises(RuntimeError, match="bad sizes"):                                               # the sizes, quirks = 1
            entry(_solver("tpss_x + pbe_c", quirks=1), n=0)
    torch.cuda.synchronize()
    out.fill_(7.0)
    with pytest.raises(RuntimeError, match="quirks = 1.*not the derivatives of their energies"):           # quirks = 1, the LDS request
        grad(_solver("tpss_x + pbe_c", quirks=1), n=1700)
    for kw in ({"hs": None}, {"w": None}, {"out": None}):
        with pytest.raises(RuntimeError, match="DFT_ComputeXCGradientMetaSpin needs .*a pointer is null"):
            grad(s, **kw)
    with pytest.raises(RuntimeError, match="DFT_ComputeXCEnergyDensityMetaSpin needs .*a pointer is null"):
        dens(s, e=None)
    for fused in (0, 1):                                        # refused before any launch: the planes are never read
        s.set_option("xcg_meta_spin_fused", fused)
        with pytest.raises(RuntimeError, match="DFT_ComputeXCGradientMetaSpin: nao=1700 needs .*bytes of LDS per workgroup"):
            grad(s, n=1700)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                             # nothing was launched by any refusal
    assert grad(s) == 0                                         # ... and the solver stays usable
    torch.cuda.synchronize()
    assert s.last_error() == ""


# ---- g. end to end ------------------------------------------------------------------------------------------------------
UKS_BACKEND = dict(quirks=False, device_resident=False, fused_tail=False, eigensolver="exact")


@pytest.fixture(scope="module")
def cation():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    dense = inputs.build("H2O", "def2-svp", 1, verbose=False, charge=1, spin=1)
    be = scf.HipBackend(dense, "TPSS", **UKS_BACKEND)
    res = scf.run_uks(dense, be, "TPSS", log=None, conv_e=1e-10, meta=True)
    assert res["converged"]
    return dense, be, res


@functools.lru_cache(maxsize=None)
def _host_assembly(dm_a_bytes, dm_b_bytes, grid_response):
    from uks_meta_host_backend import UksMetaHostBackend
    dense = inputs.build("H2O", "def2-svp", 1, verbose=False, charge=1, spin=1)
    dms = {k: np.frombuffer(b).reshape(dense.shells.nao, -1) for k, b in (("dm_a", dm_a_bytes), ("dm_b", dm_b_bytes))}
    state = dict(dms, nalpha=dense.nalpha, nbeta=dense.nbeta)
    return gradients.nuclear_gradient_uks(dense, state, UksMetaHostBackend(dense, "TPSS"), "TPSS", grid_response=grid_response, meta=True)


def _bytes(res):
    return tuple(np.ascontiguousarray(res[k]).tobytes() for k in ("dm_a", "dm_b"))


@pytest.mark.parametrize("case", ["dense", "grid_response", "grad2e_device"])
def test_nuclear_gradient_on_the_device(cation, case):
    dense, be, res = cation
    grid = case == "grid_response"
    g, terms = gradients.nuclear_gradient_uks(dense, res, be, grid_response=grid, two_electron="device" if case == "grad2e_device" else "host", meta=True)
    ref, ref_terms = _host_assembly(*_bytes(res), grid)
    scale = float(np.abs(ref).max())
    for k in ref_terms:
        print(f"gpu nuclear_gradient_uks(meta=True) H2O+/def2-SVP TPSS {case} {k}: {np.abs(terms[k] - ref_terms[k]).max() / scale:.2e}")
    assert float(np.abs(terms["xc"]).max()) > 1e-3               # TPSS's eight weights are zero: the meta weights count
    _check(f"nuclear_gradient_uks(meta=True) H2O+/def2-SVP TPSS {case}", g, ref)
    net = float(np.abs(g.sum(axis=0)).max())
    print(f"gpu nuclear_gradient_uks(meta=True) H2O+/def2-SVP TPSS {case}: net force {net:.2e}")
    um.record("gpu", f"nuclear_gradient_uks(meta=True) H2O+/def2-SVP TPSS {case}: net force, Ha/bohr", None, net, "1")
    assert (net <= 1e-10) if grid else (net < 1e-3)


def test_nuclear_gradient_on_cholesky_vectors():
    """Cholesky vectors to 1e-10, so that their share of W stays below the bound."""
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=1e-10, charge=1, spin=1)
    be = scf.HipBackend(inp, "TPSS", **UKS_BACKEND)
    res = scf.run_uks(inp, be, "TPSS", log=None, conv_e=1e-10, meta=True)
    assert res["converged"]
    g, _ = gradients.nuclear_gradient_uks(inp, res, be, meta=True)
    ref, _ = _host_assembly(*_bytes(res), False)
    _check("nuclear_gradient_uks(meta=True) H2O+/def2-SVP TPSS cholesky", g, ref)


def test_backend_methods_and_refusals(cation):
    dense, be, res = cation
    dm_a, dm_b = (np.ascontiguousarray(res[k]) for k in ("dm_a", "dm_b"))
    G = be.xc_gradient_meta_spin(dm_a, dm_b)
    assert np.array_equal(G, be.xc_gradient_meta_spin(dm_a, dm_b)) and G.shape == (dense.shells.nao, 3)
    G3 = be.xc_gradient_meta_spin(dm_a, dm_b, slice_rows=3000)
    assert np.abs(G3 - G).max() <= 1e-12 * np.abs(G).max()
    for f in (lambda: be.xc_gradient_spin(dm_a, dm_b), lambda: be.xc_grid_response_spin(dm_a, dm_b),
              lambda: gradients.nuclear_gradient_uks(dense, res, be)):
        with pytest.raises(ValueError, match="meta-GGA.*not built"):
            f()
    with pytest.raises(ValueError, match="meta=True.*--open-shell-meta-gradient"):
        gradients.nuclear_gradient_uks(dense, res, be)
    pbe = scf.HipBackend(dense, "PBE0", **UKS_BACKEND)
    for name in ("xc_gradient_meta_spin", "xc_grid_response_meta_spin"):
        with pytest.raises(ValueError, match="is not one"):
            getattr(pbe, name)(dm_a, dm_b)
    with pytest.raises(ValueError, match="is not one"):
        gradients.nuclear_gradient_uks(dense, res, pbe, meta=True)


def test_driver_relaxes_the_cation_with_the_flags(tmp_path):
    """--optimize with --spin 1 --charge 1 --open-shell-meta --open-shell-gradient --open-shell-meta-gradient --grid-response
    --grad2e device, TPSS H2O+/STO-3G at grid level 1: every step honours the flags (run_uks(meta=True) included)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "run.json"
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "TPSS", "H2O", "--basis", "sto-3g", "--grid-level", "1", "--spin", "1",
           "--charge", "1", "--open-shell-meta", "--open-shell-gradient", "--open-shell-meta-gradient", "--optimize", "--grid-response",
           "--grad2e", "device", "--json", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(out.read_text().splitlines()[-1])
    assert rec["grid_response"] is True and rec["grad2e_engine"] == "device" and rec["uks"] and rec["nalpha"] == 5 and rec["nbeta"] == 4
    assert set(rec["gradient_terms"]) == {"one_electron", "two_electron", "xc", "nuclear", "external", "xc_grid"}
    assert np.abs(np.asarray(rec["gradient_terms"]["xc"])).max() > 1e-3
    assert rec["opt_converged"] and 1 <= rec["opt_steps"] <= 30
    assert rec["opt_energies"][-1] < rec["opt_energies"][0] - 1e-5
    assert np.abs(rec["net_force"]).max() < 1e-9
    assert (tmp_path / "H2O_opt.xyz").exists()
