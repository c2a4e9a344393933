"""The grid response of the nuclear gradient on the device (csrc/becke.hip, scf.HipBackend.xc_grid_response) against its host
counterparts, which tests/test_grid_response_cpu.py holds against autograd and against moving-grid differences.

* DFT_BeckeWeightGradient against grid_gen.becke_weight_gradient_host at 2e-8 of the largest component, all finite, the same
  call twice bitwise equal, the rows summing to zero; the returned cell against grid_gen.becke_weights at 1e-12.  Shapes
  (ngrid, natm): (2085, 2) and (2085, 3); (1100, 13); one natm just above each tile boundary of the kernel -- (600, 61) the
  first with 32 points per tile, (400, 121) the first with 16, (200, 241) the first with 8 -- and (300, 128); every ngrid
  leaves a ragged last tile, every case holds a point on its own and one on a foreign nucleus; and the real H2O level-1 grid
  with its exact-zero cells.
* DFT_ComputeXCEnergyDensity / ...Spin against the host at 2e-8 of max|e|, and sum_g w_g e_g against the Exc of
  DFT_ComputeXC / DFT_ComputeXCSpin (1e-12 of sum_g |w_g e_g|: the same products summed in another order), on (2085, 24),
  (2085, 114), (1100, 130) and the fully polarised (2085, 50) with three alpha and no beta electrons; LDA, GGA, B3LYP, PBE0.
* A DFT_ComputeXC before and after the new calls is bitwise equal; the refusals.
* The driver: --gradient with and without --grid-response (header, JSON fields, the flag off as before), and --optimize
  --grid-response on the unrestricted state with the two-electron term on the device, at grid level 1.
* nuclear_gradient(..., grid_response=True) on HipBackend (H2O/def2-SVP B3LYP) and nuclear_gradient_uks (H2O+) against the host
  assembly from the same dm at 2e-8 of max|g|; the per-block sum of G against xc_gradient of the whole grid at 1e-13 of max|G|.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spin_reference as sr  # noqa: E402
import xc_gradient_reference as xr  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import basis, gradients, grid_gen, inputs, scf  # noqa: E402
from test_grid_response_cpu import record  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_REL = 2e-8
FUNCTIONALS = ["LDA", "GGA", "B3LYP", "PBE0"]
ELEMENTS = ["H", "C", "N", "O", "P", "S"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(functional="LDA", quirks=1):
    s = q.DFTSolverWrapper(q.build_library(), functional)
    s.set_option("quirks", quirks)
    return s


def synthetic(ngrid, natm, seed=7):
    """(coords, owner, atom_xyz, charges, f): atoms on a jittered lattice 2.2 bohr apart (none closer than 1.4), points at
    log-uniform distances 0.02 .. 8 bohr from their owners, the first on its own nucleus, the second on a foreign one."""
    rng = np.random.default_rng(seed + natm)
    side = int(np.ceil(natm ** (1.0 / 3.0)))
    cells = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)
    xyz = 2.2 * cells[rng.permutation(len(cells))[:natm]] + rng.uniform(-0.4, 0.4, (natm, 3))
    sym = [str(s) for s in rng.choice(ELEMENTS, natm)]
    if natm >= 2:
        sym[0], sym[1] = "H", "O"
    own = rng.integers(0, natm, ngrid)
    d = rng.standard_normal((ngrid, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    coords = xyz[own] + d * np.exp(rng.uniform(np.log(0.02), np.log(8.0), ngrid))[:, None]
    coords[0] = xyz[own[0]]
    if natm >= 2:
        coords[1] = xyz[(own[1] + 1) % natm]
    return coords, own, xyz, [basis.atomic_number(s) for s in sym], rng.standard_normal(ngrid)


def device_weight_gradient(s, dev, coords, own, xyz, z, f, cell=True):
    d_c, d_f = torch.as_tensor(np.ascontiguousarray(coords), device=dev), torch.as_tensor(np.ascontiguousarray(f), device=dev)
    d_o = torch.as_tensor(np.asarray(own).astype(np.int32), device=dev)
    d_out = torch.full((len(z), 3), 7.0, dtype=torch.float64, device=dev)
    d_cell = torch.full((len(own),), 7.0, dtype=torch.float64, device=dev) if cell else None
    assert s.becke_weight_gradient(len(own), xyz, grid_gen.bragg_radii_bohr(z), d_c, d_o, d_f, d_out, d_cell) == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), (d_cell.cpu().numpy() if cell else None)


def _weight_check(label, s, dev, coords, own, xyz, z, f):
    got, cell = device_weight_gradient(s, dev, coords, own, xyz, z, f)
    again, _ = device_weight_gradient(s, dev, coords, own, xyz, z, f, cell=False)
    ref = grid_gen.becke_weight_gradient_host(coords, own, xyz, z, f)
    ref_cell = grid_gen.becke_weights(coords, own, xyz, z)
    scale = float(np.abs(ref).max())
    err, cerr = float(np.abs(got - ref).max()) / scale, float(np.abs(cell - ref_cell).max())
    print(f"gpu DFT_BeckeWeightGradient {label}: max|out| {scale:.3e}  err {err:.2e}  cell err {cerr:.2e}  rows sum {np.abs(got.sum(axis=0)).max():.1e}"
          f"  exact-zero cells {int((cell == 0).sum())}")
    record(f"gpu  DFT_BeckeWeightGradient device / host, {label}", None, err, "max|out|")
    record(f"gpu  DFT_BeckeWeightGradient cell against becke_weights, {label}", None, cerr, "1")
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(cell)), label
    assert np.array_equal(got, again), label
    assert err <= ERR_REL, (label, err)
    assert cerr <= 1e-12, (label, cerr)
    assert np.abs(got.sum(axis=0)).max() <= 1e-12 * scale * np.sqrt(len(own)), label


@pytest.mark.parametrize("shape", [(2085, 2), (2085, 3), (1100, 13), (600, 61), (400, 121), (300, 128), (200, 241)])
def test_weight_gradient_matches_the_host(dev, shape):
    _weight_check(str(shape), _solver(), dev, *synthetic(*shape))


def test_weight_gradient_on_the_water_grid(dev):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    g = inp.grids
    z = [basis.atomic_number(s) for s in inp.symbols]
    assert (grid_gen.becke_weights(g.coords, g.atom_index, inp.atom_xyz, z) == 0).sum() > 0      # the trap is in the case
    f = g.atomic_weights * np.random.default_rng(5).standard_normal(g.size)
    _weight_check("H2O level-1 grid", _solver(), dev, g.coords, g.atom_index, inp.atom_xyz, z, f)


def test_weight_gradient_one_atom_and_new_atoms_on_one_solver(dev):
    """One atom: zeros and cell = 1.  A second call with other atoms on the same solver uploads its own tables."""
    s = _solver()
    co, own, xyz, z, f = synthetic(333, 1)
    got, cell = device_weight_gradient(s, dev, co, own, xyz, z, f)
    assert np.all(got == 0.0) and np.all(cell == 1.0)
    for seed in (1, 2):
        co, own, xyz, z, f = synthetic(333, 5, seed)
        got, _ = device_weight_gradient(s, dev, co, own, xyz, z, f)
        ref = grid_gen.becke_weight_gradient_host(co, own, xyz, z, f)
        assert np.abs(got - ref).max() <= ERR_REL * np.abs(ref).max()


def test_weight_gradient_refusals(dev):
    s = _solver()
    co, own, xyz, z, f = synthetic(64, 3)
    d_c, d_f, d_o = torch.as_tensor(co, device=dev), torch.as_tensor(f, device=dev), torch.as_tensor(own.astype(np.int32), device=dev)
    d_out = torch.zeros((3, 3), dtype=torch.float64, device=dev)
    rad = grid_gen.bragg_radii_bohr(z)
    with pytest.raises(RuntimeError, match="needs the atom positions"):
        s.becke_weight_gradient(64, xyz, rad, d_c, None, d_f, d_out)
    with pytest.raises(RuntimeError, match="coincide"):
        s.becke_weight_gradient(64, xyz[[0, 1, 1]], rad, d_c, d_o, d_f, d_out)
    with pytest.raises(RuntimeError, match="not positive"):
        s.becke_weight_gradient(64, xyz, rad * np.array([1.0, 0.0, 1.0]), d_c, d_o, d_f, d_out)
    with pytest.raises(RuntimeError, match="bad sizes"):
        s.becke_weight_gradient(0, xyz, rad, d_c, d_o, d_f, d_out)
    with pytest.raises(ValueError, match="radii"):
        s.becke_weight_gradient(64, xyz, rad[:2], d_c, d_o, d_f, d_out)
    many = 1006                                                            # the first natm whose 8-point tile no longer fits 160 KB
    big = np.arange(3 * many, dtype=np.float64).reshape(many, 3)
    with pytest.raises(RuntimeError, match="bytes of LDS"):
        s.becke_weight_gradient(64, big, np.ones(many), d_c, d_o, d_f, torch.zeros((many, 3), dtype=torch.float64, device=dev))


# ---- the energy density --------------------------------------------------------------------------------------------------
class Planes:
    def __init__(self, dev, ngrid, nao, na=None, nb=None):
        self.dm, self.ao, self.gr, self.w, _ = xr.inputs(ngrid, nao)
        self.ngrid, self.nao, self.dev = ngrid, nao, dev
        self.d_dm, self.d_ao, self.d_gr, self.d_w = (torch.as_tensor(np.array(a), device=dev) for a in (self.dm, self.ao, self.gr, self.w))
        if na is not None:
            self.dm_a, self.dm_b = sr.spin_inputs(ngrid, nao, na, nb)[:2]
            self.d_a, self.d_b = (torch.as_tensor(np.array(a), device=dev) for a in (self.dm_a, self.dm_b))


def _edens_check(label, e, ref, w, exc):
    scale = float(np.abs(ref).max())
    err = float(np.abs(e - ref).max()) / scale
    total, mass = float(w @ e), float(np.abs(w * e).sum())
    print(f"gpu {label}: max|e| {scale:.3e}  err {err:.2e}  sum w e {total:.12f}  Exc {exc:.12f}  ({abs(total - exc) / mass:.1e} of sum |w e|)")
    record(f"gpu  {label} device / host", None, err, "max|e|")
    record(f"gpu  {label} sum w e against Exc", None, abs(total - exc) / mass, "sum|w e|")
    assert np.all(np.isfinite(e)), label
    assert err <= ERR_REL, (label, err)
    assert abs(total - exc) <= 1e-12 * mass, (label, total, exc)


@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("shape", [(2085, 24), (2085, 114), (1100, 130)])
@pytest.mark.parametrize("quirks", [1, 0])
def test_energy_density_matches_the_host(dev, shape, functional, quirks):
    p = Planes(dev, *shape)
    s = _solver(functional, quirks)
    n = p.nao
    gr = p.d_gr if s.needs_gradient else None
    d_v = torch.zeros((n, n), dtype=torch.float64, device=dev)
    s.compute_xc(p.ngrid, n, p.d_dm, p.d_ao, p.d_w, d_v, gr)
    exc0, v0 = s.compute_xc(p.ngrid, n, p.d_dm, p.d_ao, p.d_w, d_v, gr), d_v.cpu().numpy()      # the second call is the one a graph would be recorded from
    d_e = torch.full((p.ngrid,), 7.0, dtype=torch.float64, device=dev)
    assert s.compute_xc_energy_density(p.ngrid, n, p.d_dm, p.d_ao, d_e, gr) == 0
    torch.cuda.synchronize()
    e = d_e.cpu().numpy()
    ref = gradients.xc_energy_density_host(functional, p.dm, p.ao, p.gr if s.needs_gradient else None, bool(quirks))
    _edens_check(f"DFT_ComputeXCEnergyDensity {functional} quirks={quirks} {shape}", e, ref, p.w, exc0)
    exc1 = s.compute_xc(p.ngrid, n, p.d_dm, p.d_ao, p.d_w, d_v, gr)
    assert exc1 == exc0 and np.array_equal(d_v.cpu().numpy(), v0)                                 # the sweep is left as it was


@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("shape", [(2085, 24, 5, 4), (2085, 114, 21, 19), (1100, 130, 12, 9), (2085, 50, 3, 0)])
def test_spin_energy_density_matches_the_host(dev, shape, functional):
    p = Planes(dev, *shape)
    if shape[3] == 0:
        assert not np.any(p.dm_b)
    s = _solver(functional, 0)
    n = p.nao
    gr = p.d_gr if s.needs_gradient else None
    d_va, d_vb = (torch.zeros((n, n), dtype=torch.float64, device=dev) for _ in range(2))
    exc0 = s.compute_xc_spin(p.ngrid, n, p.d_a, p.d_b, p.d_ao, p.d_w, d_va, d_vb, gr)
    va0, vb0 = d_va.cpu().numpy(), d_vb.cpu().numpy()
    d_e = torch.full((p.ngrid,), 7.0, dtype=torch.float64, device=dev)
    assert s.compute_xc_energy_density_spin(p.ngrid, n, p.d_a, p.d_b, p.d_ao, d_e, gr) == 0
    torch.cuda.synchronize()
    e = d_e.cpu().numpy()
    ref = gradients.xc_energy_density_spin_host(functional, p.dm_a, p.dm_b, p.ao, p.gr if s.needs_gradient else None)
    _edens_check(f"DFT_ComputeXCEnergyDensitySpin {functional} {shape}", e, ref, p.w, exc0)
    assert s.compute_xc_spin(p.ngrid, n, p.d_a, p.d_b, p.d_ao, p.d_w, d_va, d_vb, gr) == exc0
    assert np.array_equal(d_va.cpu().numpy(), va0) and np.array_equal(d_vb.cpu().numpy(), vb0)


def test_the_sweep_is_left_as_it_was_by_all_three_calls(dev):
    """DFT_ComputeXC (B3LYP, a shape whose calls are replayed as a recorded graph) before and after the three new entries."""
    p = Planes(dev, 2085, 24, 5, 4)
    s = _solver("B3LYP")
    n = p.nao
    d_v = torch.zeros((n, n), dtype=torch.float64, device=dev)

    def sweep():
        e = s.compute_xc(p.ngrid, n, p.d_dm, p.d_ao, p.d_w, d_v, p.d_gr)
        return e, d_v.cpu().numpy()

    sweep(); sweep(); e0, v0 = sweep()
    d_e = torch.zeros(p.ngrid, dtype=torch.float64, device=dev)
    assert s.compute_xc_energy_density(p.ngrid, n, p.d_dm, p.d_ao, d_e, p.d_gr) == 0
    assert s.compute_xc_energy_density_spin(p.ngrid, n, p.d_a, p.d_b, p.d_ao, d_e, p.d_gr) == 0
    co, own, xyz, z, f = synthetic(p.ngrid, 13)
    device_weight_gradient(s, dev, co, own, xyz, z, f)
    e1, v1 = sweep()
    assert e0 == e1 and np.array_equal(v0, v1)


def test_energy_density_refusals(dev):
    p = Planes(dev, 37, 50, 6, 5)
    d_e = torch.zeros(37, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="null for a gradient-corrected functional"):
        _solver("GGA").compute_xc_energy_density(37, 50, p.d_dm, p.d_ao, d_e, None)
    with pytest.raises(RuntimeError, match="needs dm"):
        _solver("LDA").compute_xc_energy_density(37, 50, None, p.d_ao, d_e, None)
    for functional in ("LDA", "GGA", "PBE0"):          # vwn5_c, pbe_c, pbe_c in a mix: DFT_ComputeXCSpin's refusal
        with pytest.raises(RuntimeError, match="--quirks 0"):
            _solver(functional, 1).compute_xc_energy_density_spin(37, 50, p.d_a, p.d_b, p.d_ao, d_e, p.d_gr)
    assert _solver("B3LYP", 1).compute_xc_energy_density_spin(37, 50, p.d_a, p.d_b, p.d_ao, d_e, p.d_gr) == 0
    with pytest.raises(RuntimeError, match="needs both density matrices"):
        _solver("LDA", 0).compute_xc_energy_density_spin(37, 50, p.d_a, None, p.d_ao, d_e, None)
    torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def _check(label, g, ref):
    scale = float(np.abs(ref).max())
    err = float(np.abs(g - ref).max()) / scale
    print(f"gpu {label}: max {scale:.3e}  err {err:.2e}")
    record(f"gpu  {label} device / host", None, err, "max|g|")
    assert np.all(np.isfinite(g)), label
    assert err <= ERR_REL, (label, err)


@pytest.mark.parametrize("functional,quirks", [("B3LYP", True), ("LDA", False)])
def test_nuclear_gradient_with_the_grid_response_on_the_device(functional, quirks):
    """B3LYP: resident planes; LDA: the backend keeps no gradient planes and evaluates them per slice."""
    from scf_oracle_backend import OracleBackend
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    be = scf.HipBackend(inp, functional, quirks=quirks)
    res = scf.run_scf(inp, be, functional, log=None, conv_e=1e-10)
    assert res["converged"]
    g0, t0 = gradients.nuclear_gradient(inp, res, be)
    g, terms = gradients.nuclear_gradient(inp, res, be, grid_response=True)
    assert all(np.array_equal(t0[k], terms[k]) for k in t0) and set(terms) == set(t0) | {"xc_grid"}      # xc_gradient keeps its bits
    ref, ref_terms = gradients.nuclear_gradient(inp, {"dm": res["dm"]}, OracleBackend(inp, functional, quirks=quirks), functional, quirks=quirks,
                                                grid_response=True)
    scale = float(np.abs(ref).max())
    print(f"gpu nuclear_gradient grid_response H2O/def2-SVP {functional} xc_grid: {np.abs(terms['xc_grid'] - ref_terms['xc_grid']).max() / scale:.2e} of max|g|,"
          f" net force {np.abs(g.sum(axis=0)).max():.2e} (fixed grid {np.abs(g0.sum(axis=0)).max():.2e})")
    _check(f"nuclear_gradient grid_response=True H2O/def2-SVP {functional}", g, ref)
    assert np.abs(terms["xc_grid"] - ref_terms["xc_grid"]).max() <= ERR_REL * scale
    assert np.abs(g.sum(axis=0)).max() <= ERR_REL * scale          # translational invariance, to the bound of the device terms
    # the blocks in slices: the same term to the rounding of the slice sums
    sliced = be.xc_grid_response(np.asarray(res["dm"]), slice_rows=1000)
    assert np.abs(sliced - terms["xc_grid"]).max() <= 1e-12 * scale
    be.close()


def test_uks_gradient_with_the_grid_response_on_the_device():
    from uks_host_backend import UksHostBackend
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False, charge=1, spin=1)
    be = scf.HipBackend(inp, "B3LYP", device_resident=False, fused_tail=False, eigensolver="exact")
    res = scf.run_uks(inp, be, "B3LYP", log=None, conv_e=1e-10)
    assert res["converged"]
    g0, t0 = gradients.nuclear_gradient_uks(inp, res, be)
    g, terms = gradients.nuclear_gradient_uks(inp, res, be, grid_response=True)
    assert all(np.array_equal(t0[k], terms[k]) for k in t0) and set(terms) == set(t0) | {"xc_grid"}
    state = {k: res[k] for k in ("dm_a", "dm_b", "nalpha", "nbeta")}
    ref, ref_terms = gradients.nuclear_gradient_uks(inp, state, UksHostBackend(inp, "B3LYP"), "B3LYP", grid_response=True)
    scale = float(np.abs(ref).max())
    _check("nuclear_gradient_uks grid_response=True H2O+/def2-SVP B3LYP", g, ref)
    assert np.abs(terms["xc_grid"] - ref_terms["xc_grid"]).max() <= ERR_REL * scale
    assert np.abs(g.sum(axis=0)).max() <= ERR_REL * scale
    be.close()


def test_the_blocks_add_up_to_the_whole_grid():
    """sum over the atom blocks of G (what xc_grid_response subtracts) against xc_gradient of the whole grid: 1e-13 of max|G|,
    the bound of the slice test of tests/test_gpu_xc_gradient.py."""
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    be = scf.HipBackend(inp, "B3LYP")
    res = scf.run_scf(inp, be, "B3LYP", log=None, conv_e=1e-10)
    dm = np.ascontiguousarray(res["dm"])
    G = be.xc_gradient(dm)
    d_dm = be._dev(dm)
    entry = lambda m, ao, w, out, gr, hs: be.solver.compute_xc_gradient(m, be.nao, d_dm, ao, w, out, gr, hs)      # noqa: E731
    own = inp.grids.atom_index
    cut = np.flatnonzero(np.diff(own)) + 1
    assert len(cut) == 2
    blocks = sum(be._xc_gradient_slices(None, entry, block=(int(lo), int(hi))) for lo, hi in zip([0, *cut], [*cut, len(own)]))
    err = float(np.abs(blocks - G).max() / np.abs(G).max())
    print(f"gpu per-block sum of G against the whole grid H2O/def2-SVP B3LYP: {err:.2e}")
    record("gpu  per-block sum of G against xc_gradient of the whole grid", None, err, "max|G|")
    assert err <= 1e-13
    assert np.array_equal(G, be.xc_gradient(dm))          # and the whole-grid call keeps its bits
    be.close()


def test_backend_refusals():
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    dm = np.eye(inp.shells.nao)
    be = scf.HipBackend(inp, "LDA", xc_occ=False, dm_factor=True, quirks=False)
    with pytest.raises(ValueError, match="without dm_factor"):
        be.xc_grid_response(dm)
    be = scf.HipBackend(inp, "B3LYP", device_resident=True)          # a closed-shell tail: what xc_gradient_spin refuses
    with pytest.raises(ValueError, match="open-shell DFT"):
        be.xc_grid_response_spin(dm, dm)
    be = scf.HipBackend(inp, "B3LYP", device_resident=False, fused_tail=False)
    be.world = 2
    with pytest.raises(ValueError, match="one rank"):
        be.xc_grid_response(dm)
    with pytest.raises(ValueError, match="one rank"):
        be.xc_grid_response_spin(dm, dm)
    import dataclasses
    import types
    g = inp.grids
    bare = types.SimpleNamespace(coords=g.coords, weights=g.weights, size=g.size)
    be = scf.HipBackend(dataclasses.replace(inp, grids=bare), "B3LYP")
    with pytest.raises(ValueError, match="atom_index and atomic_weights"):
        be.xc_grid_response(dm)
    bad = types.SimpleNamespace(coords=g.coords, weights=g.weights, size=g.size, atom_index=g.atom_index + 1, atomic_weights=g.atomic_weights)
    be = scf.HipBackend(dataclasses.replace(inp, grids=bad), "B3LYP")
    with pytest.raises(ValueError, match="do not match"):
        be.xc_grid_response(dm)


def _driver(tmp_path, *argv):
    out = tmp_path / "run.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", *argv, "--json", str(out)]
    r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(out.read_text().splitlines()[-1]), r.stdout


def test_driver_gradient_with_and_without_the_flag(tmp_path):
    """B3LYP H2O/def2-SVP at grid level 1: the flag adds xc_grid, the header and grid_response, and takes the net force to
    rounding; without it the record has the fields it had."""
    base = ["B3LYP", "H2O", "--basis", "def2-svp", "--grid-level", "1", "--gradient"]
    off, text_off = _driver(tmp_path, *base)
    on, text_on = _driver(tmp_path, *base, "--grid-response")
    assert "grid_response" not in off and set(off["gradient_terms"]) == {"one_electron", "two_electron", "xc", "nuclear", "external"}
    assert "at fixed quadrature points and weights" in text_off and "includes the grid" not in text_off
    assert on["grid_response"] is True and set(on["gradient_terms"]) == set(off["gradient_terms"]) | {"xc_grid"}
    assert "the derivative includes the grid" in text_on and "at fixed quadrature points and weights" not in text_on
    print(f"gpu driver --gradient H2O/def2-SVP B3LYP grid level 1: net force {np.abs(off['net_force']).max():.2e} -> {np.abs(on['net_force']).max():.2e}")
    assert np.abs(off["net_force"]).max() > 1e-6 and np.abs(on["net_force"]).max() < 1e-9
    g_on, g_off = np.asarray(on["gradient"]), np.asarray(off["gradient"])
    assert np.abs(g_on - g_off - np.asarray(on["gradient_terms"]["xc_grid"])).max() < 1e-9          # two SCF runs: the other terms to convergence


def test_driver_relaxes_the_cation_at_grid_level_1(tmp_path):
    """--optimize --grid-response --spin 1 --charge 1 --open-shell-gradient --grad2e device: every step honours the flag."""
    rec, text = _driver(tmp_path, "LDA", "H2O", "--quirks", "0", "--grid-level", "1", "--spin", "1", "--charge", "1", "--optimize",
                        "--open-shell-gradient", "--grad2e", "device", "--grid-response")
    assert rec["uks"] is True and rec["grid_response"] is True and rec["grad2e_engine"] == "device"
    assert rec["opt_converged"] and 1 <= rec["opt_steps"] <= 30
    assert rec["opt_energies"][-1] < rec["opt_energies"][0] - 1e-5
    assert "xc_grid" in rec["gradient_terms"] and np.abs(rec["net_force"]).max() < 1e-9
    last = [l for l in text.splitlines() if l.strip().startswith("sum")][-1]          # the table of the last step's gradient
    assert max(abs(float(x)) for x in last.split()[1:4]) < 1e-9
    assert (tmp_path / "H2O_opt.xyz").exists()
