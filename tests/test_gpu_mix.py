"""Mix solvers (DFT_CreateSolverMix, k_xc_points_mix) on a real MI355X against the numpy composition of the oracle's
own pieces (tests/mix_reference.py).  Tolerances are the project's (test_gpu_parity.py): Exc |rel| <= 1e-12,
Vxc |abs| <= 1e-11 max|V| + 1e-13.

Inputs: helpers.synth_inputs(ngrid, nao, seed=ngrid + nao) with the first seven grid rows of ao and of the three
gradient planes scaled so that those points sit at rho = 1e-14, below the density cut-off.  A point ON a cut-off could
legitimately differ between device and oracle, so every case first asserts, on the oracle's own rho and sigma, that no
point has rho in [0.5e-12, 2e-12] or sigma in [0.5e-20, 8e-20] (8e-20 covers B88's sigma/4)."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402  (the checker)
import quantum_compute_dft_amd as q  # noqa: E402
from helpers import synth_inputs  # noqa: E402
from mix_reference import MixBackend, compute_xc_mix, density  # noqa: E402
from quantum_compute_dft_amd import basis, inputs, scf  # noqa: E402
from quantum_compute_dft_amd.functionals import COMPONENTS, TABLE  # noqa: E402

# the three kernel families (wave-specialised nao <= 128, large-basis above) and nao <= 32, where the tiny path must be bypassed
SHAPES = [(2000, 24), (3000, 57), (4096, 114), (1500, 150), (1200, 246)]
NCUT = 7
MIX_NAMES = [k for k, f in TABLE.items() if f.builtin_type is None]
SINGLE = {name: [1.0 if j == k else 0.0 for j in range(len(COMPONENTS))] for k, name in enumerate(COMPONENTS)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _below_cutoff(dm, ao, gr, nrows=NCUT):
    rho = np.einsum("gi,ij,gj->g", ao[:nrows], dm, ao[:nrows])
    sc = np.sqrt(1e-14 / rho)
    ao[:nrows] *= sc[:, None]
    gr[:, :nrows] *= sc[None, :, None]


def _assert_clear_of_the_cutoffs(dm, ao, gr, w, ncut):
    rho, _, sigma = density(dm, ao, w, gr, True)
    assert int(np.sum(rho < 1e-12)) == ncut
    assert not np.any((rho >= 0.5e-12) & (rho <= 2e-12))
    assert not np.any((sigma >= 0.5e-20) & (sigma <= 8e-20))


@functools.lru_cache(maxsize=None)
def _case(ngrid, nao):
    dm, ao, gr, w = synth_inputs(ngrid, nao, seed=ngrid + nao)
    _below_cutoff(dm, ao, gr)
    _assert_clear_of_the_cutoffs(dm, ao, gr, w, NCUT)
    return dm, ao, gr, w


@functools.lru_cache(maxsize=2)
def _device_case(ngrid, nao):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    return tuple(t(a) for a in _case(ngrid, nao))


def _solver(spec, **opts):
    """spec: a table name / expression, or eight weights (then straight through DFT_CreateSolverMix)."""
    if isinstance(spec, str):
        s = q.DFTSolverWrapper(q.build_library(), spec)
    else:
        from quantum_compute_dft_amd.functionals import Functional
        s = q.DFTSolverWrapper(q.build_library(), Functional("weights", {c: v for c, v in zip(COMPONENTS, spec) if v}, 0.0, None))
    for k, v in opts.items():
        s.set_option(k, v)
    return s


def _run(s, d_dm, d_ao, d_gr, d_w):
    ngrid, nao = d_ao.shape
    d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=d_ao.device)   # must be overwritten
    exc = s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
    torch.cuda.synchronize()
    return exc, d_v.cpu().numpy()


def _check(exc, v, exc_ref, v_ref, what=""):
    scale = np.abs(v_ref).max()
    print(f"{what}: Exc {exc:.15e} ref {exc_ref:.15e} rel {abs(exc - exc_ref) / max(abs(exc_ref), 1e-300):.2e}; "
          f"max|dV| {np.abs(v - v_ref).max():.2e} of max|V| {scale:.3e}")
    assert exc == pytest.approx(exc_ref, rel=1e-12, abs=1e-14)
    assert np.abs(v - v_ref).max() <= 1e-11 * scale + 1e-13


def _weights_of(spec):
    return SINGLE[spec] if spec in SINGLE else TABLE[spec].weight_vector()


@pytest.mark.parametrize("ngrid,nao", SHAPES)
@pytest.mark.parametrize("spec", list(COMPONENTS) + MIX_NAMES)
def test_mix_sweep_matches_the_composition(dev, spec, ngrid, nao):
    """Each component alone (unit weight) and every table entry that is not a built-in type."""
    dm, ao, gr, w = _case(ngrid, nao)
    wv = _weights_of(spec)
    gga = any(wv[4:])
    exc_ref, v_ref = compute_xc_mix(wv, dm, ao, w, gr)
    d_dm, d_ao, d_gr, d_w = _device_case(ngrid, nao)
    s = _solver(wv if spec in SINGLE else spec, profile=1)
    assert s.mix() == wv and s.needs_gradient == gga
    exc, v = _run(s, d_dm, d_ao, d_gr if gga else None, d_w)
    names = [n for n, _ in s.timings()]
    assert "xc_points" in names and "sweep_tiny" not in names        # nao <= 32 too: a mix never takes the one-pass kernel
    _check(exc, v, exc_ref, v_ref, f"{spec} ({ngrid}, {nao})")


@pytest.mark.parametrize("quirks", [1, 0])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_quirks_option_and_validation_paths(dev, quirks, path):
    """Option "quirks" reaches vwn5_c and pbe_c of a mix; options path = 1 / 2 share the pointwise kernel."""
    ngrid, nao = 3000, 57
    dm, ao, gr, w = _case(ngrid, nao)
    wv = [0.3, 0.7, 0.0, 0.2, 0.5, 0.9, 0.4, -0.3]
    exc_ref, v_ref = compute_xc_mix(wv, dm, ao, w, gr, quirks=bool(quirks))
    exc, v = _run(_solver(wv, quirks=quirks, path=path), *_device_case(ngrid, nao))
    _check(exc, v, exc_ref, v_ref, f"all-but-one components, quirks {quirks}, path {path}")


@pytest.mark.parametrize("ngrid,nao", SHAPES)
@pytest.mark.parametrize("name", ["LDA", "GGA", "B3LYP"])
def test_builtin_weights_as_a_mix_match_the_builtin_solver(dev, name, ngrid, nao):
    """DFT_GetMix(built-in) fed to DFT_CreateSolverMix against the built-in solver on the device: LDA and GGA directly,
    B3LYP after (V + V^T)/2 (its library output is symmetric already).  Another summation order, so not bit-equal."""
    d_dm, d_ao, d_gr, d_w = _device_case(ngrid, nao)
    builtin = _solver(name)
    grad = d_gr if name != "LDA" else None
    exc_ref, v_ref = _run(builtin, d_dm, d_ao, grad, d_w)
    mix = _solver(builtin.mix())
    assert mix.functional.builtin_type is None and mix.needs_gradient == (name != "LDA")
    exc, v = _run(mix, d_dm, d_ao, grad, d_w)
    if name == "B3LYP":
        assert np.array_equal(v_ref, v_ref.T)
        v = 0.5 * (v + v.T)
    _check(exc, v, exc_ref, v_ref, f"{name} as a mix ({ngrid}, {nao})")


def test_negative_definite_density_gives_zero(dev):
    ngrid, nao = 3000, 57
    dm, ao, gr, w = synth_inputs(ngrid, nao, seed=ngrid + nao)
    dm = -dm
    rho, _, _ = density(dm, ao, w, gr, True)
    assert np.all(rho < 0.0)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    for spec in ("PBE0", "BLYP", "PW92"):
        s = _solver(spec)
        exc, v = _run(s, t(dm), t(ao), t(gr) if s.needs_gradient else None, t(w))
        assert exc == 0.0 and not v.any()


def test_gradient_pointer_rules(dev):
    ngrid, nao = 2000, 24
    dm, ao, gr, w = _case(ngrid, nao)
    d_dm, d_ao, d_gr, d_w = _device_case(ngrid, nao)
    lda_class = _solver("slater + 0.5*pw92 + 0.5*vwn_rpa")
    exc_ref, v_ref = compute_xc_mix(lda_class.weights, dm, ao, w, None)
    _check(*_run(lda_class, d_dm, d_ao, None, d_w), exc_ref, v_ref, "LDA-class mix, ao_grad = None")
    _check(*_run(lda_class, d_dm, d_ao, d_gr, d_w), exc_ref, v_ref, "LDA-class mix, ao_grad given and ignored")
    gga_class = _solver("PBE0")
    d_v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError):
        gga_class.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, None)
    assert "ao_grad" in gga_class.last_error()
    import ctypes
    u = ctypes.c_uint64
    r = gga_class.lib.DFT_ComputeXC(gga_class.solver, ngrid, nao, u(d_dm.data_ptr()), u(d_ao.data_ptr()), u(0), u(d_w.data_ptr()), u(d_v.data_ptr()))
    assert np.isnan(r) and gga_class.lib.DFT_GetLastError(gga_class.solver)


def _occ_case(ngrid, nao, nocc):
    """test_gpu_occ.occ_inputs' recipe, seven rows below the cut-off."""
    rng = np.random.default_rng(ngrid + nao + nocc)
    ao = 0.4 * rng.standard_normal((ngrid, nao))
    gr = 0.3 * rng.standard_normal((3, ngrid, nao))
    w = 0.05 * rng.random(ngrid)
    cocc = np.sqrt(2.0) * 0.7 * rng.standard_normal((nao, nocc))
    dm = cocc @ cocc.T
    _below_cutoff(dm, ao, gr)
    _assert_clear_of_the_cutoffs(dm, ao, gr, w, NCUT)
    return cocc, dm, ao, gr, w


@pytest.mark.parametrize("ngrid,nao,nocc", [(4096, 114, 21), (1200, 246, 47)])
@pytest.mark.parametrize("spec", ["PBE0", "B3LYP5", "PW92"])
def test_occupied_orbital_async_and_replayed_calls(dev, spec, ngrid, nao, nocc):
    """DFT_ComputeXCOcc agrees with DFT_ComputeXC of the same mix solver (and both with the composition); the async
    entries and graph-replayed repeats are bit-identical to the first call."""
    cocc, dm, ao, gr, w = _occ_case(ngrid, nao, nocc)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    d_c, d_dm, d_ao, d_w = t(cocc), t(dm), t(ao), t(w)
    s = _solver(spec, graph=0)
    d_gr = t(gr) if s.needs_gradient else None
    exc_ref, v_ref = compute_xc_mix(s.weights, dm, ao, w, gr)
    exc0, v0 = _run(s, d_dm, d_ao, d_gr, d_w)
    _check(exc0, v0, exc_ref, v_ref, f"{spec} dm ({ngrid}, {nao})")
    d_v = torch.full((nao, nao), 7.0, dtype=torch.float64, device=dev)
    d_e = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    for occ in (0, 1):                                   # auto (what the SCF loop gets) and the occupied form forced
        s.set_option("occ", occ)
        d_v.fill_(7.0)
        exc1 = s.compute_xc_occ(ngrid, nao, nocc, d_c, d_ao, d_w, d_v, d_gr, d_dm)
        torch.cuda.synchronize()
        v1 = d_v.cpu().numpy()
        _check(exc1, v1, exc0, v0, f"{spec} occ={occ} against the dm call")
        _check(exc1, v1, exc_ref, v_ref, f"{spec} occ={occ} against the composition")
        d_v.fill_(7.0)
        assert s.compute_xc_occ_async(ngrid, nao, nocc, d_c, d_ao, d_w, d_v, d_e, d_gr, d_dm) == 0
        torch.cuda.synchronize()
        assert float(d_e.item()) == exc1 and np.array_equal(d_v.cpu().numpy(), v1)
    s.set_option("occ", 0)
    d_v.fill_(7.0)
    assert s.compute_xc_async(ngrid, nao, d_dm, d_ao, d_w, d_v, d_e, d_gr) == 0
    torch.cuda.synchronize()
    assert float(d_e.item()) == exc0 and np.array_equal(d_v.cpu().numpy(), v0)
    s.set_option("graph", 1)                             # plain, recorded, replayed, replayed
    for rep in range(4):
        d_v.fill_(7.0)
        e = s.compute_xc(ngrid, nao, d_dm, d_ao, d_w, d_v, d_gr)
        assert e == exc0 and np.array_equal(d_v.cpu().numpy(), v0), rep
    s.set_option("occ", 1)
    for rep in range(4):
        d_v.fill_(7.0)
        e = s.compute_xc_occ(ngrid, nao, nocc, d_c, d_ao, d_w, d_v, d_gr, d_dm)
        assert e == exc1 and np.array_equal(d_v.cpu().numpy(), v1), rep


@pytest.mark.parametrize("molecule,ngrid,nao,nocc", [("Benzene", 4096, 114, 21), ("Anthracene", 1200, 246, 47)])
@pytest.mark.parametrize("spec", ["PBE0", "PW92"])
def test_direct_sweep_with_a_mix_solver(dev, spec, molecule, ngrid, nao, nocc):
    """DFT_ComputeXCDirect (AO planes re-evaluated chunk by chunk) against DFT_ComputeXC of the same mix solver on the
    AO kernel's resident planes: real def2-SVP shells, grid points scattered around the atoms."""
    syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, molecule + ".xyz"))
    sh = basis.build_shells(syms, xyz, "def2-svp")
    assert sh.nao == nao
    rng = np.random.default_rng(ngrid + nao)
    centres = np.asarray(sh.xyz).reshape(-1, 3)
    coords = centres[rng.integers(0, len(centres), ngrid)] + rng.normal(0.0, 0.8, (ngrid, 3))
    wts = 0.02 * rng.random(ngrid)
    C = 0.3 * rng.standard_normal((nao, nocc)); dm = 2.0 * C @ C.T
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    d_c, d_w, d_dm = t(coords), t(wts), t(dm)
    s = _solver(spec)
    d_ao = torch.zeros((ngrid, nao), dtype=torch.float64, device=dev)
    d_gr = torch.zeros((3, ngrid, nao), dtype=torch.float64, device=dev)
    s.eval_ao(sh, d_c, ngrid, d_ao, d_gr)
    exc0, v0 = _run(s, d_dm, d_ao, d_gr if s.needs_gradient else None, d_w)
    ao, gr = d_ao.cpu().numpy(), d_gr.cpu().numpy()
    rho, _, sigma = density(dm, ao, wts, gr, True)
    assert not np.any((rho >= 0.5e-12) & (rho <= 2e-12)) and not np.any((sigma >= 0.5e-20) & (sigma <= 8e-20))
    exc_ref, v_ref = compute_xc_mix(s.weights, dm, ao, wts, gr)
    _check(exc0, v0, exc_ref, v_ref, f"{spec} resident planes, {molecule}")
    d_v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
    d_e = torch.zeros(1, dtype=torch.float64, device=dev)
    for chunk in (1024, 1000, 0):
        d_v.fill_(7.0); d_e.fill_(7.0)
        s.compute_xc_direct(sh, ngrid, d_c, d_w, d_dm, d_v, d_e, chunk)
        torch.cuda.synchronize()
        _check(float(d_e.item()), d_v.cpu().numpy(), exc0, v0, f"{spec} direct, chunk {chunk}, {molecule}")


@pytest.mark.parametrize("fn,bname", [("PBE0", "sto-3g"), ("BLYP", "sto-3g"), ("PBE0", "def2-svp")])
def test_full_scf_matches_the_composition_driven_scf(dev, fn, bname):
    """test_gpu_parity.test_full_scf_matches_the_oracle_driven_scf's recipe with a mixed functional: the whole device
    path (AO kernel, J/K, mix sweep, exact-exchange fraction) against the same loop on the composition backend."""
    inp = inputs.build("H2O", bname, 3, verbose=False)
    kw = dict(log=None, conv_e=1e-11, conv_dm=1e-9)
    r_gpu = scf.run_scf(inp, scf.HipBackend(inp, fn), fn, **kw)
    r_cpu = scf.run_scf(inp, MixBackend(inp, fn), fn, **kw)
    print(f"{fn}/{bname}: E_tot gpu {r_gpu['E_tot']:.12f} cpu {r_cpu['E_tot']:.12f}; E_xc {r_gpu['E_xc']:.12f} / {r_cpu['E_xc']:.12f}; "
          f"E_ex_hf {r_gpu['E_ex_hf']:.12f} / {r_cpu['E_ex_hf']:.12f}; cycles {r_gpu['cycles']} / {r_cpu['cycles']}; "
          f"max|ddm| {np.abs(r_gpu['dm'] - r_cpu['dm']).max():.2e}")
    assert r_gpu["converged"] and r_cpu["converged"]
    assert r_gpu["E_tot"] == pytest.approx(r_cpu["E_tot"], abs=1e-9)
    assert r_gpu["E_xc"] == pytest.approx(r_cpu["E_xc"], abs=1e-9)
    assert np.abs(r_gpu["dm"] - r_cpu["dm"]).max() < 1e-7
    assert (r_gpu["E_ex_hf"] != 0.0) == (TABLE[fn].c_hf != 0.0)


def test_fused_loop_matches_the_host_loop_for_pbe0_on_benzene(dev):
    """Benzene/def2-SVP, factorised J/K, PBE0: the loop with its host part on the device (DFT_ScfTailStep carries c_hf)
    against the host loop on the same backend class.  Both stop at |dE| < 1e-8 (dft.py:243), hence 2e-8 between the
    final energies, as test_gpu_scf_tail.test_fused_loop_matches_the_host_loop argues.  The per-cycle gap is printed,
    not asserted: that test's CYCLE_GAP numbers were measured per functional and none exists for PBE0."""
    inp = inputs.build("Benzene", "def2-svp", 3, device=dev, verbose=False, eri_mode="cholesky", chol_tol=1e-8)
    host = scf.HipBackend(inp, "PBE0", device=dev, device_resident=False)
    assert host.tail is None and host.solver.c_hf == 0.25
    r_host = scf.run_scf(inp, host, "PBE0", log=None)
    fused = scf.HipBackend(inp, "PBE0", device=dev)
    assert fused.tail is not None
    r_fused = scf.run_scf(inp, fused, "PBE0", log=None)
    gaps = [abs(a[0] - b[0]) for a, b in zip(r_host["per_cycle"], r_fused["per_cycle"])]
    print(f"Benzene PBE0/def2-SVP: E_tot host {r_host['E_tot']:.10f} fused {r_fused['E_tot']:.10f}; cycles {r_host['cycles']} / "
          f"{r_fused['cycles']}; E_ex_hf {r_host['E_ex_hf']:.8f} / {r_fused['E_ex_hf']:.8f}; largest per-cycle gap {max(gaps):.2e} Ha; "
          f"median XC {r_fused['xc_ms']:.4f} ms, iteration {r_fused['iter_ms']:.4f} ms")
    assert r_host["converged"] and r_fused["converged"] and r_fused["loop"] == "fused"
    assert abs(r_host["cycles"] - r_fused["cycles"]) <= 1
    assert abs(r_host["E_tot"] - r_fused["E_tot"]) <= 2e-8, (r_host["E_tot"], r_fused["E_tot"])
    assert r_fused["E_ex_hf"] < -1.0 and r_host["E_ex_hf"] < -1.0
