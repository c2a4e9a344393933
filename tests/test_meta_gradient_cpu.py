"""The nuclear gradient of a meta-GGA on the host: gradients.xc_gradient_meta_host against finite differences of
metagga.xc_meta_host's Exc (tests/meta_gradient_reference.py), the assembled gradient (nuclear_gradient(meta=True) on
meta_reference.MetaHostBackend) against finite differences of the converged energy, the refusals, the optimiser.

Whole gradient: tests/test_gradient_scf_cpu.py's method and directions -- H2O/STO-3G with both bonds 0.15 bohr shorter, grid
level 1, conv_e = conv_dm = 1e-11, h = 2e-4 and 2 h, one Richardson level, the z of O, the y of one H and one random unit
vector -- once with the grid of the undisplaced geometry in every displaced run (the fixed-quadrature derivative) and once
with grid_response=True against runs whose grid is rebuilt at every displaced geometry.  Bound per direction
max(10 bar, 1e-9 scale); the cap on the reference's own bar is 10 bar <= 1e-5 scale here, not 1e-6: the O-z direction at the
fixed grid has a bar of 4.9e-7 of the scale with TPSS (the energy's noise under h = 2e-4 next to the h^2 term of a functional
with a z-clamp and tau in it), and a missing tau term is a 1e-3 effect, so the cap still cannot hide one.

With QCDFT_WRITE_PROFILES set the figures are recorded as "cpu ..." lines of meta_gradient_parity.txt in that directory.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import meta_gradient_reference as mg
import spin_reference as sr
import test_gradient_scf_cpu as gs
import quantum_compute_dft_amd as q
from meta_reference import MetaHostBackend
from quantum_compute_dft_amd import functionals, gradients, inputs, optimize, scf

SHAPES = [(333, 24), (333, 114)]


# ---- a. the XC force on synthetic planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("functional", mg.FUNCTIONALS)
def test_host_gradient_against_finite_differences(functional, shape):
    cols, ref, bar = mg.reference(functional, *shape)
    G = mg.host_gradient(functional, *shape)
    assert G.shape == (shape[1], 3)
    mg.check_fd("cpu", f"xc_gradient_meta_host {functional} {shape}", G[list(cols)], ref, bar)
    # the same call without the tau term misses the bound (so that the test cannot pass without it): a 1e-3 effect
    dm, ao, gr, w, hs = mg.inputs(*shape)
    G0 = gradients.xc_gradient_meta_host(functional, dm, ao, w, gr, hs, tau_term=False)[list(cols)]
    scale = float(np.abs(ref).max())
    miss = float(np.abs(G0 - ref).max())
    print(f"cpu xc_gradient_meta_host {functional} {shape} without the tau term: miss {miss / scale:.2e}")
    assert miss > 100.0 * max(10.0 * bar, 1e-9 * scale) and miss > 1e-4 * scale


@pytest.mark.parametrize("mix", ["PBE0", "BLYP", "slater_x + pw92_c"])
def test_zero_meta_weights_give_the_mix(mix):
    dm, ao, gr, w, hs = mg.inputs(333, 24)
    G = gradients.xc_gradient_meta_host(mix, dm, ao, w, gr, hs)
    G0 = gradients.xc_gradient_host(mix, dm, ao, w, gr, hs, quirks=False)
    err = float(np.abs(G - G0).max() / np.abs(G0).max())
    print(f"cpu xc_gradient_meta_host {mix} against xc_gradient_host at quirks 0: {err:.2e}")
    mg.record("cpu", f"zero meta weights {mix} (333, 24) against xc_gradient_host", None, err)
    assert err <= sr.CLOSED_SHELL_BAR
    e = gradients.xc_energy_density_meta_host(mix, dm, ao, gr)
    e0 = gradients.xc_energy_density_host(mix, dm, ao, gr, quirks=False)
    assert np.abs(e - e0).max() <= sr.CLOSED_SHELL_BAR * np.abs(e0).max()


def test_only_the_symmetric_part_of_dm_counts():
    dm, ao, gr, w, hs = mg.inputs(333, 24)
    a = np.random.default_rng(11).standard_normal(dm.shape)
    G = gradients.xc_gradient_meta_host("TPSS", dm + (a - a.T), ao, w, gr, hs)
    assert np.abs(G - mg.host_gradient("TPSS", 333, 24)).max() <= 1e-12 * np.abs(G).max()
    e = gradients.xc_energy_density_meta_host("TPSS", dm + (a - a.T), ao, gr)
    assert np.abs(e - gradients.xc_energy_density_meta_host("TPSS", dm, ao, gr)).max() <= 1e-12 * np.abs(e).max()


def test_energy_density_sums_to_exc():
    from quantum_compute_dft_amd import metagga
    dm, ao, gr, w, _ = mg.inputs(333, 114)
    for functional in mg.FUNCTIONALS:
        e = gradients.xc_energy_density_meta_host(functional, dm, ao, gr)
        exc = metagga.xc_meta_host(functional, dm, ao, w, gr)[0]
        assert abs(float(np.sum(w * e)) - exc) <= 1e-13 * abs(exc)
    with pytest.raises(ValueError, match="needed for a meta-GGA"):
        gradients.xc_gradient_meta_host("TPSS", dm, ao, w, gr, None)
    with pytest.raises(ValueError, match="needed for a meta-GGA"):
        gradients.xc_energy_density_meta_host("TPSS", dm, ao, None)


# ---- b. the whole gradient ------------------------------------------------------------------------------------------------
def _run(base, functional, xyz, fixed_grid):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz)
    if fixed_grid:
        inp = dataclasses.replace(inp, grids=base.grids)
    be = MetaHostBackend(inp, functional)
    res = scf.run_scf(inp, be, functional, **gs.KW)
    assert res["converged"]
    return inp, be, res


@pytest.mark.parametrize("grid", ["fixed", "rebuilt"])
@pytest.mark.parametrize("functional", ["TPSS", "TPSSh"])
def test_whole_gradient_sto3g(functional, grid):
    fixed = grid == "fixed"
    H = gs.H
    base = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=gs._stretched("sto-3g", -0.15))
    inp, be, res = _run(base, functional, base.atom_xyz, fixed)
    g, terms = gradients.nuclear_gradient(inp, res, be, functional, grid_response=not fixed, meta=True)
    assert set(terms) == {"one_electron", "two_electron", "xc", "nuclear", "external"} | (set() if fixed else {"xc_grid"})
    assert np.allclose(sum(terms.values()), g, rtol=0, atol=1e-14)
    assert np.abs(terms["xc"]).max() > 1e-2          # TPSS's eight GGA weights are all zero: the meta weights count
    directions = [gs._unit(3, 0, 2), gs._unit(3, 1, 1), gs._random(3)]
    refs = []
    for d in directions:
        E = {t: _run(base, functional, base.atom_xyz + t * d, fixed)[2]["E_tot"] for t in (H, -H, 2 * H, -2 * H)}
        D1, D2 = (E[H] - E[-H]) / (2 * H), (E[2 * H] - E[-2 * H]) / (4 * H)
        ref = (4.0 * D1 - D2) / 3.0
        refs.append((ref, abs(ref - D1)))
    scale = max(abs(r) for r, _ in refs[:-1])
    label = f"nuclear_gradient(meta=True) H2O/sto-3g {functional} grid {grid}"
    for k, (d, (ref, bar)) in enumerate(zip(directions, refs)):
        an = float(np.sum(g * d))
        print(f"cpu {label} direction {k}: analytic {an:+.10e}  D_R {ref:+.10e}  bar {bar / scale:.2e}  err {abs(an - ref) / scale:.2e}")
        mg.record("cpu", f"{label} direction {k}", bar / scale, abs(an - ref) / scale, "max|g|")
    for k, (d, (ref, bar)) in enumerate(zip(directions, refs)):
        an = float(np.sum(g * d))
        assert 10.0 * bar <= 1e-5 * scale, (label, k, bar / scale)
        assert abs(an - ref) <= max(10.0 * bar, 1e-9 * scale), (label, k, abs(an - ref) / scale, bar / scale)
    net = float(np.abs(g.sum(axis=0)).max())
    print(f"cpu {label}: max|g| {np.abs(g).max():.3e}  net force {net:.2e}")
    if fixed:
        assert net > 1e-6                              # grid level 1: the fixed quadrature's share is there to be removed
    else:
        assert net <= 1e-12


# ---- c. refusals ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def water():
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    be = MetaHostBackend(inp, "TPSS")
    res = scf.run_scf(inp, be, "TPSS", log=None)
    assert res["converged"]
    return inp, be, res


def test_the_keyword_is_needed_and_named(water):
    inp, be, res = water
    with pytest.raises(ValueError) as e:
        gradients.nuclear_gradient(inp, res, be, "TPSS")
    msg = str(e.value)
    assert "meta-GGA" in msg and "not built" in msg and "meta=True" in msg and "--meta-gradient" in msg
    with pytest.raises(ValueError, match="is not one"):
        gradients.nuclear_gradient(inp, res, be, "PBE0", quirks=False, meta=True)
    uks = {"dm_a": 0.5 * res["dm"], "dm_b": 0.5 * res["dm"]}
    with pytest.raises(ValueError, match="meta-GGA.*not built"):
        gradients.nuclear_gradient_uks(inp, uks, be, "TPSS")
    with pytest.raises(ValueError, match="meta-GGA.*not built"):
        gradients.xc_grid_response_host("TPSS", res["dm"], inp.shells, inp.grids, inp.symbols, inp.atom_xyz)
    # the keyword changes nothing for anybody else
    assert "meta" in gradients.nuclear_gradient.__code__.co_varnames
    assert gradients.nuclear_gradient.__defaults__[-1] is False


@pytest.mark.parametrize("flags", [["--gradient"], ["--optimize"], ["--gradient", "--grid-response"]])
def test_driver_names_the_flag(flags, capsys):
    from quantum_compute_dft_amd import dft
    with pytest.raises(SystemExit) as e:
        dft.main(["TPSS", "H2O", "--basis", "sto-3g"] + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "meta-GGA" in err and flags[0] in err and "not built" in err and "--meta-gradient" in err


@pytest.mark.parametrize("argv,text", [(["PBE0", "H2O", "--gradient", "--meta-gradient", "--quirks", "0"], "--meta-gradient is for a meta-GGA"),
                                       (["TPSS", "H2O", "--gradient", "--meta-gradient", "--spin", "2", "--open-shell-meta"], "closed-shell gradient of a meta-GGA"),
                                       (["TPSS", "H2O", "--meta-gradient"], "--meta-gradient goes with --gradient or --optimize"),
                                       (["TPSS", "H2O", "--polarizability", "--gradient", "--meta-gradient"], "--polarizability")])
def test_driver_refuses_the_flag_where_it_does_not_belong(argv, text, capsys):
    from quantum_compute_dft_amd import dft
    with pytest.raises(SystemExit) as e:
        dft.main(argv + ["--basis", "sto-3g"])
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_library_refusals_without_a_device():
    lib = q.load_library(q.build_library())
    dp, u64 = ctypes.POINTER(ctypes.c_double), ctypes.c_uint64
    for name in ("DFT_ComputeXCGradientMeta", "DFT_ComputeXCEnergyDensityMeta"):
        assert hasattr(lib, name), name
    lib.DFT_CreateSolverMeta.argtypes, lib.DFT_CreateSolverMeta.restype = [dp, ctypes.c_int, dp, ctypes.c_int], ctypes.c_void_p
    lib.DFT_CreateSolverMix.argtypes, lib.DFT_CreateSolverMix.restype = [dp, ctypes.c_int], ctypes.c_void_p
    lib.DFT_GetLastError.argtypes, lib.DFT_GetLastError.restype = [ctypes.c_void_p], ctypes.c_char_p
    lib.DFT_DestroySolver.argtypes = [ctypes.c_void_p]
    lib.DFT_SetOption.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]
    lib.DFT_GetOption.argtypes, lib.DFT_GetOption.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_double
    lib.DFT_ComputeXCGradientMeta.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [u64] * 6
    lib.DFT_ComputeXCEnergyDensityMeta.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [u64] * 4
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5
    arr = lambda v: (ctypes.c_double * len(v))(*v)
    zero8 = [0.0] * 8
    s = lib.DFT_CreateSolverMeta(arr(zero8), 8, arr([1.0, 1.0]), 2)
    k = lib.DFT_CreateSolverMeta(arr([0, 0, 0, 0, 0, 1.0, 0, 0]), 8, arr([1.0, 0.0]), 2)      # tpss_x + pbe_c, quirks = 1 by default
    g = lib.DFT_CreateSolverMix(arr([0, 0, 0, 0, 1.0, 1.0, 0, 0]), 8)
    assert s and k and g
    P = 8                      # a non-null address: every refusal below comes before anything is read
    try:
        def grad(h, ng=10, n=4, ptrs=(P,) * 6):
            rc = lib.DFT_ComputeXCGradientMeta(h, ng, n, *ptrs)
            return rc, lib.DFT_GetLastError(h).decode()

        def dens(h, ng=10, n=4, ptrs=(P,) * 4):
            rc = lib.DFT_ComputeXCEnergyDensityMeta(h, ng, n, *ptrs)
            return rc, lib.DFT_GetLastError(h).decode()

        for entry, name, nptr in ((grad, "DFT_ComputeXCGradientMeta", 6), (dens, "DFT_ComputeXCEnergyDensityMeta", 4)):
            rc, msg = entry(g)
            assert rc == -1 and name in msg and "DFT_CreateSolverMeta" in msg and "no meta-GGA weights" in msg
            for i in range(nptr):              # every pointer, ao_grad and ao_hess included
                rc, msg = entry(s, ptrs=tuple(0 if j == i else P for j in range(nptr)))
                assert rc == -1 and name in msg and "a pointer is null" in msg, i
            for kw in ({"ng": 0}, {"n": 0}, {"ng": -1}):
                rc, msg = entry(s, **kw)
                assert rc == -1 and "bad sizes" in msg
            rc, msg = entry(k)
            assert rc == -1 and "quirks = 1" in msg and "not the derivatives of their energies" in msg
        for fused, nao in ((1.0, 1217), (0.0, 1329)):     # the first basis past each form's 160 KB
            assert lib.DFT_SetOption(s, b"xcg_meta_fused", fused) == 0 and lib.DFT_GetOption(s, b"xcg_meta_fused") == fused
            rc, msg = grad(s, n=nao)
            assert rc == -1 and "bytes of LDS per workgroup" in msg and f"nao={nao}" in msg
    finally:
        for h in (s, k, g):
            lib.DFT_DestroySolver(h)


# ---- d. the optimiser -----------------------------------------------------------------------------------------------------
def test_optimiser_relaxes_a_stretched_bond():
    """H2O/STO-3G TPSS from the shipped geometry with one O-H bond stretched by 0.2 bohr, grid level 1, the grid response on:
    converged at the customary thresholds, lower in energy than the start, the net force at rounding level all the way."""
    base = inputs.build("H2O", "sto-3g", 1, verbose=False)
    xyz0 = base.atom_xyz.copy()
    bond = xyz0[1] - xyz0[0]
    xyz0[1] += 0.2 * bond / np.linalg.norm(bond)
    nets = []

    def fun(xyz):
        inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz)
        be = MetaHostBackend(inp, "TPSS")
        res = scf.run_scf(inp, be, "TPSS", log=None, conv_e=1e-10, conv_dm=1e-8)
        assert res["converged"]
        g = gradients.nuclear_gradient(inp, res, be, "TPSS", grid_response=True, meta=True)[0]
        nets.append(float(np.abs(g.sum(axis=0)).max()))
        return res["E_tot"], g

    out = optimize.bfgs(fun, xyz0, max_steps=30)
    print(f"cpu optimiser TPSS, grid level 1, grid response on: {out['steps']} steps, {out['evaluations']} evaluations, "
          f"E {out['energies'][0]:.8f} -> {out['energy']:.8f}, max|g| {np.abs(out['gradient']).max():.2e}, largest net force on the way {max(nets):.2e}")
    assert out["converged"] and out["steps"] <= 30
    assert out["energy"] < out["energies"][0] - 1e-4
    assert optimize.converged(out["gradient"]) and np.abs(out["gradient"]).max() < 3e-4
    assert max(nets) <= 1e-10
    r1, r2 = (np.linalg.norm(out["xyz"][k] - out["xyz"][0]) for k in (1, 2))
    assert abs(r1 - r2) < 5e-3
