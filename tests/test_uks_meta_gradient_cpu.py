"""The nuclear gradient of an open-shell meta-GGA on the host: gradients.xc_gradient_meta_spin_host against finite differences
of metagga.xc_meta_spin_host's Exc (tests/uks_meta_gradient_reference.py), its limits, the assembled gradient
(nuclear_gradient_uks(meta=True) on UksMetaHostBackend) against finite differences of the converged run_uks(meta=True) energy,
the refusals of the assembly, the driver and the library, and the optimiser.

Whole gradient: tests/test_uks_gradient_cpu.py's protocol -- H2O/STO-3G with both bonds 0.15 bohr shorter, grid level 1,
conv_e = conv_dm = 1e-11, h = 2e-4 and 2 h, one Richardson level, the z of O, the y of one H and one random unit vector, the
displaced runs on the undisplaced grid; one case with grid_response=True against runs whose grid is rebuilt.  Bound per
direction max(10 bar, 1e-9 scale); the cap on the reference's own bar is 10 bar <= 1e-5 scale, the closed-shell meta test's cap
and reason (tests/test_meta_gradient_cpu.py): the O-z direction's bar was measured at 1.3e-7 .. 1.5e-7 of the scale for these
states, above the 1e-6 / 10 of the GGA tests, and a missing tau term is a 1e-3 effect, so the cap still cannot hide one.

With QCDFT_WRITE_PROFILES set the figures are recorded as "cpu ..." lines of uks_meta_gradient_parity.txt in that directory.
"""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import spin_reference as sr
import test_uks_gradient_cpu as ug
import uks_meta_gradient_reference as um
import quantum_compute_dft_amd as q
from meta_reference import MetaHostBackend
from uks_host_backend import UksHostBackend
from uks_meta_host_backend import UksMetaHostBackend
from quantum_compute_dft_amd import functionals, gradients, inputs, metagga, optimize, scf

FD_CASES = [(f, s) for s in [(333, 24, 5, 4), (333, 114, 9, 7), (333, 24, 3, 0)] for f in um.FUNCTIONALS] + \
           [(f, (333, 24, 1, 1)) for f in ("TPSS", "TPSSh")]


# ---- a. the XC force on synthetic planes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("functional,shape", FD_CASES, ids=lambda v: str(v))
def test_host_gradient_against_finite_differences(functional, shape):
    cols, ref, bar = um.reference(functional, shape)
    G = um.host_gradient(functional, shape)
    assert G.shape == (shape[1], 3)
    um.check_fd("cpu", f"xc_gradient_meta_spin_host {functional} {shape}", G[list(cols)], ref, bar)


@pytest.mark.parametrize("functional,shape", FD_CASES, ids=lambda v: str(v))
def test_without_the_tau_lines_the_gradient_misses(functional, shape):
    """The same call without the tau lines misses the differences by more than 1e-3 of the scale: the case above cannot pass
    without them."""
    cols, ref, bar = um.reference(functional, shape)
    dm_a, dm_b, ao, gr, w, hs = um.inputs(*shape)
    G0 = gradients.xc_gradient_meta_spin_host(functional, dm_a, dm_b, ao, w, gr, hs, tau_term=False)[list(cols)]
    scale = float(np.abs(ref).max())
    miss = float(np.abs(G0 - ref).max())
    print(f"cpu xc_gradient_meta_spin_host {functional} {shape} without the tau lines: miss {miss / scale:.2e}")
    um.record("cpu", f"without the tau lines {functional} {shape}: the miss", bar / scale, miss / scale)
    assert miss > 1e-3 * scale and miss > 100.0 * max(10.0 * bar, 1e-9 * scale)


# ---- b. limits and sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", ["TPSS", "TPSSh"])
def test_closed_shell_limit(functional):
    import meta_gradient_reference as mg
    dm, ao, gr, w, hs = mg.inputs(333, 24)
    G = gradients.xc_gradient_meta_spin_host(functional, 0.5 * dm, 0.5 * dm, ao, w, gr, hs)
    G0 = mg.host_gradient(functional, 333, 24)
    err = float(np.abs(G - G0).max() / np.abs(G0).max())
    print(f"cpu xc_gradient_meta_spin_host {functional} (dm/2, dm/2) against xc_gradient_meta_host(dm): {err:.2e}")
    um.record("cpu", f"(dm/2, dm/2) against xc_gradient_meta_host {functional} (333, 24)", None, err)
    assert err <= sr.CLOSED_SHELL_BAR
    e = gradients.xc_energy_density_meta_spin_host(functional, 0.5 * dm, 0.5 * dm, ao, gr)
    e0 = gradients.xc_energy_density_meta_host(functional, dm, ao, gr)
    assert np.abs(e - e0).max() <= sr.CLOSED_SHELL_BAR * np.abs(e0).max()


@pytest.mark.parametrize("mix", ["PBE0", "BLYP", "slater_x + pw92_c"])
def test_zero_meta_weights_give_the_mix(mix):
    dm_a, dm_b, ao, gr, w, hs = um.inputs(333, 24, 5, 4)
    G = gradients.xc_gradient_meta_spin_host(mix, dm_a, dm_b, ao, w, gr, hs)
    G0 = gradients.xc_gradient_spin_host(mix, dm_a, dm_b, ao, w, gr, hs)
    err = float(np.abs(G - G0).max() / np.abs(G0).max())
    print(f"cpu xc_gradient_meta_spin_host {mix} against xc_gradient_spin_host: {err:.2e}")
    um.record("cpu", f"zero meta weights {mix} (333, 24, 5, 4) against xc_gradient_spin_host", None, err)
    assert err <= sr.CLOSED_SHELL_BAR
    e = gradients.xc_energy_density_meta_spin_host(mix, dm_a, dm_b, ao, gr)
    e0 = gradients.xc_energy_density_spin_host(mix, dm_a, dm_b, ao, gr)
    assert np.abs(e - e0).max() <= sr.CLOSED_SHELL_BAR * np.abs(e0).max()


def test_an_empty_beta_channel_contributes_nothing():
    dm_a, dm_b, ao, gr, w, hs = um.inputs(333, 24, 3, 0)
    assert not np.any(dm_b)
    for functional in um.FUNCTIONALS:
        G = um.host_gradient(functional, (333, 24, 3, 0))
        # beta's coefficient planes may be anything at rho_b = 0: with D_b = 0 nothing of them reaches G
        from quantum_compute_dft_amd import gradients as gr_mod
        ra, ga, ta, rb, gb, tb = metagga.density_spin_host(dm_a, dm_b, ao, gr)
        p = metagga.point_meta_spin_host(functional, ra, rb, ga, gb, ta, tb, w)
        Ga = gr_mod._xc_contract(1.0, True, ao, gr, hs, [(dm_a, p["coef_a"])])
        Y = [gr[k] @ dm_a for k in range(3)]
        for x in range(3):
            Ga[:, x] -= 2.0 * np.einsum("g,gm->m", p["ct_a"], sum(hs[gr_mod.HESS_INDEX[x][k]] * Y[k] for k in range(3)))
        assert np.all(np.isfinite(G)) and np.abs(G - Ga).max() <= 1e-14 * np.abs(G).max()


def test_only_the_symmetric_part_counts_and_the_planes_are_needed():
    shape = (333, 24, 5, 4)
    dm_a, dm_b, ao, gr, w, hs = um.inputs(*shape)
    a = np.random.default_rng(11).standard_normal(dm_a.shape)
    G = gradients.xc_gradient_meta_spin_host("TPSS", dm_a + (a - a.T), dm_b - 0.5 * (a - a.T), ao, w, gr, hs)
    assert np.abs(G - um.host_gradient("TPSS", shape)).max() <= 1e-12 * np.abs(G).max()
    with pytest.raises(ValueError, match="needed for a meta-GGA"):
        gradients.xc_gradient_meta_spin_host("TPSS", dm_a, dm_b, ao, w, gr, None)
    with pytest.raises(ValueError, match="needed for a meta-GGA"):
        gradients.xc_energy_density_meta_spin_host("TPSS", dm_a, dm_b, ao, None)


@pytest.mark.parametrize("shape", [(333, 114, 9, 7), (333, 24, 3, 0), (333, 24, 1, 1)], ids=str)
def test_energy_density_sums_to_exc(shape):
    dm_a, dm_b, ao, gr, w, _ = um.inputs(*shape)
    for functional in um.FUNCTIONALS:
        e = gradients.xc_energy_density_meta_spin_host(functional, dm_a, dm_b, ao, gr)
        exc = metagga.xc_meta_spin_host(functional, dm_a, dm_b, ao, w, gr)[0]
        err = abs(float(np.sum(w * e)) - exc) / abs(exc)
        print(f"cpu sum w e against xc_meta_spin_host's Exc {functional} {shape}: {err:.2e}")
        assert err <= 1e-12


# ---- c. the whole gradient ------------------------------------------------------------------------------------------------
def _run(base, functional, charge, spin, xyz, fixed_grid=True):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz, charge=charge, spin=spin)
    if fixed_grid and base is not None:
        inp = dataclasses.replace(inp, grids=base.grids)
    be = UksMetaHostBackend(inp, functional)
    res = scf.run_uks(inp, be, functional, meta=True, **ug.KW)
    assert res["converged"]
    return inp, be, res


def _whole(label, functional, charge, spin, fixed):
    H = ug.H
    xyz = ug._stretched("sto-3g", -0.15)
    base = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz, charge=charge, spin=spin)
    inp, be, res = _run(base, functional, charge, spin, base.atom_xyz, fixed)
    g, terms = gradients.nuclear_gradient_uks(inp, res, be, functional, grid_response=not fixed, meta=True)
    assert set(terms) == ug.TERMS | (set() if fixed else {"xc_grid"})
    assert np.allclose(sum(terms.values()), g, rtol=0, atol=1e-14)
    assert np.abs(terms["xc"]).max() > 1e-2              # TPSS's eight GGA weights are all zero: the meta weights count
    directions = [ug._unit(3, 0, 2), ug._unit(3, 1, 1), ug._random(3)]
    refs = []
    for d in directions:
        E = {t: _run(base, functional, charge, spin, base.atom_xyz + t * d, fixed)[2]["E_tot"] for t in (H, -H, 2 * H, -2 * H)}
        D1, D2 = (E[H] - E[-H]) / (2 * H), (E[2 * H] - E[-2 * H]) / (4 * H)
        ref = (4.0 * D1 - D2) / 3.0
        refs.append((ref, abs(ref - D1)))
    scale = max(abs(r) for r, _ in refs[:-1])
    name = f"nuclear_gradient_uks(meta=True) H2O/sto-3g {label} grid {'fixed' if fixed else 'rebuilt'}"
    figures = []
    for k, (d, (ref, bar)) in enumerate(zip(directions, refs)):
        an = float(np.sum(g * d))
        print(f"cpu {name} direction {k}: analytic {an:+.10e}  D_R {ref:+.10e}  bar {bar / scale:.2e}  err {abs(an - ref) / scale:.2e}")
        um.record("cpu", f"{name} direction {k}", bar / scale, abs(an - ref) / scale, "max|g|")
        figures.append((k, bar, abs(an - ref)))
    for k, bar, err in figures:
        assert 10.0 * bar <= 1e-5 * scale, (name, k, bar / scale)
        assert err <= max(10.0 * bar, 1e-9 * scale), (name, k, err / scale, bar / scale)
    net = float(np.abs(g.sum(axis=0)).max())
    print(f"cpu {name}: E {res['E_tot']:.9f}  <S^2> {res['s_squared']:.4f}  max|g| {np.abs(g).max():.3e}  net force {net:.2e}")
    return g, net


@pytest.mark.parametrize("label,functional,charge,spin", [("H2O+ doublet TPSS", "TPSS", 1, 1), ("H2O+ doublet TPSSh", "TPSSh", 1, 1),
                                                          ("H2O triplet TPSS", "TPSS", 0, 2)])
def test_whole_gradient(label, functional, charge, spin):
    _, net = _whole(label, functional, charge, spin, True)
    assert net > 1e-6                                    # grid level 1: the fixed quadrature's share is there to be removed


def test_whole_gradient_with_the_grid_response():
    _, net = _whole("H2O+ doublet TPSS", "TPSS", 1, 1, False)
    assert net <= 1e-12


def test_spin_zero_is_the_closed_shell_meta_gradient():
    xyz = ug._stretched("sto-3g", -0.15)
    inp, be, res = _run(None, "TPSS", 0, 0, xyz)
    g, terms = gradients.nuclear_gradient_uks(inp, res, be, "TPSS", meta=True)
    rbe = MetaHostBackend(inp, "TPSS")
    rres = scf.run_scf(inp, rbe, "TPSS", **ug.KW)
    assert rres["converged"]
    ref, ref_terms = gradients.nuclear_gradient(inp, rres, rbe, "TPSS", meta=True)
    for k in ref_terms:
        print(f"cpu nuclear_gradient_uks(meta=True) H2O/STO-3G TPSS spin 0 against nuclear_gradient(meta=True), {k}: "
              f"{np.abs(terms[k] - ref_terms[k]).max():.2e} Ha/bohr")
    err = float(np.abs(g - ref).max())
    um.record("cpu", "spin 0 against nuclear_gradient(meta=True) H2O/sto-3g TPSS, Ha/bohr", None, err, "1")
    assert err <= 1e-9


# ---- d. refusals ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cation():
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, charge=1, spin=1)
    be = UksMetaHostBackend(inp, "TPSS")
    res = scf.run_uks(inp, be, "TPSS", log=None, meta=True)
    assert res["converged"]
    return inp, be, res


def test_the_keyword_is_needed_and_named(cation):
    inp, be, res = cation
    with pytest.raises(ValueError) as e:
        gradients.nuclear_gradient_uks(inp, res, be, "TPSS")
    msg = str(e.value)
    assert "meta-GGA" in msg and "not built" in msg and "meta=True" in msg and "--open-shell-meta-gradient" in msg
    assert "--open-shell-meta-gradient" in functionals.OPEN_SHELL_META_GRADIENT_HINT
    # the keyword changes nothing for anybody else
    assert gradients.nuclear_gradient_uks.__defaults__[-1] is False
    assert gradients.nuclear_gradient.__defaults__[-1] is False


def test_assembly_refusals(cation):
    inp, be, res = cation
    with pytest.raises(ValueError, match="is not one"):                       # a functional that is no meta-GGA
        gradients.nuclear_gradient_uks(inp, res, UksMetaHostBackend(inp, "PBE0"), "PBE0", meta=True)
    with pytest.raises(ValueError, match="uks_meta_parts.*this backend has none"):
        gradients.nuclear_gradient_uks(inp, res, UksHostBackend(inp, "B3LYP"), "TPSS", meta=True)
    with pytest.raises(ValueError, match="uniform electric field"):
        gradients.nuclear_gradient_uks(dataclasses.replace(inp, efield=np.array([0.0, 0.0, 1e-3])), res, be, "TPSS", meta=True)

    class TwoRanks(UksMetaHostBackend):
        world = 2

    with pytest.raises(ValueError, match="one rank"):
        gradients.nuclear_gradient_uks(inp, res, TwoRanks(inp, "TPSS"), "TPSS", meta=True)
    restricted = {k: v for k, v in res.items() if k not in ("dm_a", "dm_b")}
    with pytest.raises(ValueError, match="run_uks result"):
        gradients.nuclear_gradient_uks(inp, restricted, be, "TPSS", meta=True)
    with pytest.raises(ValueError, match="device two-electron gradient"):
        gradients.nuclear_gradient_uks(inp, res, be, "TPSS", two_electron="device", meta=True)


GRAD = ["--spin", "1", "--charge", "1", "--open-shell-meta", "--open-shell-gradient", "--gradient"]


@pytest.mark.parametrize("argv,needles", [
    # without the new flag the refusal stands, and names it
    (["TPSS", "H2O"] + GRAD, ["meta-GGA", "not built", "--open-shell-meta-gradient"]),
    (["TPSS", "H2O"] + GRAD + ["--grid-response"], ["meta-GGA", "not built", "--open-shell-meta-gradient"]),
    (["TPSS", "H2O"] + GRAD[:-1] + ["--optimize"], ["meta-GGA", "not built", "--open-shell-meta-gradient"]),
    # a companion is missing: named
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--gradient"], ["--spin N", "--open-shell-meta", "--open-shell-gradient", "missing"]),
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--spin", "1", "--charge", "1", "--open-shell-meta", "--gradient"],
     ["--open-shell-gradient is missing"]),
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--spin", "1", "--charge", "1", "--open-shell-gradient", "--gradient"],
     ["--open-shell-meta is missing"]),
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--spin", "1", "--charge", "1", "--open-shell-meta", "--open-shell-gradient"],
     ["--gradient or --optimize is missing"]),
    # no meta-GGA
    (["PBE0", "H2O", "--quirks", "0", "--open-shell-meta-gradient", "--spin", "1", "--charge", "1", "--open-shell-gradient", "--gradient"],
     ["--open-shell-meta-gradient is for a meta-GGA"]),
    # what stays refused with the flag
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--meta-gradient"] + GRAD, ["closed-shell gradient of a meta-GGA"]),
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--polarizability", "--open-shell-response"] + GRAD, ["--polarizability", "not built"]),
    (["TPSS", "H2O", "--open-shell-meta-gradient", "--efield", "0", "0", "0.001"] + GRAD, ["--efield"]),
])
def test_driver_refuses_before_it_touches_a_device(argv, needles, capsys):
    from quantum_compute_dft_amd import dft
    with pytest.raises(SystemExit) as e:
        dft.main(argv + ["--basis", "sto-3g"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    for needle in needles:
        assert needle in err, (needle, err)


def test_driver_flag_parses():
    from quantum_compute_dft_amd import dft
    a = dft.build_parser().parse_args(["TPSS", "H2O", "--open-shell-meta-gradient", "--grid-response", "--grad2e", "device"] + GRAD)
    assert a.open_shell_meta_gradient and a.open_shell_meta and a.open_shell_gradient and a.grid_response and a.grad2e == "device"
    assert not dft.build_parser().parse_args(["TPSS", "H2O"] + GRAD).open_shell_meta_gradient


def _header_int(text, name):
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def first_nao_past_lds():
    """{fused: the first nao whose tiles do not fit 160 KB}, from the constants of the launch headers: the fused kernel's six
    tiles at its K chunk; the plain form's larger request, k_xc_grad's two tiles or k_xc_grad_meta<false>'s three."""
    csrc = os.path.join(os.path.dirname(q.__file__), "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in ("xc_grad_launch.hpp", "xc_grad_meta_launch.hpp", "xc_grad_meta_spin_launch.hpp"))
    rows = _header_int(text, "XCG_ROWS")

    def lds(nao, tiles, cap, ncs):
        NP = (nao + 15) // 16 * 16
        return 8 * (tiles * rows * (min(NP, cap) | 1) + 3 * NP + ncs)

    forms = {1: lambda n: lds(n, 6, _header_int(text, "XCGMS_KC_MAX"), 160),
             0: lambda n: max(lds(n, 2, _header_int(text, "XCG_KC_MAX"), 64), lds(n, 3, _header_int(text, "XCGT_KC_MAX"), 16))}
    return {fused: next(n for n in range(1, 4000) if f(n) > 160 * 1024) for fused, f in forms.items()}


def test_library_refusals_without_a_device():
    lib = q.load_library(q.build_library())
    dp, u64 = ctypes.POINTER(ctypes.c_double), ctypes.c_uint64
    for name in ("DFT_ComputeXCGradientMetaSpin", "DFT_ComputeXCEnergyDensityMetaSpin"):
        assert hasattr(lib, name), name
    lib.DFT_CreateSolverMeta.argtypes, lib.DFT_CreateSolverMeta.restype = [dp, ctypes.c_int, dp, ctypes.c_int], ctypes.c_void_p
    lib.DFT_CreateSolverMix.argtypes, lib.DFT_CreateSolverMix.restype = [dp, ctypes.c_int], ctypes.c_void_p
    lib.DFT_GetLastError.argtypes, lib.DFT_GetLastError.restype = [ctypes.c_void_p], ctypes.c_char_p
    lib.DFT_DestroySolver.argtypes = [ctypes.c_void_p]
    lib.DFT_SetOption.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]
    lib.DFT_GetOption.argtypes, lib.DFT_GetOption.restype = [ctypes.c_void_p, ctypes.c_char_p], ctypes.c_double
    lib.DFT_ComputeXCGradientMetaSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [u64] * 7
    lib.DFT_ComputeXCEnergyDensityMetaSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [u64] * 5
    lib.DFT_GetVersion.restype = ctypes.c_int
    assert lib.DFT_GetVersion() == 5
    arr = lambda v: (ctypes.c_double * len(v))(*v)
    s = lib.DFT_CreateSolverMeta(arr([0.0] * 8), 8, arr([1.0, 1.0]), 2)
    k = lib.DFT_CreateSolverMeta(arr([0, 0, 0, 0, 0, 1.0, 0, 0]), 8, arr([1.0, 0.0]), 2)      # tpss_x + pbe_c, quirks = 1 by default
    g = lib.DFT_CreateSolverMix(arr([0, 0, 0, 0, 1.0, 1.0, 0, 0]), 8)
    assert s and k and g
    P = 8                      # a non-null address: every refusal below comes before anything is read
    try:
        def grad(h, ng=10, n=4, ptrs=(P,) * 7):
            rc = lib.DFT_ComputeXCGradientMetaSpin(h, ng, n, *ptrs)
            return rc, lib.DFT_GetLastError(h).decode()

        def dens(h, ng=10, n=4, ptrs=(P,) * 5):
            rc = lib.DFT_ComputeXCEnergyDensityMetaSpin(h, ng, n, *ptrs)
            return rc, lib.DFT_GetLastError(h).decode()

        for entry, name, nptr in ((grad, "DFT_ComputeXCGradientMetaSpin", 7), (dens, "DFT_ComputeXCEnergyDensityMetaSpin", 5)):
            rc, msg = entry(g)
            assert rc == -1 and name in msg and "DFT_CreateSolverMeta" in msg and "no meta-GGA weights" in msg
            for i in range(nptr):              # every pointer, both matrices, ao_grad and ao_hess included
                rc, msg = entry(s, ptrs=tuple(0 if j == i else P for j in range(nptr)))
                assert rc == -1 and name in msg and "a pointer is null" in msg, i
            for kw in ({"ng": 0}, {"n": 0}, {"ng": -1}):
                rc, msg = entry(s, **kw)
                assert rc == -1 and "bad sizes" in msg
            rc, msg = entry(k)
            assert rc == -1 and "quirks = 1" in msg and "not the derivatives of their energies" in msg
            # two faults in one call: the first in the order the header states
            rc, msg = entry(g, ptrs=(0,) + (P,) * (nptr - 1))
            assert rc == -1 and "no meta-GGA weights" in msg
            rc, msg = entry(s, ng=0, ptrs=(0,) + (P,) * (nptr - 1))
            assert rc == -1 and "a pointer is null" in msg
            rc, msg = entry(k, n=0)
            assert rc == -1 and "bad sizes" in msg
        past = first_nao_past_lds()
        assert past[1] > 1150 and past[0] > 1150           # the largest basis of the benchmark configurations fits both forms
        for fused, nao in past.items():     # the first basis past each form's 160 KB (every call here is refused: nothing is read)
            assert lib.DFT_SetOption(s, b"xcg_meta_spin_fused", float(fused)) == 0 and lib.DFT_GetOption(s, b"xcg_meta_spin_fused") == fused
            rc, msg = grad(s, n=nao)
            assert rc == -1 and "bytes of LDS per workgroup" in msg and f"nao={nao}" in msg and "DFT_ComputeXCGradientMetaSpin" in msg
            rc, msg = grad(k, n=nao)           # quirks before the LDS request
            assert rc == -1 and "quirks = 1" in msg
        # DFT_ComputeXCGradientMeta's own limits stay where they were
        lib.DFT_ComputeXCGradientMeta.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [u64] * 6
        for fused, nao in ((1.0, 1217), (0.0, 1329)):
            assert lib.DFT_SetOption(s, b"xcg_meta_fused", fused) == 0
            assert lib.DFT_ComputeXCGradientMeta(s, 10, nao, *(P,) * 6) == -1 and "bytes of LDS" in lib.DFT_GetLastError(s).decode()
    finally:
        for h in (s, k, g):
            lib.DFT_DestroySolver(h)


# ---- e. the optimiser -----------------------------------------------------------------------------------------------------
def test_optimiser_relaxes_the_cation():
    """H2O+/STO-3G TPSS from the shipped geometry with one O-H bond stretched by 0.2 bohr, grid level 1, the grid response on,
    every step through run_uks(meta=True): converged at the customary thresholds, lower in energy than the start, the net
    force at rounding level all the way."""
    base = inputs.build("H2O", "sto-3g", 1, verbose=False, charge=1, spin=1)
    xyz0 = base.atom_xyz.copy()
    bond = xyz0[1] - xyz0[0]
    xyz0[1] += 0.2 * bond / np.linalg.norm(bond)
    nets = []

    def fun(xyz):
        inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz, charge=1, spin=1)
        be = UksMetaHostBackend(inp, "TPSS")
        res = scf.run_uks(inp, be, "TPSS", log=None, conv_e=1e-10, conv_dm=1e-8, meta=True)
        assert res["converged"]
        g = gradients.nuclear_gradient_uks(inp, res, be, "TPSS", grid_response=True, meta=True)[0]
        nets.append(float(np.abs(g.sum(axis=0)).max()))
        return res["E_tot"], g

    out = optimize.bfgs(fun, xyz0, max_steps=30)
    print(f"cpu UKS optimiser TPSS, grid level 1, grid response on: {out['steps']} steps, {out['evaluations']} evaluations, "
          f"E {out['energies'][0]:.8f} -> {out['energy']:.8f}, max|g| {np.abs(out['gradient']).max():.2e}, largest net force on the way {max(nets):.2e}")
    assert out["converged"] and out["steps"] <= 30
    assert out["energy"] < out["energies"][0] - 1e-4
    assert optimize.converged(out["gradient"]) and np.abs(out["gradient"]).max() < 3e-4
    assert max(nets) <= 1e-10
