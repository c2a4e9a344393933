"""Grid response of the nuclear gradient on the host: the Becke weight gradient against an independent autograd restatement,
the energy density against the sweep's Exc, the whole gradient with grid_response=True against MOVING-grid differences of
the converged energy, its translational invariance, the flag's default, the refusals, the driver's flag and the optimiser.

Whole gradient: the protocol of tests/test_gradient_scf_cpu.py (H2O/STO-3G, both O-H bonds 0.15 bohr shorter, grid level 1,
SCF to conv_e = conv_dm = 1e-11, central differences at h = 2e-4 bohr and 2 h, Richardson-extrapolated, bar = |D_R - D(h)|;
directions O z, one H y, the seed-3 random unit vector; scale = the largest Cartesian component among D_R) except that the
displaced inputs keep the grid they were built with: the points and the Becke weights follow the atoms.  Per direction

    10 bar <= 1e-6 scale    and    |analytic - D_R| <= max(10 bar, FLOOR scale).

The 1e-9 floor of the fixed-grid tests does not carry over: the moving-grid reference has directions whose bar is
accidentally small (GGA, O z: 7.6e-10 of the scale) while the analytic value sits a few 1e-8
from D_R there -- the h^4 term the extrapolation leaves and the SCF's own convergence, neither of which the bar sees.
FLOOR is three times the worst error of the host implementation on these five cases.  Measured when this was written
(bar / scale, error / scale per direction; profiles/grid_response_parity.txt):

    RKS LDA     1.99e-08 6.58e-08 | 3.84e-08 1.04e-08 | 3.16e-08 3.94e-08
    RKS GGA     7.57e-10 3.95e-08 | 3.11e-08 7.54e-10 | 1.89e-08 6.26e-09
    RKS B3LYP   8.56e-09 1.03e-09 | 4.69e-08 4.52e-08 | 1.99e-08 1.13e-08
    UKS LDA     6.34e-09 5.71e-10 | 2.30e-08 4.64e-10 | 1.51e-08 3.44e-09
    UKS B3LYP   8.41e-09 1.67e-09 | 2.76e-08 6.23e-10 | 1.45e-08 5.65e-09

so FLOOR = 3 x 6.58e-8 = 1.97e-7 of the scale.  Without the term the same gradient misses these references by 2.7e-4 .. 5.6e-3 of the
scale; the net force falls from 1.6e-6 .. 8.6e-4 to 1e-14 .. 3e-14 Ha/bohr.
"""
import dataclasses
import functools
import os
import types

import numpy as np
import pytest

import grid_response_reference as gref
import oracle
from quantum_compute_dft_amd import basis, gradients, grid_gen, inputs, optimize, response, scf
from scf_oracle_backend import OracleBackend
from uks_host_backend import UksHostBackend

H = 2e-4
KW = dict(log=None, conv_e=1e-11, conv_dm=1e-11)
ERR_REL = 2e-8          # the project's bound for a contracted gradient (tests/test_gpu_xc_gradient.py)
FLOOR = 3 * 6.58e-8     # three times the worst host error above, in units of the scale
TERMS = {"one_electron", "two_electron", "xc", "nuclear", "external"}


def record(label, bar_rel, err_rel, what):
    """One line per figure into grid_response_parity.txt in the directory QCDFT_WRITE_PROFILES names (how
    profiles/grid_response_parity.txt was made); an ordinary test run only prints."""
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "grid_response_parity.txt")
    key = f"{label:78s}"
    bar = "         " if bar_rel is None else f"{bar_rel:9.2e}"
    line = f"{key} reference bar / {what} {bar}   error / {what} {err_rel:9.2e}"
    os.makedirs(out_dir, exist_ok=True)
    old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
    head = [l for l in old if l.startswith("#")] or [
        "# Grid response of the nuclear gradient (tests/test_grid_response_cpu.py: cpu; tests/test_gpu_grid_response.py: gpu).",
        "# Weight gradient: host against autograd, device against host: error <= 2e-8 of the largest component; cell: 1e-12.",
        "# Whole gradient against moving-grid differences: 10 bar <= 1e-6 scale, error <= max(10 bar, 1.97e-7 scale)."]
    body = sorted([l for l in old if l and not l.startswith("#") and not l.startswith(key)] + [line])
    with open(path, "w") as fh:
        fh.write("\n".join(head + body) + "\n")


# ---- the weight gradient against autograd ------------------------------------------------------------------------------
def _h2o_grid():
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    return inp.grids.coords, inp.grids.atom_index, inp.atom_xyz, [basis.atomic_number(s) for s in inp.symbols]


def _weight_case(name):
    rng = np.random.default_rng(11)
    if name == "one atom":
        g = grid_gen.Grids(["O"], np.zeros((1, 3)), level=1)
        return g.coords, g.atom_index, g.atom_xyz, [8]
    if name == "H-O":
        xyz = np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 1.8]])
        g = grid_gen.Grids(["H", "O"], xyz, level=1)
        return g.coords, g.atom_index, xyz, [1, 8]
    if name == "H2O level 1":
        return _h2o_grid()
    if name == "13-atom cluster":
        xyz = rng.uniform(-4.0, 4.0, (13, 3))
        sym = [str(s) for s in rng.choice(["H", "C", "N", "O", "S"], 13)]
        g = grid_gen.Grids(sym, xyz, level=0)
        keep = rng.choice(g.size, 1100, replace=False)
        return g.coords[keep], g.atom_index[keep], xyz, [basis.atomic_number(s) for s in sym]
    if name == "point on a foreign nucleus":
        co, own, xyz, z = _h2o_grid()
        keep = rng.choice(len(own), 400, replace=False)
        co, own = np.vstack([co[keep], xyz[[1, 0, 2]]]), np.concatenate([own[keep], [0, 2, 1]])   # O's point on H1, H2's on O, H1's on H2
        return co, own, xyz, z
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one atom", "H-O", "H2O level 1", "13-atom cluster", "point on a foreign nucleus"])
def test_weight_gradient_against_autograd(name):
    co, own, xyz, z = _weight_case(name)
    f = np.random.default_rng(5).standard_normal(len(own))
    got = grid_gen.becke_weight_gradient_host(co, own, xyz, z, f)
    ref, cell = gref.becke_weight_gradient_autograd(co, own, xyz, z, f)
    assert got.shape == (len(z), 3) and np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    if len(z) == 1:
        assert np.all(got == 0.0) and np.all(ref == 0.0)
        return
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max() / scale
    print(f"cpu weight gradient {name}: {len(own)} points, {len(z)} atoms, {int((cell == 0).sum())} exact-zero cells, "
          f"smallest positive {cell[cell > 0].min():.1e}, max {scale:.3e}, err {err:.2e}, rows sum {np.abs(got.sum(axis=0)).max():.1e}")
    record(f"cpu  weight gradient host / autograd, {name}", None, err, "max|out|")
    assert np.allclose(cell, grid_gen.becke_weights(co, own, xyz, z), rtol=0, atol=1e-12)      # the reference restates the same cell function (the bound of a plane)
    assert err <= ERR_REL
    assert np.abs(got.sum(axis=0)).max() <= 1e-12 * scale * np.sqrt(len(own))                   # the owner fold: translational invariance
    if name == "H2O level 1":
        assert (cell == 0).sum() > 0                                                            # the trap is in the case


def test_weight_gradient_host_refuses():
    co, own, xyz, z = _h2o_grid()
    f = np.ones(len(own))
    with pytest.raises(ValueError, match="outside the atoms"):
        grid_gen.becke_weight_gradient_host(co, own + 1, xyz, z, f)
    with pytest.raises(ValueError, match="one entry per point"):
        grid_gen.becke_weight_gradient_host(co, own, xyz, z, f[:-1])
    with pytest.raises(ValueError, match="coincide"):
        grid_gen.becke_weight_gradient_host(co, own, xyz[[0, 1, 1]], z, f)


def test_grids_keep_the_atomic_weights():
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False)
    g = inp.grids
    z = [basis.atomic_number(s) for s in inp.symbols]
    assert g.atomic_weights.shape == g.weights.shape == g.atom_index.shape
    assert np.array_equal(g.weights, g.atomic_weights * grid_gen.becke_weights(g.coords, g.atom_index, g.atom_xyz, z))
    one = grid_gen.Grids(["O"], np.zeros((1, 3)), level=1)
    assert np.array_equal(one.weights, one.atomic_weights)


# ---- the energy density ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rks(functional, quirks):
    xyz = _short_bonds()
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz)
    be = OracleBackend(inp, functional, quirks=quirks)
    res = scf.run_scf(inp, be, functional, **KW)
    assert res["converged"]
    return inp, be, res


@functools.lru_cache(maxsize=None)
def _uks(functional):
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=_short_bonds(), charge=1, spin=1)
    be = UksHostBackend(inp, functional)
    res = scf.run_uks(inp, be, functional, **KW)
    assert res["converged"]
    return inp, be, res


def _short_bonds():
    xyz = inputs.build("H2O", "sto-3g", 1, verbose=False).atom_xyz.copy()
    for k in (1, 2):
        b = xyz[k] - xyz[0]
        xyz[k] -= 0.15 * b / np.linalg.norm(b)
    return xyz


@pytest.mark.parametrize("functional,quirks", [("LDA", False), ("GGA", False), ("B3LYP", True)])
def test_energy_density_sums_to_exc(functional, quirks):
    inp, be, res = _rks(functional, quirks)
    dm = np.asarray(res["dm"])
    e = gradients.xc_energy_density_host(functional, dm, be.ao, be.gr, quirks)
    exc = oracle.compute_xc(be.t, np.ascontiguousarray(dm), be.ao, inp.grids.weights, be.gr, quirks=quirks)[0]
    got = float(inp.grids.weights @ e)
    print(f"cpu energy density {functional}: sum w e {got:.12f}  Exc {exc:.12f}")
    assert np.all(np.isfinite(e)) and abs(got - exc) <= 1e-12 * abs(exc)


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_energy_density_spin_sums_to_exc(functional):
    inp, be, res = _uks(functional)
    e = gradients.xc_energy_density_spin_host(functional, res["dm_a"], res["dm_b"], be.ao, be.gr)
    exc = response.xc_spin_host(functional, res["dm_a"], res["dm_b"], be.ao, inp.grids.weights, be.gr)[0]
    got = float(inp.grids.weights @ e)
    print(f"cpu spin energy density {functional}: sum w e {got:.12f}  Exc {exc:.12f}")
    assert np.all(np.isfinite(e)) and abs(got - exc) <= 1e-12 * abs(exc)


# ---- the whole gradient against moving-grid differences ------------------------------------------------------------------
def _unit(atom, axis):
    d = np.zeros((3, 3))
    d[atom, axis] = 1.0
    return d


def _random():
    d = np.random.default_rng(3).standard_normal((3, 3))
    return d / np.linalg.norm(d)


def _energy(kind, functional, quirks, xyz):
    """The converged energy at xyz on the grid built there: points and weights follow the atoms."""
    if kind == "RKS":
        inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz)
        res = scf.run_scf(inp, OracleBackend(inp, functional, quirks=quirks), functional, **KW)
    else:
        inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz, charge=1, spin=1)
        res = scf.run_uks(inp, UksHostBackend(inp, functional), functional, **KW)
    assert res["converged"]
    return res["E_tot"]


def whole_gradient_case(kind, functional, quirks, check=True):
    """(g, terms, figures): figures = (bar / scale, error / scale) per direction, printed and recorded before the assertions."""
    if kind == "RKS":
        inp, be, res = _rks(functional, quirks)
        g, terms = gradients.nuclear_gradient(inp, res, be, functional, quirks=quirks, grid_response=True)
    else:
        inp, be, res = _uks(functional)
        g, terms = gradients.nuclear_gradient_uks(inp, res, be, functional, grid_response=True)
    assert set(terms) == TERMS | {"xc_grid"}
    assert np.allclose(sum(terms.values()), g, rtol=0, atol=1e-14)
    directions = [_unit(0, 2), _unit(1, 1), _random()]
    refs = []
    for d in directions:
        E = {t: _energy(kind, functional, quirks, inp.atom_xyz + t * d) for t in (H, -H, 2 * H, -2 * H)}
        D1, D2 = (E[H] - E[-H]) / (2 * H), (E[2 * H] - E[-2 * H]) / (4 * H)
        ref = (4.0 * D1 - D2) / 3.0
        refs.append((ref, abs(ref - D1)))
    scale = max(abs(r) for r, _ in refs[:-1])
    label = f"whole gradient, moving grid, H2O{'' if kind == 'RKS' else '+ doublet'}/sto-3g {kind} {functional}"
    g_fixed = g - terms["xc_grid"]
    figures = []
    for k, (d, (ref, bar)) in enumerate(zip(directions, refs)):
        an, an0 = float(np.sum(g * d)), float(np.sum(g_fixed * d))
        print(f"cpu {label} direction {k}: analytic {an:+.10e}  D_R {ref:+.10e}  bar {bar / scale:.2e}  err {abs(an - ref) / scale:.2e}"
              f"  (without the term: {abs(an0 - ref) / scale:.2e})")
        record(f"cpu  {label} direction {k}", bar / scale, abs(an - ref) / scale, "scale")
        figures.append((bar / scale, abs(an - ref) / scale))
    net, net0 = np.abs(g.sum(axis=0)).max(), np.abs(g_fixed.sum(axis=0)).max()
    print(f"cpu {label}: net force {net:.2e} Ha/bohr (fixed grid: {net0:.2e})")
    record(f"cpu  {label} net force, Ha/bohr (fixed grid {net0:.1e})", None, net, "1")
    if check:
        for k, (bar, err) in enumerate(figures):
            assert 10.0 * bar <= 1e-6, (label, k, bar)
            assert err <= max(10.0 * bar, FLOOR), (label, k, err, bar)
        assert net <= 1e-10, (label, net)
    return g, terms, figures


@pytest.mark.parametrize("functional,quirks", [("LDA", False), ("GGA", False), ("B3LYP", True)])
def test_whole_gradient_rks(functional, quirks):
    whole_gradient_case("RKS", functional, quirks)


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_whole_gradient_uks(functional):
    whole_gradient_case("UKS", functional, False)


def test_flag_off_is_what_it_was():
    """grid_response=False (the default) adds no key and changes no bit; with it every other term keeps its bits."""
    inp, be, res = _rks("LDA", False)
    g0, t0 = gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False)
    g1, t1 = gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, grid_response=False)
    g2, t2 = gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, grid_response=True)
    assert set(t0) == set(t1) == TERMS and list(t0) == list(t1)
    assert np.array_equal(g0, g1) and all(np.array_equal(t0[k], t1[k]) for k in t0)
    assert all(np.array_equal(t0[k], t2[k]) for k in t0) and np.abs(t2["xc_grid"]).max() > 1e-6
    inp, be, res = _uks("LDA")
    g0, t0 = gradients.nuclear_gradient_uks(inp, res, be, "LDA")
    g1, t1 = gradients.nuclear_gradient_uks(inp, res, be, "LDA", grid_response=False)
    g2, t2 = gradients.nuclear_gradient_uks(inp, res, be, "LDA", grid_response=True)
    assert set(t0) == set(t1) == TERMS and np.array_equal(g0, g1) and all(np.array_equal(t0[k], t1[k]) for k in t0)
    assert all(np.array_equal(t0[k], t2[k]) for k in t0)


def test_a_functional_without_a_sweep_has_a_zero_term():
    import triplet_reference as tr
    inp = inputs.build("H2O", "sto-3g", 1, verbose=False, charge=1, spin=1)
    be = UksHostBackend(inp, tr.HF)
    res = scf.run_uks(inp, be, tr.HF, log=None)
    _, terms = gradients.nuclear_gradient_uks(inp, res, be, tr.HF, grid_response=True)
    assert np.all(terms["xc_grid"] == 0.0) and np.all(terms["xc"] == 0.0)


def test_refusals():
    inp, be, res = _rks("LDA", False)
    call = functools.partial(gradients.nuclear_gradient, functional="LDA", quirks=False, grid_response=True)
    g = inp.grids
    bare = types.SimpleNamespace(coords=g.coords, weights=g.weights, size=g.size)
    with pytest.raises(ValueError, match="no atom_index / atomic_weights"):
        call(dataclasses.replace(inp, grids=bare), res, be)
    no_w0 = types.SimpleNamespace(coords=g.coords, weights=g.weights, size=g.size, atom_index=g.atom_index)
    with pytest.raises(ValueError, match="no atom_index / atomic_weights"):
        call(dataclasses.replace(inp, grids=no_w0), res, be)
    for own, w0 in ((g.atom_index + 1, g.atomic_weights), (g.atom_index[:-1], g.atomic_weights), (g.atom_index, g.atomic_weights[:-1])):
        bad = types.SimpleNamespace(coords=g.coords, weights=g.weights, size=g.size, atom_index=own, atomic_weights=w0)
        with pytest.raises(ValueError, match="do not match"):
            call(dataclasses.replace(inp, grids=bad), res, be)
    with pytest.raises(ValueError, match="uniform electric field"):
        call(dataclasses.replace(inp, efield=np.array([0.0, 0.0, 1e-3])), res, be)

    class TwoRanks(OracleBackend):
        world = 2

    with pytest.raises(ValueError, match="one rank"):
        call(inp, res, TwoRanks(inp, "LDA", quirks=False))
    with pytest.raises(ValueError, match="--quirks 0"):
        gradients.nuclear_gradient(inp, res, be, "LDA", quirks=True, grid_response=True)
    uinp, ube, ures = _uks("LDA")
    with pytest.raises(ValueError, match="no atom_index / atomic_weights"):
        gradients.nuclear_gradient_uks(dataclasses.replace(uinp, grids=bare), ures, ube, "LDA", grid_response=True)
    with pytest.raises(ValueError, match="ao_grad is needed"):
        gradients.xc_energy_density_host("GGA", res["dm"], be.ao, None, False)


@pytest.mark.parametrize("argv", [["LDA", "H2O", "--grid-response"],
                                  ["B3LYP", "H2O", "--grid-response", "--spin", "1", "--charge", "1"]])
def test_driver_refuses_the_flag_alone(argv, capsys):
    from quantum_compute_dft_amd import dft
    with pytest.raises(SystemExit) as e:
        dft.main(argv)
    assert e.value.code == 2
    assert "--grid-response goes with --gradient or --optimize" in capsys.readouterr().err


def test_optimiser_relaxes_a_stretched_bond_at_grid_level_1():
    """H2O/STO-3G LDA (quirks 0) from the shipped geometry with one O-H bond stretched by 0.2 bohr, at grid level 1 -- where the
    fixed-grid gradient leaves a net force above the optimiser's thresholds -- with the grid response on: converged at the
    customary thresholds, lower in energy than the start, and the net force stays at rounding level all the way."""
    base = inputs.build("H2O", "sto-3g", 1, verbose=False)
    xyz0 = base.atom_xyz.copy()
    bond = xyz0[1] - xyz0[0]
    xyz0[1] += 0.2 * bond / np.linalg.norm(bond)
    nets = []

    def fun(xyz):
        inp = inputs.build("H2O", "sto-3g", 1, verbose=False, atom_xyz=xyz)
        be = OracleBackend(inp, "LDA", quirks=False)
        res = scf.run_scf(inp, be, "LDA", log=None, conv_e=1e-10, conv_dm=1e-8)
        assert res["converged"]
        g = gradients.nuclear_gradient(inp, res, be, "LDA", quirks=False, grid_response=True)[0]
        nets.append(float(np.abs(g.sum(axis=0)).max()))
        return res["E_tot"], g

    out = optimize.bfgs(fun, xyz0, max_steps=30)
    print(f"cpu optimiser, grid level 1, grid response on: {out['steps']} steps, {out['evaluations']} evaluations, "
          f"E {out['energies'][0]:.8f} -> {out['energy']:.8f}, max|g| {np.abs(out['gradient']).max():.2e}, largest net force on the way {max(nets):.2e}")
    assert out["converged"] and out["steps"] <= 30
    assert out["energy"] < out["energies"][0] - 1e-4
    assert optimize.converged(out["gradient"]) and np.abs(out["gradient"]).max() < 3e-4
    assert max(nets) <= 1e-10
    r1, r2 = (np.linalg.norm(out["xyz"][k] - out["xyz"][0]) for k in (1, 2))
    assert abs(r1 - r2) < 5e-3
