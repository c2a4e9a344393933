"""The open-shell response on the host: the second-derivative table of the spin-resolved energy bodies (lib/libqcfxc.so,
qc_fxc_table_pol: the header the device kernel compiles), response.HostFxcSpin on it, and the UKS solvers
(excitations.UksResponseOperators, the unrestricted CPKS of response.polarizability) on response.HostUksResponse.

1. The table against the 60-digit reference (tests/golden/spin_hessian_ref.npz), entry by entry, per component.
2. fxc_apply_spinpol_host against Richardson-extrapolated differences of response.xc_spin_host: the bound is ten times the
   reference's own bar (spin_response_reference.difference_reference), on inputs with no point at a cut-off.
3. Closed-shell limits: kind 2 (same-sign perturbation) and kind 1 (spin flip) of fxc_apply_host.
4. Spin swap.  5. A fully polarised shape.
6. UKS solvers, H2O and H2O+ / STO-3G: spin 0 against the restricted singlets and triplets, the sum over states against
   the U-CPKS alpha, alpha against the finite field, spin 0 against the restricted alpha, an H atom.  Bars: those of the
   restricted counterparts (tests/test_excitations_cpu.py, tests/test_response_cpu.py).
7. Refusals.
"""
import functools

import numpy as np
import pytest

import spin_reference as sr
import spin_response_reference as rr
import uks_excitation_dense as ued
from quantum_compute_dft_amd import excitations as ex
from quantum_compute_dft_amd import inputs, properties, response, scf
from scf_oracle_backend import OracleBackend
from uks_host_backend import UksHostBackend

KW = dict(log=None, conv_e=1e-12, conv_dm=1e-9)
NAMES = ["ra", "rb", "saa", "sab", "sbb"]


def _grad(functional, gr):
    return gr if functional != "LDA" else None


# ---- 1. the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(sr.COMPONENTS)), ids=sr.COMPONENTS)
def test_table_against_the_60_digit_reference(k):
    g = rr.golden()
    name = sr.COMPONENTS[k]
    H, _ = response.fxc_table_pol_host(sr.unit(k), g["ra"], g["rb"], g["ga"], g["gb"])
    ref = np.moveaxis(g[name], 0, 2)
    absent = np.isnan(ref)
    assert np.all(np.isfinite(H))
    assert np.all(H[absent] == 0.0)                       # rows and columns of an absent channel
    assert absent[:, :, g["zeta"] == 1.0][1].all() and not absent[:, :, np.abs(g["zeta"]) < 1.0].any()
    zero = ~absent & (ref == 0.0)
    assert np.all(H[zero] == 0.0)
    live = ~absent & (ref != 0.0)
    rel = np.zeros_like(H)
    rel[live] = np.abs(H[live] - ref[live]) / np.abs(ref[live])
    i, j, p = np.unravel_index(np.argmax(rel), rel.shape)
    print(f"{name}: worst {rel.max():.2e} at d2/d{NAMES[i]} d{NAMES[j]}, rho {g['ra'][p] + g['rb'][p]:.1e}, zeta {g['zeta'][p]}")
    rr.record(f"cpu hessian {name}", float(rel.max()), rr.HESSIAN_BAR)
    assert live.sum() >= 126
    assert rel.max() <= rr.HESSIAN_BAR


def test_first_derivatives_of_the_table_are_the_potential_points():
    """g of the table is d[] of point_spin_host (pinned by tests/test_spin_potential_cpu.py), bit for bit: the first part of a
    Dual2 evaluation carries the arithmetic of the Dual one."""
    g = rr.golden()
    for functional in ("GGA", "B3LYP"):
        _, g1 = response.fxc_table_pol_host(functional, g["ra"], g["rb"], g["ga"], g["gb"])
        d = response.point_spin_host(functional, g["ra"], g["rb"], g["ga"], g["gb"])[9:14]
        assert np.abs(g1 - d).max() <= 1e-13 * np.abs(d).max() and np.all((g1 == 0.0) == (d == 0.0))


# ---- 2. apply against differences ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", rr.FD_SHAPES, ids=str)
def test_apply_against_differences(shape, functional):
    da, db, d1a, d1b, ao, gr, w = rr.perturbed_inputs(*shape)
    assert shape[2] != shape[3]
    assert rr.no_point_at_a_cutoff(da, db, d1a, d1b, ao, gr)       # the difference quotient is legitimate everywhere
    refs, bars = rr.difference_reference(functional, shape)
    got = response.fxc_apply_spinpol_host(functional, da, db, d1a, d1b, ao, w, _grad(functional, gr))
    for s, v, ref, bar in zip("ab", got, refs, bars):
        scale = float(np.abs(ref).max())
        err = float(np.abs(v - ref).max())
        print(f"apply {functional} {shape} V1_{s}: max|V1| {scale:.3e}  bar {bar / scale:.2e}  err {err / scale:.2e}")
        rr.record(f"cpu apply {functional} {shape} V1_{s} against differences (bar: the reference's own)", err / scale, 10.0 * bar / scale)
        assert np.all(np.isfinite(v))
        assert bar <= rr.FD_BAR_CAP * scale, (bar / scale)
        assert err <= 10.0 * bar, (err / scale, bar / scale)


# ---- 3. closed-shell limits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
@pytest.mark.parametrize("shape", rr.FD_SHAPES, ids=str)
def test_closed_shell_limits(shape, functional):
    da, db, d1, _, ao, gr, w = rr.perturbed_inputs(*shape)
    dm0, g = da + db, _grad(functional, gr)
    fx = response.HostFxcSpin(functional, 0.5 * dm0, 0.5 * dm0, ao, w, g)
    worst = 0.0
    for kind, sign in (("singlet-spin", 1.0), ("triplet", -1.0)):
        va, vb = fx.apply(0.5 * d1, sign * 0.5 * d1)
        ref = response.fxc_apply_host(functional, dm0, d1, ao, w, g, quirks=False, kind=kind)
        err = max(float(np.abs(va - ref).max()), float(np.abs(sign * vb - ref).max())) / float(np.abs(ref).max())
        print(f"closed shell {functional} {shape} {kind}: err {err:.2e}")
        worst = max(worst, err)
    rr.record(f"cpu closed shell {functional} {shape}", worst, rr.CLOSED_SHELL_BAR)
    assert worst <= rr.CLOSED_SHELL_BAR


# ---- 4. spin swap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
def test_spin_swap(functional):
    da, db, d1a, d1b, ao, gr, w = rr.perturbed_inputs(*rr.FD_SHAPES[0])
    g = _grad(functional, gr)
    va, vb = response.fxc_apply_spinpol_host(functional, da, db, d1a, d1b, ao, w, g)
    ub, ua = response.fxc_apply_spinpol_host(functional, db, da, d1b, d1a, ao, w, g)
    scale = max(float(np.abs(va).max()), float(np.abs(vb).max()))
    assert max(float(np.abs(va - ua).max()), float(np.abs(vb - ub).max())) <= 1e-13 * scale


# ---- 5. a fully polarised shape ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("functional", sr.FUNCTIONALS)
def test_fully_polarised(functional):
    da, db, d1a, d1b, ao, gr, w = rr.perturbed_inputs(2085, 50, 3, 0)
    g = _grad(functional, gr)
    assert not db.any() and d1b.any()
    fx = response.HostFxcSpin(functional, da, db, ao, w, g)
    va, vb = fx.apply(d1a, d1b)
    assert np.all(np.isfinite(va)) and np.all(np.isfinite(fx.H)) and np.all(np.isfinite(fx.g)) and va.any()
    assert np.all(vb == 0.0)                               # the absent spin does not respond
    va0, vb0 = fx.apply(d1a, np.zeros_like(d1b))
    assert np.array_equal(va0, va) and np.all(vb0 == 0.0)  # and is not responded to
    assert np.all(fx.H[1] == 0.0) and np.all(fx.H[:, 1] == 0.0) and np.all(fx.H[3:] == 0.0) and np.all(fx.H[:, 3:] == 0.0)


# ---- 6. UKS solvers -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uks_state(functional, charge, spin, mol="H2O", field=None):
    inp = inputs.build(mol, "sto-3g", grid_level=1, verbose=False, charge=charge, spin=spin, **({"efield": field} if field else {}))
    be = UksHostBackend(inp, functional)
    res = scf.run_uks(inp, be, functional, **KW)
    assert res["converged"]
    return inp, res, response.HostUksResponse(inp, functional, be, be.ao, be.gr)


@functools.lru_cache(maxsize=None)
def rks_state(functional):
    inp = inputs.build("H2O", "sto-3g", grid_level=1, verbose=False)
    be = OracleBackend(inp, functional, quirks=False)
    res = scf.run_scf(inp, be, functional, **KW)
    assert res["converged"]
    return inp, res, response.HostResponse(inp, functional, be, be.ao, be.gr, quirks=False)


@pytest.mark.parametrize("tda", [True, False], ids=["tda", "tddft"])
@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_spin_zero_roots_are_the_restricted_singlets_and_triplets(functional, tda):
    inp, res, ub = uks_state(functional, 0, 0)
    out = ex.excitations(inp, res, ub, functional, nroots=6, tda=tda, tol=1e-7)
    rinp, rres, rb = rks_state(functional)
    s = ex.excitations(rinp, rres, rb, functional, nroots=6, tda=tda, tol=1e-7)
    t = ex.excitations(rinp, rres, rb, functional, nroots=6, tda=tda, tol=1e-7, triplet=True)
    w = np.concatenate([s["energies"], t["energies"]])
    f = np.concatenate([s["oscillator_strengths"], np.zeros(6)])
    order = np.argsort(w, kind="stable")[:6]
    dw = float(np.abs(out["energies"] - w[order]).max())
    print(f"spin 0 {functional} {'TDA' if tda else 'TDDFT'}: |dw| {dw:.2e}  w {out['energies']}")
    rr.record(f"cpu uks spin 0 roots against singlets and triplets {functional} {'TDA' if tda else 'TDDFT'} (Ha)", dw, 1e-9)
    assert out["converged"] and out["method"] == ("tda-uks" if tda else "tddft-uks") and out["multiplicity"] is None
    assert dw <= 1e-9                                               # the iterative-against-dense bar of test_excitations_cpu.py
    allw = np.sort(w)
    df = 0.0
    for n in range(6):
        others = np.delete(allw, np.argmin(np.abs(allw - w[order][n])))
        if np.abs(others - w[order][n]).min() > 1e-6:               # f of a root that shares its energy is not defined
            df = max(df, abs(out["oscillator_strengths"][n] - f[order][n]))
    assert df <= 1e-6


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_cation_sum_over_states_is_the_ucpks_alpha(functional):
    inp, res, ub = uks_state(functional, 1, 1)
    ops = ex.UksResponseOperators(inp, res, ub, functional)
    assert ops.size == 5 * 2 + 4 * 3
    out = ex.solve(ops, nroots=ops.size)
    pol = response.polarizability(inp, res, ub, functional)
    w, mu = out["energies"], out["transition_dipoles"]
    sos = 2.0 * np.einsum("nk,nl,n->kl", mu, mu, 1.0 / w)
    err = float(np.abs(sos - pol["alpha"]).max())
    bound = 4.0 * max(np.linalg.norm(pol["dipole_integrals"][k]) for k in range(3)) * max(pol["residual"]) + 1e-10
    print(f"SOS H2O+ {functional}: |sos - alpha| {err:.2e}  bound {bound:.2e}")
    rr.record(f"cpu uks H2O+ sum over states against U-CPKS alpha {functional}", err, bound)
    assert out["converged"] and err <= bound
    assert np.abs(out["xpy"] @ out["xmy"].T - np.eye(ops.size)).max() <= 1e-10
    wd, fd = ued.dense_solution(ops, *ued.dense_matrices(ops), False)
    assert np.abs(w - wd).max() <= 1e-9 and np.abs(out["oscillator_strengths"] - fd).max() <= 1e-6


F0 = 2e-3


def _uks_finite_field(functional):
    cols_f, cols_h = [], []
    for axis in range(3):
        def mu(h):
            F = [0.0, 0.0, 0.0]
            F[axis] = h
            inp, res, _ = uks_state(functional, 1, 1, field=tuple(F))
            return properties.dipole_moment(inp, res["dm"])
        d = lambda h: (mu(h) - mu(-h)) / (2.0 * h)
        cols_f.append(d(F0)); cols_h.append(d(0.5 * F0))
    Df, Dh = np.array(cols_f).T, np.array(cols_h).T
    value = (4.0 * Dh - Df) / 3.0
    return value, float(np.abs(value - Dh).max())


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_cation_ucpks_alpha_against_the_finite_field(functional):
    """The recipe and the bound of tests/test_response_cpu.py: ten times the finite-field bar plus the CPKS residual."""
    inp, res, ub = uks_state(functional, 1, 1)
    out = response.polarizability(inp, res, ub, functional)
    ref, bar = _uks_finite_field(functional)
    err = float(np.abs(out["alpha"] - ref).max())
    resid = 4.0 * max(np.linalg.norm(out["dipole_integrals"][k]) for k in range(3)) * max(out["residual"])
    print(f"alpha H2O+ {functional}: finite-field bar {bar:.2e}  |CPKS - finite field| {err:.2e}  iterations {out['cpks_iterations']}")
    rr.record(f"cpu uks H2O+ U-CPKS alpha against the finite field {functional}", err, 10.0 * bar + resid)
    assert max(out["residual"]) <= 1e-8
    assert err <= 10.0 * bar + resid, (err, bar, resid)
    assert np.all(np.linalg.eigvalsh(0.5 * (out["alpha"] + out["alpha"].T)) > 0.0)


@pytest.mark.parametrize("functional", ["LDA", "B3LYP"])
def test_spin_zero_alpha_is_the_restricted_alpha(functional):
    inp, res, ub = uks_state(functional, 0, 0)
    u = response.polarizability(inp, res, ub, functional)
    rinp, rres, rb = rks_state(functional)
    r = response.polarizability(rinp, rres, rb, functional)
    err = float(np.abs(u["alpha"] - r["alpha"]).max())
    bound = 4.0 * max(np.linalg.norm(r["dipole_integrals"][k]) for k in range(3)) * (max(u["residual"]) + max(r["residual"])) + 1e-8
    print(f"alpha spin 0 {functional}: |UKS - RKS| {err:.2e}  bound {bound:.2e}")
    rr.record(f"cpu uks spin 0 alpha against the restricted alpha {functional}", err, bound)
    # two SCF solutions converged to |dD| 1e-9 each, carried to alpha by |D_k| / gap ~ 10: the 1e-8
    assert err <= bound


def test_hydrogen_atom_runs(tmp_path):
    """nbeta = 0: the beta block is empty, the alpha electron has four virtual orbitals (def2-SVP: 2s1p)."""
    xyz = tmp_path / "H.xyz"
    xyz.write_text("1\nhydrogen atom\nH 0.0 0.0 0.0\n")
    inp = inputs.build(str(xyz), "def2-svp", grid_level=1, verbose=False, spin=1)
    for functional in ("LDA", "B3LYP"):
        be = UksHostBackend(inp, functional)
        res = scf.run_uks(inp, be, functional, **KW)
        ub = response.HostUksResponse(inp, functional, be, be.ao, be.gr)
        assert res["converged"] and res["nbeta"] == 0
        out = ex.excitations(inp, res, ub, functional, nroots=4)
        pol = response.polarizability(inp, res, ub, functional)
        sos = 2.0 * np.einsum("nk,nl,n->kl", out["transition_dipoles"], out["transition_dipoles"], 1.0 / out["energies"])
        print(f"H atom {functional}: w {out['energies']}  alpha {np.diag(pol['alpha'])}")
        assert out["converged"] and out["energies"][0] > 0.0 and out["xpy"].shape == (4, 4)
        assert np.abs(sos - pol["alpha"]).max() <= 1e-8
        assert np.abs(pol["alpha"] - pol["alpha"][0, 0] * np.eye(3)).max() <= 1e-8 and pol["alpha"][0, 0] > 0.0     # an atom


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    inp, res, ub = uks_state("LDA", 1, 1)
    with pytest.raises(ValueError, match="spin-conserving"):
        ex.excitations(inp, res, ub, "LDA", nroots=1, triplet=True)
    with pytest.raises(ValueError, match="22 occupied-virtual pairs"):
        ex.excitations(inp, res, ub, "LDA", nroots=23)
    with pytest.raises(ValueError, match="--quirks 0"):
        ex.excitations(inp, res, _with_quirks(ub), "LDA", nroots=1)
    with pytest.raises(ValueError, match="run_uks result"):
        ex.UksResponseOperators(inp, {"uks": True, "dm": res["dm"]}, ub, "LDA")
    ops = ex.UksResponseOperators(inp, res, ub, "LDA")
    flip = np.ones(ops.size)
    flip[np.argmin(ops.gap_flat)] = -1.0
    bad = _Shifted(ops, flip)
    with pytest.raises(ValueError, match="the unrestricted reference is unstable"):
        ex.solve(bad, nroots=2)
    with pytest.raises(ValueError, match="the unrestricted reference is unstable"):
        ex.solve(bad, nroots=2, tda=True)
    with pytest.raises(ValueError, match="ao_grad is needed"):
        response.HostFxcSpin("GGA", res["dm_a"], res["dm_b"], ub.ao, inp.grids.weights, None)
    with pytest.raises(ValueError, match="uks_response_prepare has not run"):
        response.HostUksResponse(inp, "LDA", ub.scf, ub.ao, ub.gr).uks_excitation_parts(
            np.zeros((7, 1)), np.zeros((1, 7, 1)), np.zeros((7, 1)), np.zeros((1, 7, 1)), False)


def _with_quirks(ub):
    return response.HostUksResponse(ub.inp, ub.functional, ub.scf, ub.ao, ub.gr, quirks=True)


class _Shifted:
    """The operators of `ops` with some gaps negated: an unstable reference, nothing else touched."""
    flat = True

    def __init__(self, ops, sign):
        self.ops, self.size, self.dip_flat, self.builds = ops, ops.size, ops.dip_flat, 0
        self.gap_flat = ops.gap_flat * sign
        self.shift = self.gap_flat - ops.gap_flat

    def apply(self, Z):
        P, Q = self.ops.apply(Z)
        return P + self.shift[None] * Z, Q + self.shift[None] * Z
