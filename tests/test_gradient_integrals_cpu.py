"""Derivative integrals of the nuclear gradient (csrc/integrals.c: qc_grad1e, qc_grad2e) at fixed random symmetric D and W,
against finite differences of tr(D (T + V)), tr(W S) and 1/2 D D (ab|cd) - c_hf/4 D D (ab|cd) from integrals.int1e / int2e
at displaced geometries.  The displacement runs along one random unit direction d of the 3 natm space, so the reference is
the projection sum_A d_A . g_A: central differences at h and 2 h, Richardson-extrapolated, bar = |D_R - D(h)|, and

    |analytic - D_R| <= max(10 bar, 1e-9 scale),     10 bar <= 1e-6 scale.

scale = |D_R| itself, never larger than sqrt(3 natm) times the largest gradient component and taken from the reference
alone.  h = 1e-4 bohr: the tightest functions that carry weight in a random D leave a t^2 term of 1e-9 .. 3e-8 of the
projection (measured: profiles/gradient_parity.txt), the rounding of the quotient ~1e-10.
"""
import numpy as np
import pytest

import xc_gradient_reference as xr
from quantum_compute_dft_amd import basis, inputs, integrals, properties

H = 1e-4
MOLECULES = {
    "H2O/def2-SVP": ("O 0 0 0.1173; H 0 0.7572 -0.4692; H 0 -0.7572 -0.4692", "def2-svp"),          # d shells
    "CH4/def2-TZVP": ("C 0 0 0; H 0.629 0.629 0.629; H -0.629 -0.629 0.629; H -0.629 0.629 -0.629; H 0.629 -0.629 -0.629",
                      "def2-tzvp"),                                                                   # f shells, 55 functions
}
CHARGES = np.array([[2.1, -1.3, 0.8, 0.45], [-2.6, 0.9, -1.7, -0.6]])


def _setup(name):
    geom, bname = MOLECULES[name]
    syms, xyz = basis.parse_xyz(geom)
    sh = basis.build_shells(syms, xyz, bname)
    rng = np.random.default_rng(7)
    a, b = rng.standard_normal((sh.nao, sh.nao)), rng.standard_normal((sh.nao, sh.nao))
    d = rng.standard_normal(xyz.shape)
    return syms, xyz, bname, sh, 0.1 * (a + a.T), 0.1 * (b + b.T), d / np.linalg.norm(d)


def _check(label, analytic, energy):
    D = {h: (energy(h) - energy(-h)) / (2.0 * h) for h in (H, 2.0 * H)}
    ref = (4.0 * D[H] - D[2.0 * H]) / 3.0
    bar, err, scale = abs(ref - D[H]), abs(analytic - ref), abs(ref)
    print(f"cpu {label}: D_R {ref:+.6e}  bar {bar / scale:.2e}  err {err / scale:.2e}")
    xr.record("cpu", label, bar / scale, err / scale, "|D_R|")
    assert 10.0 * bar <= 1e-6 * scale, (label, bar / scale)
    assert err <= max(10.0 * bar, 1e-9 * scale), (label, err / scale, bar / scale)


@pytest.mark.parametrize("embedded", [False, True])
@pytest.mark.parametrize("name", list(MOLECULES))
def test_one_electron_terms(name, embedded):
    syms, xyz, bname, sh, Dm, W, d = _setup(name)
    z = np.array([basis.atomic_number(s) for s in syms], dtype=np.float64)
    g = integrals.grad1e(sh, xyz, z, Dm, W)
    field = integrals.point_coulomb_field(sh, xyz, Dm)
    parts = {"-tr(W dS)": g[0], "tr(D dT)": g[1], "tr(D dV)": g[2] - z[:, None] * field}
    if embedded:
        parts["tr(D dV_ext)"] = integrals.grad1e(sh, CHARGES[:, :3], CHARGES[:, 3], Dm, W)[2]

    def shells_at(t):
        x = xyz + t * d
        return basis.build_shells(syms, x, bname), x

    def e_s(t):
        s, x = shells_at(t)
        return -float(np.sum(W * integrals.int1e(s, syms, x)[0]))

    def e_t(t):
        s, x = shells_at(t)
        return float(np.sum(Dm * integrals.int1e(s, syms, x)[1]))

    def e_v(t):
        s, x = shells_at(t)
        return float(np.sum(Dm * integrals.int1e(s, syms, x)[2]))

    def e_ext(t):
        s, x = shells_at(t)
        return float(np.sum(Dm * inputs.external_charges(syms, x, s, CHARGES)[1]))

    energies = {"-tr(W dS)": e_s, "tr(D dT)": e_t, "tr(D dV)": e_v, "tr(D dV_ext)": e_ext}
    for key, part in parts.items():
        if embedded and key != "tr(D dV_ext)":
            continue      # the other three do not know of the charges: held in the plain case
        _check(f"{key} {name}", float(np.sum(part * d)), energies[key])


@pytest.mark.parametrize("c_hf", [0.0, 0.25])
@pytest.mark.parametrize("name", list(MOLECULES))
def test_two_electron_term(name, c_hf):
    syms, xyz, bname, sh, Dm, _, d = _setup(name)
    g = integrals.grad2e(sh, Dm, c_hf)

    def e2(t):
        eri = integrals.int2e(basis.build_shells(syms, xyz + t * d, bname))
        J = np.einsum("ijkl,kl->ij", eri, Dm)
        e = 0.5 * float(np.sum(Dm * J))
        if c_hf:
            e -= 0.25 * c_hf * float(np.sum(Dm * np.einsum("ikjl,kl->ij", eri, Dm)))
        return e

    _check(f"two-electron c_hf={c_hf} {name}", float(np.sum(g * d)), e2)


@pytest.mark.parametrize("name", list(MOLECULES))
def test_translational_invariance(name):
    """Every integral term sums to zero over the atoms, to 1e-10 of its largest component; with charges present the
    derivative by the charges' positions (minus the electronic part of properties.point_charge_forces) joins the sum."""
    syms, xyz, bname, sh, Dm, W, _ = _setup(name)
    z = np.array([basis.atomic_number(s) for s in syms], dtype=np.float64)
    g = integrals.grad1e(sh, xyz, z, Dm, W)
    v = g[2] - z[:, None] * integrals.point_coulomb_field(sh, xyz, Dm)
    for label, part in (("S", g[0]), ("T", g[1]), ("V", v), ("2e c_hf=0", integrals.grad2e(sh, Dm, 0.0)),
                        ("2e c_hf=0.25", integrals.grad2e(sh, Dm, 0.25))):
        scale = float(np.abs(part).max())
        print(f"cpu sum over atoms {label} {name}: {np.abs(part.sum(axis=0)).max() / scale:.2e}")
        assert np.abs(part.sum(axis=0)).max() <= 1e-10 * scale, label
    ext = integrals.grad1e(sh, CHARGES[:, :3], CHARGES[:, 3], Dm, W)[2]
    # d/dR_c of tr(D V_ext) = -q_c sum D d<1/|r - R_c|>/dR_c: the electronic part of the force on the charge, reversed
    on_charges = -CHARGES[:, 3:4] * integrals.point_coulomb_field(sh, CHARGES[:, :3], Dm)
    total = ext.sum(axis=0) + on_charges.sum(axis=0)
    scale = max(float(np.abs(ext).max()), float(np.abs(on_charges).max()))
    print(f"cpu sum over atoms and charges V_ext {name}: {np.abs(total).max() / scale:.2e}")
    assert np.abs(total).max() <= 1e-10 * scale


def test_the_force_on_a_charge_is_the_one_properties_reports():
    """The sign convention of the sum above, against the public routine: F_c = q_c (field of the nuclei + G_c)."""
    syms, xyz, bname, sh, Dm, _, _ = _setup("H2O/def2-SVP")
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False, point_charges=CHARGES)
    F = properties.point_charge_forces(inp, Dm)
    z = np.array([basis.atomic_number(s) for s in inp.symbols], dtype=np.float64)
    dd = CHARGES[:, None, :3] - inp.atom_xyz[None, :, :]
    nuc = (z[None, :, None] * dd / np.linalg.norm(dd, axis=2)[:, :, None] ** 3).sum(axis=1)
    G = integrals.point_coulomb_field(inp.shells, CHARGES[:, :3], Dm)
    assert np.allclose(F, CHARGES[:, 3:4] * (nuc + G), rtol=1e-12, atol=1e-14)


def test_refusals():
    syms, xyz, bname, sh, Dm, W, _ = _setup("H2O/def2-SVP")
    a = Dm.copy(); a[0, 1] += 1.0
    with pytest.raises(ValueError, match="symmetric"):
        integrals.grad2e(sh, a)
    with pytest.raises(ValueError, match="one charge per centre"):
        integrals.grad1e(sh, xyz, np.ones(2), Dm, W)
