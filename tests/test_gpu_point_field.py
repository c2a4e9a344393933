"""The field of a density at points ON THE DEVICE (csrc/point_coulomb.hip: k_pc_field through integrals.PointCoulomb.field)
against the stored 100-digit reference and the host engine, and the forces on the charges of an embedded run."""
import ctypes
import os

import numpy as np
import pytest

import point_field_fixtures as F
from quantum_compute_dft_amd import basis, inputs, integrals, properties, scf

pytestmark = pytest.mark.gpu
BOUND = F.BOUND
CHARGES = np.array([[3.0, 0.5, -1.0, -0.8], [-2.5, 2.0, 1.5, 0.4]])      # bohr, e: the set-up of test_gpu_point_coulomb.py


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engines(dev):
    made = {name: integrals.PointCoulomb(F.family(name)["sh"]) for name in ("z1", "z3")}
    yield made
    for pc in made.values():
        pc.close()


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_field_for_a_full_and_ten_class_masked_matrices_at_every_batch_size(dev, engines, name):
    """Per point and component BOUND * max(1, sum |D| |dA[c, k]|).  256 is the workgroup size: 257 points take a second
    workgroup.  Every element of a sentinel-filled `out` is overwritten and two calls give the same bits.  The table of
    error / allowed per class is printed (profiles/point_field_parity.txt)."""
    import torch
    f, pc = F.family(name), engines[name]
    P = len(f["points"])
    table = {}
    for label, D, ref, allowed in F.references(name):
        d_D = _t(D, dev)
        worst = 0.0
        for n in (1, 63, 64, 65, 255, 256, 257, P):
            idx = (np.arange(n) * 5 + 3) % P                  # the stored points, repeated to fill the batch (5 is coprime to P)
            pts = _t(f["points"][idx], dev)
            out = torch.full((n, 3), 777.0, dtype=torch.float64, device=dev)
            res = pc.field(pts, d_D, out=out)
            assert res.data_ptr() == out.data_ptr()
            g1 = res.cpu().numpy()
            g2 = pc.field(pts, d_D).cpu().numpy()
            assert g1.shape == (n, 3) and not (g1 == 777.0).any(), (name, label, n)
            err = np.abs(g1 - ref[idx])
            worst = max(worst, float((err / allowed[idx]).max()))
            assert (err <= allowed[idx]).all(), (name, label, n, (err / allowed[idx]).max())
            assert np.array_equal(g1, g2), (name, label, n)
        table[label] = worst
    print(f"\n{name}, device: worst |G - reference| / allowed over the batch sizes (allowed = {BOUND:g} x max(1, sum |D| |dA[c, k]|)):")
    for label, w in table.items():
        print(f"  {label:10s} {w:.2e}")


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_derivative_of_a_unit_charge_matches_the_reference_per_class(dev, engines, name):
    """dA[c, k, mu, nu] out of the device contraction with D = e_mu e_nu^T: per element BOUND * max(1, max|dA[c, k]|), the
    host test's bound, and the same table per class (la, lb)."""
    f, pc = F.family(name), engines[name]
    pts = _t(f["points"], dev)
    got = F.unit_matrix_from_contractions(lambda D: pc.field(pts, _t(D, dev)).cpu().numpy(), f["sh"])
    allowed = BOUND * np.maximum(1.0, np.abs(f["dA"]).max(axis=(2, 3)))[:, :, None, None]
    ratio = np.abs(got - f["dA"]) / allowed
    F.print_class_table(f"{name}, device: worst |dA - reference| / allowed per class over the {len(f['points'])} stored points "
                        f"(allowed = {BOUND:g} x max(1, max|dA[c, k]|))", F.class_ratios(ratio, f["sh"]))
    assert ratio.max() <= 1.0, (name, np.unravel_index(np.argmax(ratio), ratio.shape))


def test_device_against_the_host_engine_on_benzene_def2_svp(dev):
    shells = basis.build_shells(*basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz")), "def2-svp")
    _, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
    assert shells.nao == 114
    rng = np.random.default_rng(300)                          # the point set of test_gpu_point_coulomb.py
    pts = np.empty((0, 3))
    while len(pts) < 300:
        cand = rng.uniform(-10.0, 10.0, (400, 3)) + xyz.mean(axis=0)
        pts = np.concatenate([pts, cand[np.linalg.norm(cand[:, None] - xyz[None], axis=2).min(axis=1) >= 0.1]])[:300]
    rng.uniform(-1.0, 1.0, 300)
    D = rng.standard_normal((114, 114))
    G_ref = integrals.point_coulomb_field(shells, pts, D)
    # the host's own size per point and component: sum |D| |dA[c, k]| from the host's derivative integrals
    scale = np.array([np.einsum("ij,kij->k", np.abs(D), np.abs(integrals.point_coulomb_field_matrix(shells, p[None, :], np.ones(1)))) for p in pts])
    pc = integrals.PointCoulomb(shells)
    G = pc.field(_t(pts, dev), _t(D, dev)).cpu().numpy()
    pc.close()
    allowed = BOUND * np.maximum(1.0, scale)
    print(f"\nBenzene/def2-SVP, 300 points: max |G| = {np.abs(G_ref).max():.3e}, worst |device - host| / allowed = {(np.abs(G - G_ref) / allowed).max():.2e}")
    assert (np.abs(G - G_ref) <= allowed).all()
    assert np.array_equal(integrals.point_field(shells, pts, D, device=dev), G)       # the dispatcher takes the same kernel


def test_no_points_and_error_returns(dev, engines):
    import torch
    f, pc = F.family("z1"), engines["z1"]
    n = f["sh"].nao
    empty = torch.empty((0, 3), dtype=torch.float64, device=dev)
    assert pc.field(empty, _t(np.eye(n), dev)).shape == (0, 3)
    L = pc.lib                                         # the engine's ctypes handle: argument types are set
    assert L.DFT_GetVersion() == 5                     # the entry was added without a version change
    one, dm = _t(f["points"][:1], dev), _t(np.eye(n), dev)
    out = torch.full((1, 3), 777.0, dtype=torch.float64, device=dev)
    u64 = ctypes.c_uint64
    # null output pointer, negative count: -1 and a message, nothing launched
    assert L.DFT_PointCoulombField(pc._h, 1, u64(one.data_ptr()), u64(dm.data_ptr()), u64(0)) == -1
    assert b"DFT_PointCoulombField" in L.DFT_PointCoulombLastError(pc._h) and b"null pointer" in L.DFT_PointCoulombLastError(pc._h)
    assert L.DFT_PointCoulombField(pc._h, -1, u64(one.data_ptr()), u64(dm.data_ptr()), u64(out.data_ptr())) == -1
    assert b"negative point count" in L.DFT_PointCoulombLastError(pc._h)
    assert L.DFT_PointCoulombField(None, 1, u64(one.data_ptr()), u64(dm.data_ptr()), u64(out.data_ptr())) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == 777.0                   # none of the refused calls wrote
    assert L.DFT_PointCoulombField(pc._h, 1, u64(one.data_ptr()), u64(dm.data_ptr()), u64(out.data_ptr())) == 0
    assert L.DFT_PointCoulombLastError(pc._h) == b""
    torch.cuda.synchronize()
    assert not (out == 777.0).any().item()


def test_forces_on_the_charges_of_an_embedded_run_match_the_host(dev):
    """H2O / STO-3G, B3LYP, in the field of two charges through the device loops (the run of
    test_gpu_point_coulomb.test_embedded_scf_matches_the_oracle_driven_scf): the forces from the device kernel against the
    host engine on the same density, BOUND * max(1, |F|)."""
    inp = inputs.build("H2O", "sto-3g", 1, device=dev, verbose=False, point_charges=CHARGES)
    res = scf.run_scf(inp, scf.HipBackend(inp, "B3LYP"), "B3LYP", log=None, conv_e=1e-11, conv_dm=1e-9)
    assert res["converged"]
    F_dev = properties.point_charge_forces(inp, res["dm"], device=dev)
    F_host = properties.point_charge_forces(inp, res["dm"])
    print(f"\nforces on the charges (Ha/bohr), device:\n{F_dev}\n|device - host| = {np.abs(F_dev - F_host).max():.2e}")
    assert F_dev.shape == (2, 3) and np.abs(F_host).max() > 1e-3
    assert (np.abs(F_dev - F_host) <= BOUND * np.maximum(1.0, np.abs(F_host))).all()
