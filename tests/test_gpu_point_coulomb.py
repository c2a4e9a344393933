"""One-electron Coulomb integrals at points ON THE DEVICE (csrc/point_coulomb.hip through integrals.PointCoulomb) against
the stored 100-digit reference and the host engine, and the embedded SCF through the device loops."""
import ctypes

import numpy as np
import pytest

import point_coulomb_fixtures as F
from quantum_compute_dft_amd import basis, inputs, integrals, properties, scf

pytestmark = pytest.mark.gpu
BOUND = F.BOUND
CHARGES = np.array([[3.0, 0.5, -1.0, -0.8], [-2.5, 2.0, 1.5, 0.4]])      # bohr, e: the set-up of the CPU Hellmann-Feynman tests


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
def test_matrix_of_a_unit_charge_matches_the_reference_at_every_stored_point(dev, engines, name):
    import torch
    f, pc = F.family(name), engines[name]
    n = f["sh"].nao
    worst = {}
    for c, (r, A) in enumerate(zip(f["points"], f["A"])):
        out = torch.full((n, n), 777.0, dtype=torch.float64, device=dev)           # sentinel: every element must be written
        M = pc.matrix(_t(r[None, :], dev), torch.ones(1, dtype=torch.float64, device=dev), out=out).cpu().numpy()
        allowed = BOUND * max(1.0, np.abs(A).max())
        for k, e in F.class_errors(M, A, f["sh"]).items():
            worst[k] = max(worst.get(k, 0.0), e)
        assert np.abs(M - A).max() <= allowed, (name, c, r, np.abs(M - A).max(), allowed)
        assert np.array_equal(M, M.T), (name, c)
    print(f"\n{name}: worst |M - A| per class (la, lb) over the {len(f['points'])} stored points (bound {BOUND:g} x max(1, max|A|)):")
    for (la, lb), e in sorted(worst.items()):
        print(f"  ({'spdf'[la]}{'spdf'[lb]})  {e:.2e}")


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_matrix_of_all_stored_points_with_weights_of_both_signs(dev, engines, name):
    f, pc = F.family(name), engines[name]
    w = np.random.default_rng(7).uniform(-2.0, 2.0, len(f["points"]))
    assert (w > 0).any() and (w < 0).any()
    ref = np.einsum("c,cij->ij", w, f["A"])
    allowed = BOUND * max(1.0, float(np.sum(np.abs(w) * np.abs(f["A"]).max(axis=(1, 2)))))
    M1 = pc.matrix(_t(f["points"], dev), _t(w, dev)).cpu().numpy()
    M2 = pc.matrix(_t(f["points"], dev), _t(w, dev)).cpu().numpy()
    print(f"\n{name}: |M - sum w A| = {np.abs(M1 - ref).max():.2e} (allowed {allowed:.2e})")
    assert np.abs(M1 - ref).max() <= allowed
    assert np.array_equal(M1, M1.T) and np.array_equal(M1, M2)


@pytest.mark.parametrize("name", ["z1", "z3"])
def test_contraction_for_a_full_and_ten_class_masked_matrices_at_every_batch_size(dev, engines, name):
    f, pc = F.family(name), engines[name]
    P = len(f["points"])
    for label, D in F.densities(f["sh"]):
        ref, allowed = F.contract_reference(D, f["A"])
        d_D = _t(D, dev)
        worst = 0.0
        for n in (1, 63, 64, 65, P):
            idx = (np.arange(n) * 5 + 3) % P                  # the stored points, repeated to fill the batch (5 is coprime to P)
            pts = _t(f["points"][idx], dev)
            u1 = pc.contract(pts, d_D).cpu().numpy()
            u2 = pc.contract(pts, d_D).cpu().numpy()
            err = np.abs(u1 - ref[idx])
            worst = max(worst, float((err / allowed[idx]).max()))
            assert (err <= allowed[idx]).all(), (name, label, n, err.max())
            assert np.array_equal(u1, u2), (name, label, n)
        print(f"{name} {label}: worst error / allowed = {worst:.2e}")


def test_device_against_the_host_engine_on_benzene_def2_svp(dev):
    import os
    shells = basis.build_shells(*basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz")), "def2-svp")
    _, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
    assert shells.nao == 114
    rng = np.random.default_rng(300)
    pts = np.empty((0, 3))
    while len(pts) < 300:
        cand = rng.uniform(-10.0, 10.0, (400, 3)) + xyz.mean(axis=0)
        pts = np.concatenate([pts, cand[np.linalg.norm(cand[:, None] - xyz[None], axis=2).min(axis=1) >= 0.1]])[:300]
    w = rng.uniform(-1.0, 1.0, 300)
    D = rng.standard_normal((114, 114))
    # per-point host matrices: the reference's own size for the two bounds
    A = np.array([integrals.point_coulomb_matrix(shells, p[None, :], np.ones(1)) for p in pts])
    M_ref, u_ref = integrals.point_coulomb_matrix(shells, pts, w), integrals.point_coulomb_contract(shells, pts, D)
    pc = integrals.PointCoulomb(shells)
    M = pc.matrix(_t(pts, dev), _t(w, dev)).cpu().numpy()
    u = pc.contract(_t(pts, dev), _t(D, dev)).cpu().numpy()
    pc.close()
    allowed_M = BOUND * max(1.0, float(np.sum(np.abs(w) * np.abs(A).max(axis=(1, 2)))))
    allowed_u = BOUND * np.maximum(1.0, np.einsum("ij,cij->c", np.abs(D), np.abs(A)))
    print(f"\nBenzene/def2-SVP, 300 points: |M - host| = {np.abs(M - M_ref).max():.2e} (allowed {allowed_M:.2e}), "
          f"worst contract error / allowed = {(np.abs(u - u_ref) / allowed_u).max():.2e}")
    assert np.abs(M - M_ref).max() <= allowed_M and np.array_equal(M, M.T)
    assert (np.abs(u - u_ref) <= allowed_u).all()
    # the dispatcher takes the same kernels
    assert np.array_equal(integrals.point_coulomb(shells, pts, weights=w, device=dev), M)
    assert np.array_equal(integrals.point_coulomb(shells, pts, dm=D, device=dev), u)


def test_no_points_and_error_returns(dev, engines):
    import torch
    f, pc = F.family("z1"), engines["z1"]
    n = f["sh"].nao
    empty = torch.empty((0, 3), dtype=torch.float64, device=dev)
    out = torch.full((n, n), 777.0, dtype=torch.float64, device=dev)
    assert float(pc.matrix(empty, torch.empty(0, dtype=torch.float64, device=dev), out=out).abs().max()) == 0.0
    assert pc.contract(empty, _t(np.eye(n), dev)).shape == (0,)
    L = pc.lib                                         # the engine's ctypes handle: argument types are set
    assert L.DFT_GetVersion() == 5
    # null output pointer, negative count: -1 and a message, nothing launched
    one, w1 = _t(f["points"][:1], dev), torch.ones(1, dtype=torch.float64, device=dev)
    u64 = ctypes.c_uint64
    assert L.DFT_PointCoulombMatrix(pc._h, 1, u64(one.data_ptr()), u64(w1.data_ptr()), u64(0)) == -1
    assert b"null pointer" in L.DFT_PointCoulombLastError(pc._h)
    assert L.DFT_PointCoulombContract(pc._h, 1, u64(one.data_ptr()), u64(out.data_ptr()), u64(0)) == -1
    assert L.DFT_PointCoulombMatrix(pc._h, -1, u64(one.data_ptr()), u64(w1.data_ptr()), u64(out.data_ptr())) == -1
    # a g shell: no handle, and the entries refuse the null handle
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    xyz, ex, cf = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 1)(1.0), (ctypes.c_double * 1)(1.0)
    l4, one_i, zero_i = (ctypes.c_int * 1)(4), (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0)
    h = L.DFT_PointCoulombOpen(1, xyz, l4, one_i, zero_i, zero_i, ex, cf, 9, 1)
    assert not h
    assert L.DFT_PointCoulombMatrix(None, 1, u64(one.data_ptr()), u64(w1.data_ptr()), u64(out.data_ptr())) == -1
    assert L.DFT_PointCoulombContract(None, 1, u64(one.data_ptr()), u64(out.data_ptr()), u64(out.data_ptr())) == -1
    assert L.DFT_PointCoulombLastError(None) == b"null handle"
    torch.cuda.synchronize()


def test_embedded_scf_matches_the_oracle_driven_scf(dev):
    """H2O / STO-3G in the field of two charges, whole device path (V_ext from the device kernels too) against the CPU
    oracle loop: thresholds and bounds of test_gpu_parity.test_full_scf_matches_the_oracle_driven_scf."""
    from scf_oracle_backend import OracleBackend
    inp_d = inputs.build("H2O", "sto-3g", 1, device=dev, verbose=False, point_charges=CHARGES)
    inp_h = inputs.build("H2O", "sto-3g", 1, verbose=False, point_charges=CHARGES)
    assert np.abs(inp_d.Hcore - inp_h.Hcore).max() <= BOUND and inp_d.E_nuc == inp_h.E_nuc
    kw = dict(log=None, conv_e=1e-11, conv_dm=1e-9)
    r_gpu = scf.run_scf(inp_d, scf.HipBackend(inp_d, "B3LYP"), "B3LYP", **kw)
    r_cpu = scf.run_scf(inp_h, OracleBackend(inp_h, "B3LYP"), "B3LYP", **kw)
    assert r_gpu["converged"] and r_cpu["converged"]
    assert r_gpu["E_tot"] == pytest.approx(r_cpu["E_tot"], abs=1e-9)
    assert r_gpu["E_xc"] == pytest.approx(r_cpu["E_xc"], abs=1e-9)
    assert np.abs(r_gpu["dm"] - r_cpu["dm"]).max() < 1e-7
    bare = inputs.build("H2O", "sto-3g", 1, verbose=False)
    assert abs(scf.run_scf(bare, scf.HipBackend(bare, "B3LYP"), "B3LYP", **kw)["E_tot"] - r_gpu["E_tot"]) > 1e-4      # the charges are felt


def test_energy_derivative_in_a_charge_is_the_device_potential_at_its_site(dev):
    """Hellmann-Feynman on the device: B3LYP, h = 1e-2 (truncation 7.0e-9 measured on the host), the driver's default loop,
    the ESP from the device kernel.  1e-7 leaves room for 1e-9 of SCF energy noise divided by 2h."""
    h = 1e-2
    kw = dict(log=None, conv_e=1e-11, conv_dm=1e-9)
    def run(q):
        inp = inputs.build("H2O", "sto-3g", 1, device=dev, verbose=False, point_charges=q)
        return inp, scf.run_scf(inp, scf.HipBackend(inp, "B3LYP", quirks=False), "B3LYP", **kw)
    dq = np.zeros_like(CHARGES)
    dq[0, 3] = h
    (_, rp), (_, rm), (inp, r0) = run(CHARGES + dq), run(CHARGES - dq), run(CHARGES)
    assert rp["converged"] and rm["converged"] and r0["converged"]
    esp = properties.electrostatic_potential(inp, r0["dm"], CHARGES[:1, :3], device=dev)[0]
    esp_host = properties.electrostatic_potential(inp, r0["dm"], CHARGES[:1, :3])[0]
    dE = (rp["E_tot"] - rm["E_tot"]) / (2 * h)
    print(f"\ndE/dq = {dE:.12f}, device ESP = {esp:.12f} (host {esp_host:.12f}), difference {abs(dE - esp):.2e}")
    assert abs(esp - esp_host) <= BOUND
    assert abs(dE - esp) <= 1e-7


def test_fused_loop_with_point_charges_matches_the_host_loop(dev):
    """Embedding reaches the device tail through Hcore: bound of test_gpu_scf_tail.test_fused_loop_matches_the_host_loop."""
    inp = inputs.build("Benzene", "sto-3g", 1, device=dev, verbose=False, point_charges=CHARGES + np.array([2.0, 3.0, 1.0, 0.0]))
    host = scf.HipBackend(inp, "GGA", device=dev, device_resident=False, fused_tail=False)
    assert host.tail is None
    r_host = scf.run_scf(inp, host, "GGA", log=None)
    fused = scf.HipBackend(inp, "GGA", device=dev, fused_tail=True)
    assert fused.tail is not None
    r_fused = scf.run_scf(inp, fused, "GGA", log=None)
    assert r_host["converged"] and r_fused["converged"] and r_fused["loop"] == "fused"
    print(f"\nfused {r_fused['E_tot']:.10f} host {r_host['E_tot']:.10f}")
    assert abs(r_host["E_tot"] - r_fused["E_tot"]) <= 2e-8, (r_host["E_tot"], r_fused["E_tot"])
    assert np.abs(r_host["dm"] - r_fused["dm"]).max() <= 1e-5
