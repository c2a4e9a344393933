"""DFT_EvalAOHess / DFT_ComputeXCGradient (csrc/xc_grad.hip) against their host counterparts (gradients.py), which
tests/test_xc_gradient_cpu.py holds against finite differences of the oracle.

* DFT_ComputeXCGradient against xc_gradient_host on the synthetic planes of tests/xc_gradient_reference.py, bound 2e-8 of
  max|G| (the bar tests/test_gpu_triplet.py applies to device against host).  Shapes: (2085, 24) where the sweep would
  go tiny or use a graph; (2085, 114) seven whole column tiles and two columns, a ragged last tile of rows, more tiles
  than workgroups of one round per CU; (1100, 130) nao > 128 (the big density kernel, nine column tiles: three rounds
  of the four waves, the last with one wave); (37, 50) less than three tiles of rows, the last with five; (37, 530) wider
  than the 512-column tile a workgroup stages at once (the chunked K loop).
* The same call twice is bitwise equal; the grid in two slices equals the whole grid to 1e-13 of max|G|; a following
  DFT_ComputeXC and a following DFT_FxcApply are bitwise what they were before the gradient call.
* DFT_EvalAOHess against ao_hessian_host at 1e-12 of the plane maximum.
* HipBackend.xc_gradient (slices, resident and per-slice planes) against the host from the same dm, 2e-8 of max|G|.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle  # noqa: E402
import xc_gradient_reference as xr  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import basis, gradients, grid_gen, inputs, scf  # noqa: E402

ERR_REL = 2e-8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(functional, quirks=1, **opts):
    s = q.DFTSolverWrapper(q.build_library(), functional)
    s.set_option("quirks", quirks)
    for k, v in opts.items():
        s.set_option(k, v)
    return s


class Planes:
    """The inputs of one shape on the device."""

    def __init__(self, dev, ngrid, nao):
        self.host = xr.inputs(ngrid, nao)
        self.ngrid, self.nao, self.dev = ngrid, nao, dev
        self.d_dm, self.d_ao, self.d_gr, self.d_w, self.d_hs = (torch.as_tensor(np.array(a), device=dev) for a in self.host)

    def gradient(self, s, lo=0, hi=None, hess=True):
        hi = self.ngrid if hi is None else hi
        d_out = torch.full((self.nao, 3), 7.0, dtype=torch.float64, device=self.dev)
        gr = self.d_gr[:, lo:hi].contiguous()
        hs = self.d_hs[:, lo:hi].contiguous() if hess else None
        assert s.compute_xc_gradient(hi - lo, self.nao, self.d_dm, self.d_ao[lo:hi], self.d_w[lo:hi], d_out, gr, hs) == 0
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    def host_gradient(self, functional, quirks=True):
        dm, ao, gr, w, hs = self.host
        return gradients.xc_gradient_host(functional, dm, ao, w, gr, hs, quirks)


def _check(label, G, ref, bound=ERR_REL):
    scale = float(np.abs(ref).max())
    err = float(np.abs(G - ref).max())
    print(f"gpu {label}: max|G| {scale:.3e}  err {err / scale:.2e}")
    xr.record("gpu", label, None, err / scale)
    assert np.all(np.isfinite(G)), label
    assert err <= bound * scale, (label, err / scale)


SHAPES = [(2085, 24), (2085, 114), (1100, 130), (37, 50), (37, 530)]


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP", "PBE0", "BLYP"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_matches_the_host(dev, shape, functional):
    p = Planes(dev, *shape)
    G = p.gradient(_solver(functional), hess=functional != "LDA")
    _check(f"DFT_ComputeXCGradient {functional} quirks=1 {shape}", G, p.host_gradient(functional))


@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP"])
def test_gradient_without_quirks(dev, functional):
    p = Planes(dev, 2085, 114)
    G = p.gradient(_solver(functional, 0))
    _check(f"DFT_ComputeXCGradient {functional} quirks=0 (2085, 114)", G, p.host_gradient(functional, False))


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP"])
def test_validation_paths(dev, functional, path):
    p = Planes(dev, 2085, 24)
    G = p.gradient(_solver(functional, 1, path=path))
    _check(f"DFT_ComputeXCGradient {functional} quirks=1 (2085, 24) path={path}", G, p.host_gradient(functional))


@pytest.mark.parametrize("shape", [(2085, 114), (1100, 130)])
def test_a_call_is_bitwise_reproducible_and_slices_add_up(dev, shape):
    p = Planes(dev, *shape)
    s = _solver("B3LYP")
    G = p.gradient(s)
    assert np.array_equal(G, p.gradient(s))
    cut = 16 * 41 + 3      # not a multiple of the row tile: both slices end ragged
    two = p.gradient(s, 0, cut) + p.gradient(s, cut, shape[0])
    err = float(np.abs(two - G).max() / np.abs(G).max())
    print(f"gpu two slices against the whole grid {shape}: {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("functional,shape", [("GGA", (2085, 24)), ("B3LYP", (2085, 114)), ("LDA", (1100, 130))])
def test_the_sweep_and_the_response_table_are_left_as_they_were(dev, functional, shape):
    p = Planes(dev, *shape)
    s = _solver(functional)
    n = p.nao
    gr = p.d_gr if functional != "LDA" else None

    def sweep():
        d_v = torch.zeros((n, n), dtype=torch.float64, device=dev)
        e = s.compute_xc(p.ngrid, n, p.d_dm, p.d_ao, p.d_w, d_v, gr)
        return e, d_v.cpu().numpy()

    def apply():
        d_v = torch.zeros((n, n), dtype=torch.float64, device=dev)
        assert s.fxc_apply(p.ngrid, n, p.d_dm, p.d_ao, d_v, gr) == 0
        torch.cuda.synchronize()
        return d_v.cpu().numpy()

    sweep(); e0, v0 = sweep()          # the second call is the one a graph would be recorded from
    assert s.fxc_prepare(p.ngrid, n, p.d_dm, p.d_ao, p.d_w, gr) == 0
    a0 = apply()
    G = p.gradient(s)
    assert np.all(np.isfinite(G))
    a1 = apply()
    e1, v1 = sweep()
    assert np.array_equal(a0, a1)
    assert e0 == e1 and np.array_equal(v0, v1)


def test_refusals(dev):
    p = Planes(dev, 37, 50)
    d_out = torch.zeros((50, 3), dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="null for a gradient-corrected functional"):
        _solver("GGA").compute_xc_gradient(37, 50, p.d_dm, p.d_ao, p.d_w, d_out, p.d_gr, None)
    with pytest.raises(RuntimeError, match="null for a gradient-corrected functional"):
        _solver("B3LYP").compute_xc_gradient(37, 50, p.d_dm, p.d_ao, p.d_w, d_out, None, p.d_hs)
    with pytest.raises(RuntimeError, match="needs ao_grad"):
        _solver("LDA").compute_xc_gradient(37, 50, p.d_dm, p.d_ao, p.d_w, d_out, None, None)


MOLECULES = {
    "H2O/def2-SVP": ("O 0 0 0.1173; H 0 0.7572 -0.4692; H 0 -0.7572 -0.4692", "def2-svp", 2085),
    "CH4/def2-TZVP": ("C 0 0 0; H 0.629 0.629 0.629; H -0.629 -0.629 0.629; H -0.629 0.629 -0.629; H 0.629 -0.629 -0.629",
                      "def2-tzvp", 2085),
    # 141 columns: two column blocks of the AO kernels (at most 126 each)
    "C3H8/def2-TZVP": ("C 0 0 0.587; C 0 1.266 -0.260; C 0 -1.266 -0.260; H 0.876 0 1.242; H -0.876 0 1.242; H 0 2.166 0.362; "
                       "H 0.883 1.306 -0.905; H -0.883 1.306 -0.905; H 0 -2.166 0.362; H 0.883 -1.306 -0.905; H -0.883 -1.306 -0.905",
                       "def2-tzvp", 333),
}


@pytest.mark.parametrize("name", list(MOLECULES))
def test_ao_hessian_matches_the_host(dev, name):
    geom, bname, npts = MOLECULES[name]
    syms, xyz = basis.parse_xyz(geom)
    sh = basis.build_shells(syms, xyz, bname)
    coords = np.asarray(grid_gen.Grids(syms, xyz, level=1).coords)
    coords = np.ascontiguousarray(coords[::max(1, len(coords) // npts)][:npts])      # near and far points of every atom
    assert len(coords) == npts and npts % 16 != 0
    assert (sh.nao > 126) == name.startswith("C3H8")
    d_c = torch.as_tensor(coords, device=dev)
    d_h = torch.full((6, npts, sh.nao), 7.0, dtype=torch.float64, device=dev)
    s = _solver("GGA")
    assert s.eval_ao_hess(sh, d_c, npts, d_h) == 0
    torch.cuda.synchronize()
    got, ref = d_h.cpu().numpy(), gradients.ao_hessian_host(sh, coords)
    for k in range(6):
        scale = float(np.abs(ref[k]).max())
        err = float(np.abs(got[k] - ref[k]).max())
        print(f"gpu DFT_EvalAOHess {name} plane {'xx xy xz yy yz zz'.split()[k]}: max {scale:.3e}  err {err / scale:.2e}")
        xr.record("gpu", f"DFT_EvalAOHess {name} plane {k}", None, err / scale, "plane max")
        assert err <= 1e-12 * scale, (name, k, err / scale)


@pytest.fixture(scope="module")
def water():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    inp = inputs.build("H2O", "def2-svp", 1, verbose=False)
    be = scf.HipBackend(inp, "B3LYP")
    res = scf.run_scf(inp, be, "B3LYP", log=None, conv_e=1e-10)
    assert res["converged"]
    ao, gr = oracle.eval_ao(inp.shells, inp.grids.coords, deriv=1)
    return inp, be, np.ascontiguousarray(res["dm"]), ao, gr, gradients.ao_hessian_host(inp.shells, inp.grids.coords)


@pytest.mark.parametrize("slice_rows", [None, 3000])
def test_backend_gradient_b3lyp(water, slice_rows):
    """The resident planes, whole (None) and in slices of 3000 rows (the gradient planes of a slice copied together)."""
    inp, be, dm, ao, gr, hs = water
    G = be.xc_gradient(dm, slice_rows=slice_rows)
    ref = gradients.xc_gradient_host("B3LYP", dm, ao, inp.grids.weights, gr, hs, True)
    _check(f"HipBackend.xc_gradient H2O/def2-SVP B3LYP slice_rows={slice_rows}", G, ref)
    g = gradients.sum_over_atoms(inp.shells, G)
    assert g.shape == (3, 3) and np.abs(g - gradients.sum_over_atoms(inp.shells, ref)).max() <= ERR_REL * np.abs(ref).max() * inp.shells.nao


def test_backend_gradient_lda_evaluates_its_own_gradient_planes(water):
    inp, _, dm, ao, gr, _ = water
    be = scf.HipBackend(inp, "LDA", quirks=False)
    assert be.d_gr is None
    G = be.xc_gradient(dm, slice_rows=4096)
    _check("HipBackend.xc_gradient H2O/def2-SVP LDA quirks=0 slice_rows=4096", G,
           gradients.xc_gradient_host("LDA", dm, ao, inp.grids.weights, gr, None, False))


def test_backend_refuses_dm_factor(water):
    inp, _, dm, _, _, _ = water
    be = scf.HipBackend(inp, "LDA", xc_occ=False, dm_factor=True)
    with pytest.raises(ValueError, match="without dm_factor"):
        be.xc_gradient(dm)


@pytest.mark.parametrize("eri_mode", ["dense", "cholesky"])
def test_nuclear_gradient_on_the_device(eri_mode):
    """gradients.nuclear_gradient on HipBackend (XC part by DFT_ComputeXCGradient, Fock parts from the device) against the
    host assembly (oracle Fock parts from the dense ERI, xc_gradient_host) from the same converged dm: 2e-8 of max|g|.
    Cholesky vectors to 1e-10, so that their share of W stays below the bound."""
    from scf_oracle_backend import OracleBackend
    dense = inputs.build("H2O", "def2-svp", 1, verbose=False)
    inp = dense if eri_mode == "dense" else inputs.build("H2O", "def2-svp", 1, verbose=False, eri_mode="cholesky", chol_tol=1e-10)
    be = scf.HipBackend(inp, "B3LYP")
    res = scf.run_scf(inp, be, "B3LYP", log=None, conv_e=1e-10)
    assert res["converged"]
    g, terms = gradients.nuclear_gradient(inp, res, be)
    ref, ref_terms = gradients.nuclear_gradient(dense, {"dm": res["dm"]}, OracleBackend(dense, "B3LYP"), "B3LYP", quirks=True)
    scale = float(np.abs(ref).max())
    for k in ref_terms:
        print(f"gpu nuclear_gradient H2O/def2-SVP B3LYP {eri_mode} {k}: {np.abs(terms[k] - ref_terms[k]).max() / scale:.2e}")
    _check(f"nuclear_gradient H2O/def2-SVP B3LYP {eri_mode}", g, ref)
    assert g.shape == (3, 3) and np.abs(g.sum(axis=0)).max() < 1e-3      # grid level 1: the fixed quadrature's net force
