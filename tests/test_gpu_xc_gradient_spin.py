"""DFT_ComputeXCGradientSpin (csrc/dft_api.hip, csrc/xc_grad.hip) against its host counterpart
gradients.xc_gradient_spin_host, which tests/test_xc_gradient_spin_cpu.py holds against finite differences of the
open-shell energy.

* Device against host at 2e-8 of max|G| (the ERR_REL of tests/test_gpu_xc_gradient.py) on that file's shapes -- (2085, 24),
  (2085, 114), (1100, 130), (37, 50), (37, 530): the last is wider than the K chunk a workgroup stages at once -- and the
  fully polarised (2085, 50) with three alpha and no beta electrons; and (37, 330), padded to 336: the smallest width at
  which the plan of two spins in one kernel chunks K (320 + 16) while the plan of one spin does not.  LDA, GGA, B3LYP,
  PBE0, BLYP, all at quirks 0; `path` 1 and 2.
* k_xc_grad on both spins in one launch (the default) against k_xc_grad once per spin (option xcg_spin_fused = 0) at 1e-13
  of max|G|, every shape and functional above.
* The closed-shell limit dm_a = dm_b = dm/2 against DFT_ComputeXCGradient at quirks 0.
* The same call twice is bitwise equal; two grid slices add up to the whole to 1e-13 of max|G|.
* DFT_ComputeXC, DFT_ComputeXCSpin and the table of DFT_FxcPrepareSpinPol are bit for bit what they were before the call.
* HipBackend.xc_gradient_spin (whole grid and slices) against the host.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import spin_reference as sr  # noqa: E402
import xc_gradient_reference as xr  # noqa: E402
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import gradients  # noqa: E402

ERR_REL = 2e-8
FUNCTIONALS = ["LDA", "GGA", "B3LYP", "PBE0", "BLYP"]
# (ngrid, nao, nalpha, nbeta)
SHAPES = [(2085, 24, 5, 4), (2085, 114, 21, 19), (1100, 130, 12, 9), (37, 50, 6, 5), (37, 530, 40, 38), (2085, 50, 3, 0),
          (37, 330, 20, 18)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _solver(functional, **opts):
    s = q.DFTSolverWrapper(q.build_library(), functional)
    s.set_option("quirks", 0)
    for k, v in opts.items():
        s.set_option(k, v)
    return s


class Planes:
    """The inputs of one shape on the device: the planes of xc_gradient_reference.inputs, the densities of spin_inputs."""

    def __init__(self, dev, ngrid, nao, na, nb):
        dm, ao, gr, w, hs = xr.inputs(ngrid, nao)
        dm_a, dm_b = sr.spin_inputs(ngrid, nao, na, nb)[:2]
        self.host = (dm_a, dm_b, ao, gr, w, hs)
        self.dm = dm
        self.ngrid, self.nao, self.dev = ngrid, nao, dev
        self.d_a, self.d_b, self.d_ao, self.d_gr, self.d_w, self.d_hs = (torch.as_tensor(np.array(a), device=dev) for a in self.host)

    def gradient(self, s, lo=0, hi=None, hess=True, dms=None):
        hi = self.ngrid if hi is None else hi
        d_a, d_b = dms if dms is not None else (self.d_a, self.d_b)
        d_out = torch.full((self.nao, 3), 7.0, dtype=torch.float64, device=self.dev)
        gr = self.d_gr[:, lo:hi].contiguous()
        hs = self.d_hs[:, lo:hi].contiguous() if hess else None
        assert s.compute_xc_gradient_spin(hi - lo, self.nao, d_a, d_b, self.d_ao[lo:hi], self.d_w[lo:hi], d_out, gr, hs) == 0
        torch.cuda.synchronize()
        return d_out.cpu().numpy()

    def host_gradient(self, functional):
        dm_a, dm_b, ao, gr, w, hs = self.host
        return gradients.xc_gradient_spin_host(functional, dm_a, dm_b, ao, w, gr, hs)


def _check(label, G, ref, bound=ERR_REL):
    scale = float(np.abs(ref).max())
    err = float(np.abs(G - ref).max())
    print(f"gpu {label}: max|G| {scale:.3e}  err {err / scale:.2e}")
    assert np.all(np.isfinite(G)), label
    assert err <= bound * scale, (label, err / scale)


@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_matches_the_host(dev, shape, functional):
    p = Planes(dev, *shape)
    if shape[3] == 0:
        assert not np.any(p.host[1])
    G = p.gradient(_solver(functional), hess=functional != "LDA")
    _check(f"DFT_ComputeXCGradientSpin {functional} {shape}", G, p.host_gradient(functional))


@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("shape", SHAPES)
def test_one_kernel_for_both_spins_matches_one_launch_per_spin(dev, shape, functional):
    p = Planes(dev, *shape)
    s = _solver(functional)
    assert s.get_option("xcg_spin_fused") == 1.0          # the default
    G = p.gradient(s, hess=functional != "LDA")
    s.set_option("xcg_spin_fused", 0)
    G2 = p.gradient(s, hess=functional != "LDA")
    err = float(np.abs(G - G2).max() / np.abs(G2).max())
    print(f"gpu k_xc_grad on both spins against two launches of k_xc_grad {functional} {shape}: {err:.2e}")
    assert err <= 1e-13
    _check(f"DFT_ComputeXCGradientSpin xcg_spin_fused=0 {functional} {shape}", G2, p.host_gradient(functional))
    assert np.array_equal(G2, p.gradient(s, hess=functional != "LDA"))          # the plain form is reproducible too


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("functional", ["LDA", "GGA", "B3LYP"])
def test_validation_paths(dev, functional, path):
    p = Planes(dev, 2085, 24, 5, 4)
    G = p.gradient(_solver(functional, path=path))
    _check(f"DFT_ComputeXCGradientSpin {functional} (2085, 24) path={path}", G, p.host_gradient(functional))


@pytest.mark.parametrize("functional", FUNCTIONALS)
@pytest.mark.parametrize("shape", [(2085, 24, 5, 4), (2085, 114, 21, 19), (1100, 130, 12, 9)])
def test_closed_shell_limit(dev, shape, functional):
    """dm_a = dm_b = dm/2 against DFT_ComputeXCGradient of dm at quirks 0.  Densities, matrices and contraction are the same
    arithmetic (halving is exact); the coefficients come from two formulations of the functional, the closed-shell bodies
    and the spin-resolved ones, which agree point by point to 3.9e-13 at the worst (pw92_c / pbe_c, profiles/spin_parity.txt,
    "cpu reference").  G is a sum of such coefficients times fixed factors, so 1e-12 of max|G| bounds the difference."""
    p = Planes(dev, *shape)
    s = _solver(functional)
    d_dm = torch.as_tensor(np.array(p.dm), device=dev)
    half = (0.5 * d_dm).contiguous()
    G = p.gradient(s, dms=(half, half))
    d_out = torch.zeros((p.nao, 3), dtype=torch.float64, device=dev)
    assert s.compute_xc_gradient(p.ngrid, p.nao, d_dm, p.d_ao, p.d_w, d_out, p.d_gr, p.d_hs) == 0
    torch.cuda.synchronize()
    _check(f"DFT_ComputeXCGradientSpin {functional} {shape[:2]} at dm/2, dm/2 against DFT_ComputeXCGradient", G, d_out.cpu().numpy(), 1e-12)


@pytest.mark.parametrize("shape", [(2085, 114, 21, 19), (1100, 130, 12, 9)])
def test_a_call_is_bitwise_reproducible_and_slices_add_up(dev, shape):
    p = Planes(dev, *shape)
    s = _solver("B3LYP")
    G = p.gradient(s)
    assert np.array_equal(G, p.gradient(s))
    cut = 16 * 41 + 3      # not a multiple of the row tile: both slices end ragged
    two = p.gradient(s, 0, cut) + p.gradient(s, cut, shape[0])
    err = float(np.abs(two - G).max() / np.abs(G).max())
    print(f"gpu spin gradient, two slices against the whole grid {shape}: {err:.2e}")
    assert err <= 1e-13


@pytest.mark.parametrize("functional,shape", [("GGA", (2085, 24, 5, 4)), ("B3LYP", (2085, 114, 21, 19)), ("LDA", (1100, 130, 12, 9))])
def test_the_sweeps_and_the_response_table_are_left_as_they_were(dev, functional, shape):
    p = Planes(dev, *shape)
    s = _solver(functional)
    n = p.nao
    gr = p.d_gr if functional != "LDA" else None
    d_dm = torch.as_tensor(np.array(p.dm), device=dev)

    def sweep():
        d_v = torch.zeros((n, n), dtype=torch.float64, device=dev)
        e = s.compute_xc(p.ngrid, n, d_dm, p.d_ao, p.d_w, d_v, gr)
        return e, d_v.cpu().numpy()

    def spin_sweep():
        d_va, d_vb = (torch.zeros((n, n), dtype=torch.float64, device=dev) for _ in range(2))
        e = s.compute_xc_spin(p.ngrid, n, p.d_a, p.d_b, p.d_ao, p.d_w, d_va, d_vb, gr)
        return e, d_va.cpu().numpy(), d_vb.cpu().numpy()

    sweep(); e0, v0 = sweep()          # the second call is the one a graph would be recorded from
    s0 = spin_sweep()
    assert s.fxc_prepare_spinpol(p.ngrid, n, p.d_a, p.d_b, p.d_ao, p.d_w, gr) == 0
    t0 = s.fxc_spinpol_table(p.ngrid, dev).clone()
    G = p.gradient(s)
    assert np.all(np.isfinite(G))
    t1 = s.fxc_spinpol_table(p.ngrid, dev)
    assert torch.equal(t0, t1)
    s1 = spin_sweep()
    e1, v1 = sweep()
    assert s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and np.array_equal(s0[2], s1[2])
    assert e0 == e1 and np.array_equal(v0, v1)


def test_refusals(dev):
    p = Planes(dev, 37, 50, 6, 5)
    d_out = torch.zeros((50, 3), dtype=torch.float64, device=dev)
    args = (37, 50, p.d_a, p.d_b, p.d_ao, p.d_w, d_out)
    with pytest.raises(RuntimeError, match="null for a gradient-corrected functional"):
        _solver("GGA").compute_xc_gradient_spin(*args, p.d_gr, None)
    with pytest.raises(RuntimeError, match="null for a gradient-corrected functional"):
        _solver("B3LYP").compute_xc_gradient_spin(*args, None, p.d_hs)
    with pytest.raises(RuntimeError, match="needs ao_grad"):
        _solver("LDA").compute_xc_gradient_spin(*args, None, None)
    with pytest.raises(RuntimeError, match="needs both density matrices"):
        _solver("LDA").compute_xc_gradient_spin(37, 50, p.d_a, None, p.d_ao, p.d_w, d_out, p.d_gr, None)
    with pytest.raises(RuntimeError, match="needs both density matrices"):
        _solver("LDA").compute_xc_gradient_spin(37, 50, p.d_a, p.d_b, p.d_ao, p.d_w, None, p.d_gr, None)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _solver("LDA").compute_xc_gradient_spin(0, 50, p.d_a, p.d_b, p.d_ao, p.d_w, d_out, p.d_gr, None)
    for functional in ("LDA", "GGA", "PBE0"):          # quirks = 1 with vwn5_c, pbe_c, pbe_c in a mix: DFT_ComputeXCSpin's refusal
        s = q.DFTSolverWrapper(q.build_library(), functional)
        s.set_option("quirks", 1)
        with pytest.raises(RuntimeError, match="first derivatives of the energy.*--quirks 0"):
            s.compute_xc_gradient_spin(*args, p.d_gr, p.d_hs)
    s = q.DFTSolverWrapper(q.build_library(), "B3LYP")          # neither component: served at quirks 1
    s.set_option("quirks", 1)
    assert s.compute_xc_gradient_spin(*args, p.d_gr, p.d_hs) == 0
    torch.cuda.synchronize()
    # Two faults in one call: the first in the order include/dft_solver.h states for the six gradient-side entries, one case
    # per adjacent pair (the LDS request and the device end it: tests/test_meta_gradient_cpu.py, where there is no device)
    nodm = (37, 50, None, p.d_b, p.d_ao, p.d_w, d_out)
    with pytest.raises(RuntimeError, match="meta-GGA.*this entry would drop it"):       # the solver's kind, a null pointer
        _solver("TPSS").compute_xc_gradient_spin(*nodm, p.d_gr, p.d_hs)
    with pytest.raises(RuntimeError, match="needs both density matrices"):              # a null pointer, the sizes
        _solver("GGA").compute_xc_gradient_spin(0, 50, None, p.d_b, p.d_ao, p.d_w, d_out, p.d_gr, p.d_hs)
    with pytest.raises(RuntimeError, match="bad sizes"):                                # the sizes, ao_grad of a gradient solver
        _solver("GGA").compute_xc_gradient_spin(0, 50, p.d_a, p.d_b, p.d_ao, p.d_w, d_out, None, p.d_hs)
    with pytest.raises(RuntimeError, match="ao_grad pointer is null"):                  # ao_grad, ao_hess of a gradient solver
        _solver("GGA").compute_xc_gradient_spin(*args, None, None)
    with pytest.raises(RuntimeError, match="ao_hess pointer is null"):                  # ao_hess, quirks = 1
        _solver("GGA", quirks=1).compute_xc_gradient_spin(*args, p.d_gr, None)
    with pytest.raises(RuntimeError, match="needs ao_grad"):                            # ao_grad of an LDA solver, quirks = 1
        _solver("LDA", quirks=1).compute_xc_gradient_spin(*args, None, None)
    with pytest.raises(RuntimeError, match="first derivatives of the energy"):          # quirks = 1, the LDS request
        _solver("GGA", quirks=1).compute_xc_gradient_spin(37, 1700, p.d_a, p.d_b, p.d_ao, p.d_w, d_out, p.d_gr, p.d_hs)
    with pytest.raises(RuntimeError, match="bytes of LDS per workgroup"):               # ... which alone is refused too, before any launch
        _solver("GGA").compute_xc_gradient_spin(37, 1700, p.d_a, p.d_b, p.d_ao, p.d_w, d_out, p.d_gr, p.d_hs)
