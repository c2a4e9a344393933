"""Shared pieces of the open-shell response tests (TEST INFRASTRUCTURE: lives under tests/).

* golden(): tests/golden/spin_hessian_ref.npz -- all second derivatives of the energy per component at polarised points, from
  the 60-digit restatements (tests/golden/make_spin_hessian_reference.py; its docstring defines the points).
* perturbed_inputs(): spin_reference.spin_inputs with two random symmetric perturbations dm1_a, dm1_b, each scaled so that
  max_g |rho1_s / rho0_s| = 0.25 (the recipe of fxc_reference.inputs, per spin).
* difference_reference(): Richardson-extrapolated central differences of response.xc_spin_host along (dm0_a + t dm1_a,
  dm0_b + t dm1_b), steps as in fxc_reference.reference: ref = R(0.05), bar = max |R(0.1) - R(0.05)| per spin.
* record(): one line per measured figure into spin_response_parity.txt in the directory QCDFT_WRITE_PROFILES names -- how
  profiles/spin_response_parity.txt was made; an ordinary test run writes nothing.

HESSIAN_BAR and CLOSED_SHELL_BAR are ten times the worst figure the host tests measured (profiles/spin_response_parity.txt).
"""
import functools
import os

import numpy as np

import spin_reference as sr
from quantum_compute_dft_amd import response

HERE = os.path.dirname(os.path.abspath(__file__))
# fxc_table_pol_host against the 60-digit reference, |got - ref| / |ref| entry by entry (an entry the code leaves out must be
# exactly zero): worst measured 5.4e-12, pbe_c d2/drb2 at rho = 1e-7, zeta = 0.9 (profiles/spin_response_parity.txt, "cpu hessian")
HESSIAN_BAR = 5.4e-11
# fxc_apply_spinpol_host at dm0_a = dm0_b against fxc_apply_host kinds "singlet-spin" and "triplet", relative to max|V1|:
# worst measured 5.0e-16 (profiles/spin_response_parity.txt, "cpu closed shell")
CLOSED_SHELL_BAR = 5.0e-15
FD_SHAPES = [(257, 24, 5, 4), (333, 114, 21, 20)]
# the difference reference's own bar must stay a small fraction of max|V1| for the comparison to mean anything: the t^4 term
# at these steps, measured 1.3e-9 .. 1.3e-7 over FD_SHAPES and the five functionals
FD_BAR_CAP = 1e-6
RHO_CUT, SIGMA_CUT = 1e-12, 1e-20


@functools.lru_cache(maxsize=None)
def golden():
    ref = np.load(os.path.join(HERE, "golden", "spin_hessian_ref.npz"))
    assert list(ref["components"]) == sr.COMPONENTS
    return {k: ref[k] for k in ref.files}


def _rho(dm, ao):
    return np.einsum("gi,gi->g", ao @ (0.5 * (dm + dm.T)), ao)


@functools.lru_cache(maxsize=None)
def perturbed_inputs(ngrid, nao, na, nb, symmetric=True, seed=41):
    """(dm0_a, dm0_b, dm1_a, dm1_b, ao, ao_grad, w), read-only.  nb = 0: dm1_b is a random matrix of norm 1 (no density to
    scale it by)."""
    da, db, ao, gr, w, _, _ = sr.spin_inputs(ngrid, nao, na, nb)
    rng = np.random.default_rng(seed + 1000 * nao + ngrid)
    out = []
    for d0 in (da, db):
        a = rng.standard_normal((nao, nao))
        d1 = 0.5 * (a + a.T) if symmetric else a
        r0, r1 = _rho(d0, ao), _rho(d1, ao)
        live = r0 > 0.0
        d1 = d1 * (0.25 / np.max(np.abs(r1[live] / r0[live]))) if live.any() else d1 / np.linalg.norm(d1)
        d1.setflags(write=False)
        out.append(d1)
    return da, db, out[0], out[1], ao, gr, w


def no_point_at_a_cutoff(da, db, d1a, d1b, ao, gr, tmax=0.1):
    """True when, along the whole difference stencil, both spin densities stay above the density cut-off and the three
    quantities the bodies compare with the sigma cut-off (4 sigma_aa, 4 sigma_bb, sigma) stay above it."""
    ok = True
    for t in (-tmax, 0.0, tmax):
        ra, ga = response._density(da + t * d1a, ao, gr)
        rb, gb = response._density(db + t * d1b, ao, gr)
        ok &= bool(ra.min() > 10.0 * RHO_CUT and rb.min() > 10.0 * RHO_CUT)
        if gr is not None:
            saa, sbb, sab = (np.einsum("gk,gk->g", u, v) for u, v in ((ga, ga), (gb, gb), (ga, gb)))
            ok &= bool(min(saa.min(), sbb.min(), (saa + 2.0 * sab + sbb).min()) > 10.0 * SIGMA_CUT)
    return ok


@functools.lru_cache(maxsize=None)
def difference_reference(functional, shape):
    """((V1_a_ref, V1_b_ref), (bar_a, bar_b))."""
    da, db, d1a, d1b, ao, gr, w = perturbed_inputs(*shape)
    g = gr if functional != "LDA" else None
    D = {}
    for t in (0.1, 0.05, 0.025):
        p = response.xc_spin_host(functional, da + t * d1a, db + t * d1b, ao, w, g)[1:]
        m = response.xc_spin_host(functional, da - t * d1a, db - t * d1b, ao, w, g)[1:]
        D[t] = [(x - y) / (2.0 * t) for x, y in zip(p, m)]
    coarse = [(4.0 * b - a) / 3.0 for a, b in zip(D[0.1], D[0.05])]
    fine = [(4.0 * b - a) / 3.0 for a, b in zip(D[0.05], D[0.025])]
    for x in fine:
        x.setflags(write=False)
    return tuple(fine), tuple(float(np.abs(f - c).max()) for f, c in zip(fine, coarse))


def record(label, figure, bar):
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "spin_response_parity.txt")
    line = f"{label:78s} measured {figure:9.2e}   bar {bar:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{label:78s}")]
        if not head:
            head = ["# Open-shell response of Vxc (xc::spin_hessian_entry, DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol) and the UKS solvers on",
                    "# it: measured worst figures and the bars the tests assert (tests/test_spin_response_cpu.py on the host,",
                    "# tests/test_gpu_spin_response.py on the device).  Written with QCDFT_WRITE_PROFILES=profiles."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass
