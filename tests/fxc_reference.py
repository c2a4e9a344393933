"""Reference for the linear response of Vxc (TEST INFRASTRUCTURE: lives under tests/).

V1_ref = Richardson-extrapolated central difference of the ORACLE's Vxc along dm0 + t dm1 -- never the code under test:

    D(t)  = (Vxc(dm0 + t dm1) - Vxc(dm0 - t dm1)) / (2 t)
    R(t)  = (4 D(t/2) - D(t)) / 3                       (removes the t^2 term)
    ref   = R(0.05)   (steps 0.05 and 0.025),   bar = max |R(0.1) - R(0.05)|

Inputs: dm0 = helpers.synth_inputs(ngrid, nao, nocc=...) with nocc >= 3 (a rank-1 dm drives rho through the cut-off
under the perturbation and the quotient is then meaningless); dm1 random, scaled so that max_g |rho1 / rho0| = 0.25.

The extrapolated difference's own error is the t^4 term, weighted by how the ratio rho1 / rho0 is spread over the grid: for
a random dm1 its bar is 1e-9 .. 1e-7 of max |V1| (median 1e-8 for GGA and 3e-8 for B3LYP at (96, 5, 3) over 3000 seeds).
SEEDS holds, per shape, the first seed found whose bar is at most 1.4e-9 for EVERY functional tested at that shape (a choice
of input by a property of the reference alone -- the code under test was not consulted), so that every case can assert
bar <= 2e-9 before it looks at the device.
"""
import functools
import os

import numpy as np

import oracle
from helpers import synth_inputs
from mix_reference import compute_xc_mix

SHAPES = [(96, 5, 3), (257, 24, 6), (300, 36, 8), (333, 114, 21), (160, 130, 26)]
SEEDS = {(96, 5, 3): 1634, (257, 24, 6): 200, (300, 36, 8): 23, (333, 114, 21): 20, (160, 130, 26): 159}
TYPES = {"LDA": 0, "GGA": 1, "B3LYP": 2}
BAR_REL = 2e-9      # the reference's own error bar, relative to max |V1| (measured 7.7e-11 .. 1.65e-9 at SHAPES)
ERR_REL = 2e-8      # ten times that: the bound on |V1 - V1_ref|


def _rho(dm, ao):
    ds = 0.5 * (dm + dm.T)
    return np.einsum("gi,gi->g", ao @ ds, ao)


@functools.lru_cache(maxsize=None)
def inputs(ngrid, nao, nocc, symmetric=True, zero_rows=0, seed=None):
    """(dm0, dm1, ao, ao_grad, w), read-only."""
    seed = SEEDS[(ngrid, nao, nocc)] if seed is None else seed
    dm0, ao, gr, w = synth_inputs(ngrid, nao, nocc=nocc)
    if zero_rows:
        ao = ao.copy(); gr = gr.copy()
        ao[3:3 + zero_rows] = 0.0
        gr[:, 3:3 + zero_rows] = 0.0
    rng = np.random.default_rng(seed + 1000 * nao + ngrid)
    a = rng.standard_normal((nao, nao))
    dm1 = 0.5 * (a + a.T) if symmetric else a
    r0, r1 = _rho(dm0, ao), _rho(dm1, ao)
    live = r0 > 0.0
    dm1 = dm1 * (0.25 / np.max(np.abs(r1[live] / r0[live])))
    for x in (dm0, dm1, ao, gr, w):
        x.setflags(write=False)
    return dm0, dm1, ao, gr, w


def _vxc(functional, dm, ao, w, gr, quirks):
    if functional in TYPES:
        t = TYPES[functional]
        return oracle.compute_xc(t, dm, ao, w, gr if t else None, quirks=quirks)[1]
    return compute_xc_mix(functional, dm, ao, w, gr, quirks=quirks)[1]


@functools.lru_cache(maxsize=None)
def reference(functional, ngrid, nao, nocc, quirks, symmetric=True, zero_rows=0):
    """(V1_ref, bar) for `functional` ("LDA" / "GGA" / "B3LYP" by the oracle's solver types, anything else as a mix)."""
    dm0, dm1, ao, gr, w = inputs(ngrid, nao, nocc, symmetric, zero_rows)
    D = {}
    for t in (0.1, 0.05, 0.025):
        D[t] = (_vxc(functional, dm0 + t * dm1, ao, w, gr, quirks) - _vxc(functional, dm0 - t * dm1, ao, w, gr, quirks)) / (2.0 * t)
    r_coarse = (4.0 * D[0.05] - D[0.1]) / 3.0
    r_fine = (4.0 * D[0.025] - D[0.05]) / 3.0
    r_fine.setflags(write=False)
    return r_fine, float(np.abs(r_fine - r_coarse).max())


def record(where, label, bar_rel, err_rel):
    """One line per measured case into fxc_parity.txt (kept sorted, one line per label) in the directory
    QCDFT_WRITE_PROFILES names -- how profiles/fxc_parity.txt was made; an ordinary test run writes nothing."""
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    PROFILE = os.path.join(out_dir, "fxc_parity.txt")
    line = f"{where:4s} {label:58s} reference bar / max|V1| {bar_rel:9.2e}   error / max|V1| {err_rel:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(PROFILE)] if os.path.exists(PROFILE) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{where:4s} {label:58s}")]
        if not head:
            head = ["# Linear response of Vxc against Richardson-extrapolated differences of the oracle (tests/fxc_reference.py).",
                    "# Written by tests/test_fxc_cpu.py (cpu) and tests/test_gpu_fxc.py (gpu); bounds: bar <= 2e-9, error <= 2e-8."]
        with open(PROFILE, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass


def check(where, label, v1, ref, bar):
    """The two assertions of every parity case, figures printed and recorded first."""
    scale = float(np.abs(ref).max())
    err = float(np.abs(np.asarray(v1) - ref).max())
    print(f"{where} {label}: max|V1| {scale:.3e}  bar {bar / scale:.2e}  err {err / scale:.2e}")
    record(where, label, bar / scale, err / scale)
    assert np.all(np.isfinite(v1)), label
    assert bar <= BAR_REL * scale, (label, bar / scale)
    assert err <= ERR_REL * scale, (label, err / scale)
