"""Shared pieces of the open-shell meta-GGA tests (TEST INFRASTRUCTURE: lives under tests/).

* SHAPES / TAU_SHAPES: (ngrid, nao, nalpha, nbeta) of spin_reference.spin_inputs (dm_s = c_s c_s^T, so tau_s >= tau_W,s by
  Cauchy-Schwarz for any planes), the smallest that reach each path:
    (2085, 24, 5, 4)     ragged rows and columns
    (2085, 114, 9, 7)    the wave-specialised contraction, a ragged last 256-block
    (1100, 130, 9, 7)    two column blocks of k_vxc_tau, the split-K contraction
    (2085, 50, 3, 0)     fully polarised: an empty beta channel
    (333, 50, 1, 1)      one orbital per spin: z = 1 to rounding on both sides
    (333, 50, 1, 0)      the same with beta empty
    (400, 384, 6, 5), (400, 385, 6, 5), (112, 790, 6, 5)   tau only: one K chunk, two, three with a ragged last
* inputs(), host(), tau(): the planes, metagga.xc_meta_spin_host and metagga.tau_host per spin, computed once.
* gradients_for(): two gradients with given (sigma_aa, sigma_ab, sigma_bb).
* record(): one line per measured figure into meta_spin_parity.txt in the directory QCDFT_WRITE_PROFILES names -- how
  profiles/meta_spin_parity.txt was made; an ordinary test run writes nothing.
"""
import functools
import os

import numpy as np

import meta_reference as mr
import spin_reference as sr
from quantum_compute_dft_amd import metagga

SHAPES = [(2085, 24, 5, 4), (2085, 114, 9, 7), (1100, 130, 9, 7), (2085, 50, 3, 0), (333, 50, 1, 1), (333, 50, 1, 0)]
TAU_SHAPES = [(400, 384, 6, 5), (400, 385, 6, 5), (112, 790, 6, 5)]
FUNCTIONALS = mr.FUNCTIONALS
# xc_meta_spin_host(dm/2, dm/2) against xc_meta_host(dm), Exc relative and V_alpha, V_beta relative to max|V|.  The host pair
# stays inside spin_reference.CLOSED_SHELL_BAR (worst measured 2.2e-16,profiles/meta_spin_parity.txt, "cpu closed shell"),
# so that bar is the bar, on the host and on the device.
CLOSED_SHELL_BAR = sr.CLOSED_SHELL_BAR
E2E_BAR = 2e-8


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(dm_a, dm_b, ao, ao_grad, w) of spin_reference.spin_inputs.  Shared between tests: treat as read-only."""
    return sr.spin_inputs(*shape)[:5]


@functools.lru_cache(maxsize=None)
def host(functional, shape):
    """(Exc, V_a, V_b) of metagga.xc_meta_spin_host on inputs(shape)."""
    dm_a, dm_b, ao, gr, w = inputs(shape)
    return metagga.xc_meta_spin_host(functional, dm_a, dm_b, ao, w, gr)


@functools.lru_cache(maxsize=None)
def tau(shape):
    dm_a, dm_b, _, gr, _ = inputs(shape)
    return metagga.tau_host(dm_a, gr), metagga.tau_host(dm_b, gr)


def gradients_for(saa, sab, sbb):
    """(grad_a, grad_b), each (n, 3), with |grad_a|^2 = saa, grad_a . grad_b = sab and |grad_b|^2 = sbb up to rounding
    (sab^2 <= saa sbb): grad_a along x, grad_b in the xy plane."""
    saa, sab, sbb = (np.asarray(x, dtype=np.float64) for x in (saa, sab, sbb))
    ga, gb = np.zeros((saa.size, 3)), np.zeros((saa.size, 3))
    ga[:, 0] = np.sqrt(saa)
    live = saa > 0.0
    gb[live, 0] = sab[live] / ga[live, 0]
    gb[:, 1] = np.sqrt(np.maximum(sbb - gb[:, 0] ** 2, 0.0))
    return ga, gb


def sigmas_of(ga, gb):
    """(saa, sab, sbb) in the order of operations of xc::meta_spin_point."""
    dot = lambda p, q: p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]
    return dot(ga, ga), dot(ga, gb), dot(gb, gb)


def record(label, figure, bar):
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "meta_spin_parity.txt")
    line = f"{label:96s} measured {figure:9.2e}   bar {bar:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{label:96s}")]
        if not head:
            head = ["# Open-shell meta-GGA XC (xc::meta_spin_point, DFT_ComputeTauSpin, DFT_ComputeXCMetaSpin): measured worst figures and the",
                    "# bars the tests assert (tests/test_meta_spin_cpu.py on the host, tests/test_gpu_meta_spin.py on the device).",
                    "# Written with QCDFT_WRITE_PROFILES=profiles."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass
