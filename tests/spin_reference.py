"""Shared pieces of the open-shell tests (TEST INFRASTRUCTURE: lives under tests/).

* golden(): tests/golden/spin_potential_ref.npz -- e and its five first derivatives per component at polarised points, from
  the 60-digit restatements (tests/golden/make_spin_potential_reference.py; its docstring defines the points).
* spin_inputs(): AO planes and weights of helpers.synth_inputs with two spin densities cocc_s cocc_s^T of random orbitals.
* closed_shell_reference(): Exc and Vxc of the oracle at quirks 0 -- oracle.compute_xc for the three built-in types, the
  oracle's pieces composed by mix_reference.compute_xc_mix for every other functional.
* record(): one line per measured figure into spin_parity.txt in the directory QCDFT_WRITE_PROFILES names -- how
  profiles/spin_parity.txt was made; an ordinary test run writes nothing.

REFERENCE_BAR and CLOSED_SHELL_BAR below are shared by the host and the device tests: each is ten times the worst figure the
host tests measured (profiles/spin_parity.txt).
"""
import functools
import os

import numpy as np

import helpers
import mix_reference
import oracle
from quantum_compute_dft_amd import functionals

HERE = os.path.dirname(os.path.abspath(__file__))
COMPONENTS = list(functionals.COMPONENTS)
FUNCTIONALS = ["LDA", "GGA", "B3LYP", "PBE0", "BLYP"]
BUILTIN = {"LDA": 0, "GGA": 1, "B3LYP": 2}
# point_spin_host against the 60-digit reference, |got - ref| / |ref| point by point (an entry whose reference is exactly
# zero must be exactly zero): worst measured 3.9e-13, pw92_c and pbe_c on top of it (profiles/spin_parity.txt, "cpu reference")
REFERENCE_BAR = 3.9e-12
# xc_spin_host(dm/2, dm/2) against the oracle at quirks 0 on CLOSED_SHELL_SHAPES, Exc relative and V_alpha, V_beta relative to
# max|V|: worst measured 4.0e-15 (profiles/spin_parity.txt, "cpu closed shell")
CLOSED_SHELL_BAR = 4.0e-14
# (ngrid, nao): a small one, and the three plane shapes of tests/test_gpu_spin.py, which holds the device to the same bar
CLOSED_SHELL_SHAPES = [(700, 13), (2085, 24), (2085, 114), (1100, 130)]



@functools.lru_cache(maxsize=None)
def golden():
    ref = np.load(os.path.join(HERE, "golden", "spin_potential_ref.npz"))
    assert list(ref["components"]) == COMPONENTS
    return {k: ref[k] for k in ref.files}


def unit(k):
    w = np.zeros(len(COMPONENTS))
    w[k] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def spin_inputs(ngrid, nao, na, nb, need_grad=True, seed=helpers.SEED):
    """(dm_a, dm_b, ao, ao_grad, w, cocc_a, cocc_b): the planes of helpers.synth_inputs, dm_s = cocc_s cocc_s^T with random
    orbitals 0.5 N (nao, n_s).  Shared between tests: treat as read-only."""
    _, ao, gr, w = helpers.synth_inputs(ngrid, nao, need_grad=need_grad, seed=seed)
    rng = np.random.default_rng(seed + 17)
    ca, cb = 0.5 * rng.standard_normal((nao, na)), 0.5 * rng.standard_normal((nao, nb))
    return ca @ ca.T, cb @ cb.T, ao, gr, w, ca, cb


def closed_shell_reference(functional, dm, ao, w, gr):
    if functional in BUILTIN:
        return oracle.compute_xc(BUILTIN[functional], dm, ao, w, gr if functional != "LDA" else None, quirks=False)
    return mix_reference.compute_xc_mix(functional, dm, ao, w, gr, quirks=False)


def record(label, figure, bar):
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "spin_parity.txt")
    line = f"{label:72s} measured {figure:9.2e}   bar {bar:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{label:72s}")]
        if not head:
            head = ["# Open-shell XC (xc::spin_potential_point, DFT_ComputeXCSpin): measured worst figures and the bars the tests assert",
                    "# (tests/test_spin_potential_cpu.py and tests/test_uks_cpu.py on the host, tests/test_gpu_spin.py on the device).",
                    "# Written with QCDFT_WRITE_PROFILES=profiles."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass
