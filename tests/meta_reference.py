"""Shared pieces of the meta-GGA tests (TEST INFRASTRUCTURE: lives under tests/).

* golden(): tests/golden/meta_ref.npz -- e and its seven first derivatives per meta component, from the 60-digit restatement
  (tests/golden/make_meta_reference.py; its docstring defines the points).
* host(): metagga.xc_meta_host and metagga.tau_host per (functional, shape) on helpers.synth_inputs, computed once.
* MetaHostBackend: scf._run_scf backend (the set_dm / jk / xc interface of scf_oracle_backend.OracleBackend) for any
  functional with or without meta components, on metagga.xc_meta_host and the oracle's AO planes and J / K.
* energy_of(): the total energy of a set of occupied orbitals through such a backend (for the stationarity test).
* record(): one line per measured figure into meta_parity.txt in the directory QCDFT_WRITE_PROFILES names -- how
  profiles/meta_parity.txt was made; an ordinary test run writes nothing.

REFERENCE_BAR is ten times the worst figure the host test measured against the 60-digit reference (profiles/meta_parity.txt).
"""
import functools
import os
import time

import numpy as np

import helpers
import oracle
from quantum_compute_dft_amd import functionals, metagga

HERE = os.path.dirname(os.path.abspath(__file__))
COMPONENTS = list(functionals.META_COMPONENTS)
# meta_energy_host against the 60-digit reference, |got - ref| / |ref| entry by entry (an entry whose reference is exactly
# zero must be exactly zero).  Worst measured: tpss_x 1.4e-13 (e_sigma at z = 1e-8), tpss_c 2.0e-11 (e_tau at zeta = 0.9,
# where it is 1e-8 of e / tau and carries the cancellation of eps_PBE - eps~) -- profiles/meta_parity.txt, "cpu reference"
REFERENCE_BAR = {"tpss_x": 1.4e-12, "tpss_c": 2.0e-10}
# the shapes of tests/test_gpu_meta.py: (ngrid, nao, nocc or None for synth_inputs' own)
SHAPES = [(2085, 24, None), (2085, 114, None), (1100, 130, None), (333, 50, 1)]
# k_tau goes through K chunks above META_KC_MAX = 384 padded columns: one shape on each side of the first boundary, and
# one with three chunks whose last is ragged
CHUNK_SHAPES = [(400, 384, None), (400, 385, None), (112, 790, None)]
FUNCTIONALS = ["TPSS", "TPSSh", "0.5*tpss_x + 0.5*pbe_x + lyp_c"]


@functools.lru_cache(maxsize=None)
def golden():
    ref = np.load(os.path.join(HERE, "golden", "meta_ref.npz"))
    assert list(ref["components"]) == COMPONENTS
    return {k: ref[k] for k in ref.files}


def unit(k):
    """The weights (eight zeros, two meta weights) of meta component k alone."""
    return np.zeros(len(functionals.COMPONENTS)), np.eye(len(COMPONENTS))[k]


@functools.lru_cache(maxsize=None)
def inputs(ngrid, nao, nocc=None):
    """(dm, ao, ao_grad, w) of helpers.synth_inputs.  Shared between tests: treat as read-only."""
    return helpers.synth_inputs(ngrid, nao, nocc=nocc)


@functools.lru_cache(maxsize=None)
def host(functional, shape):
    """(Exc, V) of metagga.xc_meta_host on inputs(*shape)."""
    dm, ao, gr, w = inputs(*shape)
    return metagga.xc_meta_host(functional, dm, ao, w, gr)


class MetaHostBackend:
    def __init__(self, inp, functional):
        self.inp, self.f = inp, functionals.resolve(functional)
        self.ao, self.gr = oracle.eval_ao(inp.shells, inp.grids.coords, deriv=1)

    def set_dm(self, dm):
        self.dm = np.ascontiguousarray(dm)

    def jk(self, want_k):
        return oracle.coulomb(self.inp.eri, self.dm), (oracle.exchange(self.inp.eri, self.dm) if want_k else None)

    def xc(self):
        t0 = time.time()
        e, v = metagga.xc_meta_host(self.f, self.dm, self.ao, self.inp.grids.weights, self.gr)
        return e, v, time.time() - t0


def energy_of(inp, backend, c_hf, cocc):
    """E_tot of the closed-shell determinant of the occupied orbitals cocc (nao, nocc), orthonormal in S."""
    dm = 2.0 * cocc @ cocc.T
    backend.set_dm(dm)
    J, K = backend.jk(c_hf != 0.0)
    exc = backend.xc()[0]
    e = float(np.sum(dm * inp.Hcore)) + 0.5 * float(np.sum(dm * J)) + exc + inp.E_nuc
    if c_hf != 0.0:
        e -= 0.25 * c_hf * float(np.sum(dm * K))
    return e


def record(label, figure, bar):
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "meta_parity.txt")
    line = f"{label:84s} measured {figure:9.2e}   bar {bar:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{label:84s}")]
        if not head:
            head = ["# Meta-GGA XC (xc::meta_point, DFT_ComputeTau, DFT_ComputeXCMeta): measured worst figures and the bars the tests assert",
                    "# (tests/test_meta_cpu.py on the host, tests/test_gpu_meta.py on the device).",
                    "# Written with QCDFT_WRITE_PROFILES=profiles."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass
