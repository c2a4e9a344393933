"""References for the triplet (spin-flip) response tests (TEST INFRASTRUCTURE: lives under tests/).

* golden(): tests/golden/triplet_kernel_ref.npz -- T0..T4 of both kinds and the energy at zeta in {0, 0.3, 1} per
  component, from the 60-digit restatement of the eight spin-resolved energy densities in
  tests/golden/make_triplet_kernel_reference.py (its docstring defines the entries and the point grid).
* difference_table(): the same five entries from Richardson-extrapolated central differences of
  response.spin_energy_host, the style of tests/test_fxc_cpu.py one derivative order up.
* state() / triplet_dense(): H2O / STO-3G on the host (the pattern of tests/test_excitations_cpu.py), for any functional
  expression -- the oracle backend for the three built-in types, mix_reference.MixBackend otherwise.
* record(): one line per measured figure into triplet_parity.txt in the directory QCDFT_WRITE_PROFILES names -- how
  profiles/triplet_parity.txt was made; an ordinary test run writes nothing.
"""
import functools
import os

import numpy as np

from quantum_compute_dft_amd import excitations as ex
from quantum_compute_dft_amd import functionals, inputs, response, scf
from excitation_dense import dense_matrices
from mix_reference import MixBackend
from scf_oracle_backend import OracleBackend

COMPONENTS = list(functionals.COMPONENTS)
HERE = os.path.dirname(os.path.abspath(__file__))
# Hartree-Fock as a functional: exact exchange alone.  functionals.resolve takes a Functional as it is (the expression
# parser wants a density-functional component), and so does everything the tests hand it to.
HF = functionals.Functional("1.0*hf", {}, 1.0, None)


def functional_of(name):
    return HF if name == "1.0*hf" else name


@functools.lru_cache(maxsize=None)
def golden():
    ref = np.load(os.path.join(HERE, "golden", "triplet_kernel_ref.npz"))
    assert list(ref["components"]) == COMPONENTS
    return {k: ref[k] for k in ref.files}


def unit(k):
    w = np.zeros(len(COMPONENTS))
    w[k] = 1.0
    return w


def polarised(rho, sigma, zeta):
    """(ra, rb, saa, sab, sbb) at polarisation zeta with grad ra and grad rb parallel: the arguments of the golden energies."""
    p, m = 0.5 * (1.0 + zeta), 0.5 * (1.0 - zeta)
    return rho * p, rho * m, sigma * p * p, sigma * p * m, sigma * m * m


def difference_table(functional, rho, sigma, kind, d):
    """(5, n): T0..T4 by central differences of spin_energy_host with relative step d, the mixed second differences on
    the symmetric four-point stencil, extrapolated twice: R1(d) = (4 D(d/2) - D(d)) / 3 removes the d^2 term,
    R2(d) = (16 R1(d/2) - R1(d)) / 15 the d^4 term (steps d, d/2, d/4)."""
    sg, ab = (-1.0, 0.0) if kind == 1 else (1.0, 1.0)
    h, q = 0.5 * rho, 0.25 * sigma
    E = lambda *a: response.spin_energy_host(functional, *a)
    rdir = lambda x, u, t: E(h + x + 0.5 * t, h + sg * 0.5 * t, q + 2.0 * u, q + sg * u, q)
    sdir = lambda x, u, t: E(h + x, h, q + 2.0 * u + 0.25 * t, q + sg * u + ab * 0.25 * t, q + sg * 0.25 * t)
    z = np.zeros_like(rho)

    def twice(D):
        d1, d2, d4 = D(1.0), D(0.5), D(0.25)
        return (16.0 * (4.0 * d4 - d2) / 3.0 - (4.0 * d2 - d1) / 3.0) / 15.0

    def mixed(f, ha, hb):
        return twice(lambda s: (f(s * ha, s * hb) - f(s * ha, -s * hb) - f(-s * ha, s * hb) + f(-s * ha, -s * hb)) / (4.0 * s * s * ha * hb))

    def first(f, ha):
        return twice(lambda s: (f(s * ha) - f(-s * ha)) / (2.0 * s * ha))

    hx, hu, tr, ts = d * h, d * 0.5 * q, d * rho, d * sigma
    return np.array([mixed(lambda x, t: rdir(x, z, t), hx, tr), mixed(lambda x, t: sdir(x, z, t), hx, ts),
                     mixed(lambda u, t: rdir(z, u, t), hu, tr), mixed(lambda u, t: sdir(z, u, t), hu, ts),
                     first(lambda u: rdir(z, u, z), hu)])


@functools.lru_cache(maxsize=None)
def state(functional, quirks=0, molecule="H2O", basis="sto-3g"):
    """(inp, converged SCF result, response.HostResponse) on the host."""
    inp = inputs.build(molecule, basis, grid_level=1, verbose=False)
    name, functional = functional, functional_of(functional)
    if name.upper() in ("LDA", "GGA", "B3LYP"):
        be = OracleBackend(inp, functional, quirks=bool(quirks))
    else:
        be = MixBackend(inp, functional, quirks=bool(quirks))
    res = scf.run_scf(inp, be, functional, conv_e=1e-12, conv_dm=1e-9, log=None)
    assert res["converged"]
    return inp, res, response.HostResponse(inp, functional, be, be.ao, be.gr, quirks=bool(quirks))


@functools.lru_cache(maxsize=None)
def triplet_dense(functional, quirks=0):
    """(ops, A+B, A-B as (N, N) matrices) of the triplet operators."""
    inp, res, rb = state(functional, quirks)
    ops = ex.ResponseOperators(inp, res, rb, functional_of(functional), triplet=True)
    return (ops,) + dense_matrices(ops)


def record(label, figure, bar):
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "triplet_parity.txt")
    line = f"{label:72s} measured {figure:9.2e}   bar {bar:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{label:72s}")]
        if not head:
            head = ["# Spin-flip (triplet) and singlet tables of the spin-resolved energy bodies: measured worst figures and the bars",
                    "# the tests assert (tests/test_triplet_cpu.py on the host, tests/test_gpu_triplet.py on the device).",
                    "# Written with QCDFT_WRITE_PROFILES=profiles; figures are relative to the largest entry of the plane compared."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass
