"""Reference for the XC part of the nuclear gradient of a meta-GGA (TEST INFRASTRUCTURE: lives under tests/).

The inputs are tests/xc_gradient_reference.py's (`inputs`: the synthetic planes and its six random Hessian planes), the
reference is built exactly as `xc_gradient_reference.reference` builds it -- central differences at H and 2 H of the Exc
under the column replacement, Richardson-extrapolated, bar = max |D_R - D(H)| -- but on metagga.xc_meta_host's Exc: the
energy the closed-shell meta-GGA sweep is tested against, never the gradient code.  tau is made of the gradient planes, so
the replacement d_k phi_mu -> d_k phi_mu - t d_xk phi_mu moves it, which is the term under test.  `check_fd` is
xc_gradient_reference's, unchanged: err <= max(10 bar, 1e-9 scale) and 10 bar <= 1e-6 scale.
"""
import functools
import os

import numpy as np

from quantum_compute_dft_amd import metagga
from xc_gradient_reference import COLUMNS, H, HESS_INDEX, inputs  # noqa: F401  (inputs: shared with the GGA tests, read-only)

FUNCTIONALS = ("TPSS", "TPSSh", "0.5*tpss_x + 0.5*pbe_x + lyp_c")


@functools.lru_cache(maxsize=None)
def reference(functional, ngrid, nao):
    """(columns, D_R (len(columns), 3), bar) of the meta-GGA `functional` at inputs(ngrid, nao)."""
    dm, ao, gr, w, hs = inputs(ngrid, nao)
    cols = COLUMNS[nao]
    a, g = ao.copy(), gr.copy()
    D = {}
    for h in (H, 2.0 * H):
        out = np.zeros((len(cols), 3))
        for i, mu in enumerate(cols):
            for x in range(3):
                e = []
                for t in (h, -h):
                    a[:, mu] = ao[:, mu] - t * gr[x][:, mu]
                    for k in range(3):
                        g[k][:, mu] = gr[k][:, mu] - t * hs[HESS_INDEX[x][k]][:, mu]
                    e.append(metagga.xc_meta_host(functional, dm, a, w, g)[0])
                out[i, x] = (e[0] - e[1]) / (2.0 * h)
            a[:, mu] = ao[:, mu]
            g[:, :, mu] = gr[:, :, mu]
        D[h] = out
    ref = (4.0 * D[H] - D[2.0 * H]) / 3.0
    ref.setflags(write=False)
    return cols, ref, float(np.abs(ref - D[H]).max())


@functools.lru_cache(maxsize=None)
def host_gradient(functional, ngrid, nao):
    """gradients.xc_gradient_meta_host at inputs(ngrid, nao), computed once and shared, read-only."""
    from quantum_compute_dft_amd import gradients
    dm, ao, gr, w, hs = inputs(ngrid, nao)
    G = gradients.xc_gradient_meta_host(functional, dm, ao, w, gr, hs)
    G.setflags(write=False)
    return G


def record(where, label, bar_rel, err_rel, what="max|G|"):
    """One line per measured case into meta_gradient_parity.txt (kept sorted, one line per label) in the directory
    QCDFT_WRITE_PROFILES names -- how profiles/meta_gradient_parity.txt was made; an ordinary test run writes nothing."""
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "meta_gradient_parity.txt")
    key = f"{where:4s} {label:84s}"
    bar = "         " if bar_rel is None else f"{bar_rel:9.2e}"
    line = f"{key} reference bar / {what} {bar}   error / {what} {err_rel:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(key)]
        if not head:
            head = ["# Nuclear gradient of a meta-GGA: host against finite differences of metagga.xc_meta_host's Exc and of the converged energy,",
                    "# device against host (tests/meta_gradient_reference.py).  Written by tests/test_meta_gradient_cpu.py (cpu) and",
                    "# tests/test_gpu_meta_gradient.py (gpu) with QCDFT_WRITE_PROFILES=profiles.",
                    "# Finite-difference cases: error <= max(10 bar, 1e-9); 10 bar <= 1e-6 (planes), 1e-5 (whole gradient).  Device against host: 2e-8."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass


def check_fd(where, label, G, ref, bar, cap=1e-6):
    """xc_gradient_reference.check_fd's two assertions, figures printed and recorded (here) first.  cap: the bound on the
    reference's own bar, 1e-6 of the scale unless the case states another."""
    scale = float(np.abs(ref).max())
    err = float(np.abs(np.asarray(G) - ref).max())
    print(f"{where} {label}: scale {scale:.3e}  bar {bar / scale:.2e}  err {err / scale:.2e}")
    record(where, label, bar / scale, err / scale)
    assert np.all(np.isfinite(G)), label
    assert 10.0 * bar <= cap * scale, (label, bar / scale)
    assert err <= max(10.0 * bar, 1e-9 * scale), (label, err / scale, bar / scale)
