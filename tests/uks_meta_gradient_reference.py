"""Reference for the XC part of the nuclear gradient of an open-shell meta-GGA (TEST INFRASTRUCTURE: lives under tests/).

A shape is (ngrid, nao, n_alpha, n_beta).  The planes and the six random Hessian planes are tests/xc_gradient_reference.py's
(`inputs(ngrid, nao)`), the two density matrices tests/spin_reference.py's (`spin_inputs`: the same planes, random
orbitals).  The reference is built exactly as `meta_gradient_reference.reference` builds it for the closed shell -- central
differences at H and 2 H of the Exc under the column replacement, Richardson-extrapolated, bar = max |D_R - D(H)| -- on
metagga.xc_meta_spin_host's Exc: the energy the open-shell meta-GGA sweep is tested against, never the gradient code.
`check_fd` is meta_gradient_reference's, recorded here into uks_meta_gradient_parity.txt.
"""
import functools
import os

import numpy as np

import meta_gradient_reference as mg
import spin_reference as sr
from quantum_compute_dft_amd import metagga
from xc_gradient_reference import COLUMNS, H, HESS_INDEX
from xc_gradient_reference import inputs as _planes

FUNCTIONALS = mg.FUNCTIONALS


@functools.lru_cache(maxsize=None)
def inputs(ngrid, nao, na, nb):
    """(dm_a, dm_b, ao, ao_grad (3, ngrid, nao), w, ao_hess (6, ngrid, nao)), read-only."""
    _, ao, gr, w, hs = _planes(ngrid, nao)
    dm_a, dm_b, ao_s, _, _, _, _ = sr.spin_inputs(ngrid, nao, na, nb)
    assert np.array_equal(ao, ao_s)          # one set of planes behind both helpers
    dm_a, dm_b = np.array(dm_a), np.array(dm_b)
    for x in (dm_a, dm_b):
        x.setflags(write=False)
    return dm_a, dm_b, ao, gr, w, hs


@functools.lru_cache(maxsize=None)
def reference(functional, shape):
    """(columns, D_R (len(columns), 3), bar) of the meta-GGA `functional` at inputs(*shape)."""
    dm_a, dm_b, ao, gr, w, hs = inputs(*shape)
    cols = COLUMNS[shape[1]]
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
                    e.append(metagga.xc_meta_spin_host(functional, dm_a, dm_b, a, w, g)[0])
                out[i, x] = (e[0] - e[1]) / (2.0 * h)
            a[:, mu] = ao[:, mu]
            g[:, :, mu] = gr[:, :, mu]
        D[h] = out
    ref = (4.0 * D[H] - D[2.0 * H]) / 3.0
    ref.setflags(write=False)
    return cols, ref, float(np.abs(ref - D[H]).max())


@functools.lru_cache(maxsize=None)
def host_gradient(functional, shape, shift=0.0):
    """gradients.xc_gradient_meta_spin_host at inputs(*shape) (shift: dm_s - shift I), computed once and shared, read-only."""
    from quantum_compute_dft_amd import gradients
    dm_a, dm_b, ao, gr, w, hs = inputs(*shape)
    eye = shift * np.eye(shape[1])
    G = gradients.xc_gradient_meta_spin_host(functional, dm_a - eye, dm_b - eye, ao, w, gr, hs)
    G.setflags(write=False)
    return G


def record(where, label, bar_rel, err_rel, what="max|G|"):
    """One line per measured case into uks_meta_gradient_parity.txt (kept sorted, one line per label) in the directory
    QCDFT_WRITE_PROFILES names -- how profiles/uks_meta_gradient_parity.txt was made; an ordinary test run writes nothing."""
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "uks_meta_gradient_parity.txt")
    key = f"{where:4s} {label:108s}"
    bar = "         " if bar_rel is None else f"{bar_rel:9.2e}"
    line = f"{key} reference bar / {what} {bar}   error / {what} {err_rel:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(key)]
        if not head:
            head = ["# Nuclear gradient of an open-shell meta-GGA: host against finite differences of metagga.xc_meta_spin_host's Exc and of the",
                    "# converged run_uks(meta=True) energy, device against host (tests/uks_meta_gradient_reference.py).  Written by",
                    "# tests/test_uks_meta_gradient_cpu.py (cpu) and tests/test_gpu_uks_meta_gradient.py (gpu) with QCDFT_WRITE_PROFILES=profiles.",
                    "# Finite-difference cases: error <= max(10 bar, 1e-9); 10 bar <= 1e-6 (planes), 1e-5 (whole gradient).  Device against host: 2e-8."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass


def check_fd(where, label, G, ref, bar, cap=1e-6):
    """meta_gradient_reference.check_fd's two assertions, figures printed and recorded (here) first."""
    scale = float(np.abs(ref).max())
    err = float(np.abs(np.asarray(G) - ref).max())
    print(f"{where} {label}: scale {scale:.3e}  bar {bar / scale:.2e}  err {err / scale:.2e}")
    record(where, label, bar / scale, err / scale)
    assert np.all(np.isfinite(G)), label
    assert 10.0 * bar <= cap * scale, (label, bar / scale)
    assert err <= max(10.0 * bar, 1e-9 * scale), (label, err / scale, bar / scale)
