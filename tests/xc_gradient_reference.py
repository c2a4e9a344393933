"""Reference for the XC part of the nuclear gradient (TEST INFRASTRUCTURE: lives under tests/).

G[mu, x] is defined as d/dt of the Exc DFT_ComputeXC returns when, in column mu only, ao[:, mu] -> ao[:, mu] - t grad_x[:, mu]
and grad_k[:, mu] -> grad_k[:, mu] - t hess_xk[:, mu].  The reference is that derivative of the ORACLE's Exc -- never the
code under test -- by central differences at h and 2 h, Richardson-extrapolated:

    D(h) = (Exc(h) - Exc(-h)) / (2 h),   D_R = (4 D(h) - D(2 h)) / 3,   bar = max |D_R - D(h)|

Every comparison asserts |G - D_R| <= max(10 bar, 1e-9 scale) and 10 bar <= 1e-6 scale, scale = max |D_R|: the first is
the reference's own error with the margin the fxc tests give theirs, the second keeps the bound from hiding a missing
term (any term left out shows at 1e-3 or more).  H = 1e-4: the t^2 term of D(h) is then ~1e-8 of scale (planes of
order 0.3, so t moves a column by 3e-5 of its size) and the rounding of the difference quotient ~1e-11.

Inputs: helpers.synth_inputs planes and six random Hessian planes (0.3 N, a generator of their own, so the planes the
other tests share stay what they are).  `columns`: the columns of G a case differences -- all of them at nao = 24; at
nao = 114 the first and last two of the basis, both sides of every 16-column tile edge the kernels treat differently
(15/16, 111/112) and a spread in between, 14 columns x 3 directions (342 x 4 oracle sweeps would cost the suite 10 s per
functional and test the same formula).
"""
import functools
import os

import numpy as np

import oracle
from helpers import synth_inputs
from mix_reference import compute_xc_mix

H = 1e-4
TYPES = {"LDA": 0, "GGA": 1, "B3LYP": 2}
HESS_INDEX = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
COLUMNS = {24: tuple(range(24)), 114: (0, 1, 15, 16, 31, 40, 57, 64, 90, 101, 111, 112, 113, 77)}


@functools.lru_cache(maxsize=None)
def inputs(ngrid, nao):
    """(dm, ao, ao_grad (3, ngrid, nao), w, ao_hess (6, ngrid, nao)), read-only."""
    dm, ao, gr, w = synth_inputs(ngrid, nao)
    hs = 0.3 * np.random.default_rng(977 + 131 * nao + ngrid).standard_normal((6, ngrid, nao))
    for x in (dm, ao, gr, w, hs):
        x.setflags(write=False)
    return dm, ao, gr, w, hs


def _exc(functional, dm, ao, w, gr, quirks):
    if functional in TYPES:
        t = TYPES[functional]
        return oracle.compute_xc(t, dm, ao, w, gr if t else None, quirks=quirks)[0]
    return compute_xc_mix(functional, dm, ao, w, gr, quirks=quirks)[0]


@functools.lru_cache(maxsize=None)
def reference(functional, ngrid, nao, quirks):
    """(columns, D_R (len(columns), 3), bar) of `functional` ("LDA" / "GGA" / "B3LYP" by the oracle's solver types, anything
    else as a mix through mix_reference)."""
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
                    e.append(_exc(functional, dm, a, w, g, quirks))
                out[i, x] = (e[0] - e[1]) / (2.0 * h)
            a[:, mu] = ao[:, mu]
            g[:, :, mu] = gr[:, :, mu]
        D[h] = out
    ref = (4.0 * D[H] - D[2.0 * H]) / 3.0
    ref.setflags(write=False)
    return cols, ref, float(np.abs(ref - D[H]).max())


def record(where, label, bar_rel, err_rel, what="max|G|"):
    """One line per measured case into gradient_parity.txt (kept sorted, one line per label) in the directory
    QCDFT_WRITE_PROFILES names -- how profiles/gradient_parity.txt was made; an ordinary test run writes nothing."""
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "gradient_parity.txt")
    key = f"{where:4s} {label:62s}"
    bar = "         " if bar_rel is None else f"{bar_rel:9.2e}"
    line = f"{key} reference bar / {what} {bar}   error / {what} {err_rel:9.2e}"
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(key)]
        if not head:
            head = ["# XC part of the nuclear gradient: host and device against finite differences of the oracle and against each other",
                    "# (tests/xc_gradient_reference.py).  Written by tests/test_xc_gradient_cpu.py (cpu) and tests/test_gpu_xc_gradient.py (gpu).",
                    "# Finite-difference cases: error <= max(10 bar, 1e-9), 10 bar <= 1e-6.  Device against host: error <= 2e-8 (G), 1e-12 (planes)."]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass


def check_fd(where, label, G, ref, bar):
    """The two assertions of every finite-difference case, figures printed and recorded first."""
    scale = float(np.abs(ref).max())
    err = float(np.abs(np.asarray(G) - ref).max())
    print(f"{where} {label}: scale {scale:.3e}  bar {bar / scale:.2e}  err {err / scale:.2e}")
    record(where, label, bar / scale, err / scale)
    assert np.all(np.isfinite(G)), label
    assert 10.0 * bar <= 1e-6 * scale, (label, bar / scale)
    assert err <= max(10.0 * bar, 1e-9 * scale), (label, err / scale, bar / scale)
