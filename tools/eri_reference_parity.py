"""Worst |engine - reference| per family of tests/golden/eri_ref_z{1,2,3}.npz, for the host engine (csrc/integrals.c)
and, when a GPU is present, the device engine (csrc/eri_cols.hip): the figures of profiles/eri_reference_parity.txt.

    python tools/eri_reference_parity.py [> profiles/eri_reference_parity.txt]

The bound the tests hold both engines to is 1e-12 * max(1, max|ref| of the column block)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eri_fixtures as F  # noqa: E402
from quantum_compute_dft_amd import integrals  # noqa: E402


def main():
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        gpu = False
    rows = []

    def family(name, sh, blocks, n=None):
        """blocks: [((C, D), ref in the engines' layout over the first n functions)]"""
        n = n or sh.nao
        host = integrals.EriColumns(sh)
        q = integrals.schwarz_bounds(sh, host.diag())
        devc = integrals.DeviceEriColumns(sh, q) if gpu else None
        eh = ed = big = 0.0
        for (C, D), ref in blocks:
            eh = max(eh, np.abs(host.cols(C, D, 0.0, lower_only=True)[:, :n, :n] - ref).max())
            big = max(big, np.abs(ref).max())
            if gpu:
                buf = torch.full((ref.shape[0] * sh.nao ** 2,), 7.0, dtype=torch.float64, device="cuda:0")
                ed = max(ed, np.abs(devc.cols(C, D, 0.0, buf).cpu().numpy()[:, :n, :n] - ref).max())
        host.close()
        if gpu:
            devc.close()
        rows.append((name, len(blocks), big, eh, ed if gpu else float("nan")))

    f = F.z1()
    sh = f["sh"]
    for lc in range(4):
        for ld in range(4):
            blocks = [((C, D), F.z1_columns(C, D)) for C in range(sh.nshell) for D in range(C + 1)
                      if (int(sh.l[C]), int(sh.l[D])) == (lc, ld)]
            family("z1 ket class (%s%s|" % ("spdf"[lc], "spdf"[ld]), sh, blocks)
    for z in F.z2():
        family("z2 R = %g" % z["R"], z["sh"], list(zip(z["kets"], z["cols"])), n=16)
    z = F.z3()
    for k, name in zip(range(3), ("(f_C f_C|", "(d_C s_C|", "(p_H s_H|")):
        family("z3 ket " + name, z["sh"], [(z["kets"][k], z["cols"][k])])
    print("worst |engine - reference| per family (reference: oracle/eri_reference.py, 100 digits, rounded to double)")
    print("bound of the tests: 1e-12 * max(1, max|ref|); device: %s" % ("gfx950 (MI355X)" if gpu else "not measured (no GPU)"))
    print("%-24s %6s %10s %10s %10s" % ("family", "blocks", "max|ref|", "host", "device"))
    for r in rows:
        print("%-24s %6d %10.2e %10.2e %10.2e" % r)
    for fx, name in ((f, "z1"), (z, "z3")):
        got = integrals.int1e(fx["sh"], fx["syms"], fx["charge_xyz"])
        print("%s int1e (host)  " % name + "  ".join("%s: %.2e of %.2e" % (k, np.abs(g - fx[k]).max(), np.abs(fx[k]).max())
                                                      for g, k in zip(got, "STV")))


if __name__ == "__main__":
    main()
