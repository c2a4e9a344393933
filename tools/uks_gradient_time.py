"""Times of the two open-shell gradient entries next to their closed-shell counterparts, alternating in ONE process, HIP
events around each call (as tools/gradient_time.py measures).

* DFT_Grad2eSpin against DFT_Grad2e at Benzene/def2-SVP (c_hf 0.2): the same pass over the derivative integrals with a
  wider gather, so parity is the expectation.  Lines for profiles/grad2e_spin_time.txt.
* DFT_ComputeXCGradientSpin at the Benzene/def2-SVP shape (143 556 x 114, real shells and grid) and at 60 000 x 494
  (Anthracene/def2-TZVP shells, the first 60 000 points of its grid), three ways alternating: one k_xc_grad launch (the default,
  one kernel for both spins), k_xc_grad once per spin (option xcg_spin_fused = 0), and the closed-shell
  DFT_ComputeXCGradient of the total density for scale.  The line "fused / two launches" also gives the run-to-run spread
  of the two launches in this very measurement, (max - min) / median: the yardstick for "faster".  Lines for
  profiles/xc_gradient_spin_time.txt.  No threshold: a record.

    python tools/uks_gradient_time.py [--reps 7] [--skip-xc] [--skip-2e]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-xc", action="store_true")
    ap.add_argument("--skip-2e", action="store_true")
    args = ap.parse_args()
    import torch
    import quantum_compute_dft_amd as q
    from quantum_compute_dft_amd import basis, grid_gen, inputs, integrals
    from quantum_compute_dft_amd.build import library_path
    dev = torch.device("cuda:0")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b)

    def report(head, calls, unit=1e3, name="us"):
        for fn in calls.values():      # warm-up: allocations, LDS attributes, the first launches
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(args.reps):      # alternating, so that clocks and cache state are shared
            for k, fn in calls.items():
                ms[k].append(timed(fn))
        for k, v in ms.items():
            print(f"{head} {k:28s} median {np.median(v) * unit:9.1f} {name}   min {min(v) * unit:9.1f} {name}   max {max(v) * unit:9.1f} {name}   ({args.reps} reps)")
        return {k: (float(np.median(v)), (max(v) - min(v)) / float(np.median(v))) for k, v in ms.items()}

    if not args.skip_2e:
        syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
        sh = basis.build_shells(syms, xyz, "def2-svp")
        rng = np.random.default_rng(2)
        Ca, Cb = rng.standard_normal((sh.nao, 21)), rng.standard_normal((sh.nao, 20))
        Da, Db = Ca @ Ca.T, Cb @ Cb.T
        d_D, d_M = torch.as_tensor(Da + Db, device=dev), torch.as_tensor(Da - Db, device=dev)
        eng = integrals.DeviceGrad2e(sh)
        m = report("Benzene/def2-svp c_hf 0.2", {"DFT_Grad2e": lambda: eng.per_shell(d_D, 0.2),
                                               "DFT_Grad2eSpin": lambda: eng.per_shell_spin(d_D, d_M, 0.2)}, 1.0, "ms")
        print(f"Benzene/def2-svp DFT_Grad2eSpin / DFT_Grad2e (medians): {m['DFT_Grad2eSpin'][0] / m['DFT_Grad2e'][0]:.3f}   "
              f"spread of DFT_Grad2e (max - min) / median: {m['DFT_Grad2e'][1]:.3f}")
        ref = integrals.grad2e_spin(sh, Da + Db, Da - Db, 0.2)
        got = eng.grad_spin(Da + Db, Da - Db, 0.2)
        print(f"Benzene/def2-svp grad2e_spin largest per-atom |device - host| {np.abs(got - ref).max():.2e} (max|host| {np.abs(ref).max():.2e})")
        eng.close()

    for mol, bname, cap in () if args.skip_xc else (("Benzene", "def2-svp", None), ("Anthracene", "def2-tzvp", 60000)):
        syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, mol + ".xyz"))
        sh = basis.build_shells(syms, xyz, bname)
        grids = grid_gen.Grids(syms, xyz, level=3)
        coords, w = np.asarray(grids.coords), np.asarray(grids.weights)
        if cap:
            coords, w = coords[:cap], w[:cap]
        ng, n = len(coords), sh.nao
        rng = np.random.default_rng(1)
        C = rng.standard_normal((n, max(2, n // 5)))
        C /= np.linalg.norm(C, axis=0)
        d_a, d_b = torch.as_tensor(C @ C.T, device=dev), torch.as_tensor(C[:, :-1] @ C[:, :-1].T, device=dev)
        d_dm = (d_a + d_b).contiguous()
        d_c, d_w = torch.as_tensor(np.ascontiguousarray(coords), device=dev), torch.as_tensor(np.ascontiguousarray(w), device=dev)
        d_ao = torch.empty((ng, n), dtype=torch.float64, device=dev)
        d_gr = torch.empty((3, ng, n), dtype=torch.float64, device=dev)
        d_hs = torch.empty((6, ng, n), dtype=torch.float64, device=dev)
        d_g = torch.empty((n, 3), dtype=torch.float64, device=dev)
        for functional in ("LDA", "GGA", "B3LYP"):
            s = q.DFTSolverWrapper(library_path(), functional)
            s.set_option("quirks", 0)
            gga = functional != "LDA"
            s.eval_ao(sh, d_c, ng, d_ao, d_gr)
            s.eval_ao_hess(sh, d_c, ng, d_hs)
            torch.cuda.synchronize()
            hs = d_hs if gga else None

            def spin(fused):
                s.set_option("xcg_spin_fused", fused)
                s.compute_xc_gradient_spin(ng, n, d_a, d_b, d_ao, d_w, d_g, d_gr, hs)

            head = f"{mol}/{bname} {ng} x {n} {functional:5s}"
            m = report(head, {"spin, one k_xc_grad launch": lambda: spin(1), "spin, k_xc_grad per spin": lambda: spin(0),
                              "DFT_ComputeXCGradient": lambda: s.compute_xc_gradient(ng, n, d_dm, d_ao, d_w, d_g, d_gr, hs)})
            one, two, closed = m["spin, one k_xc_grad launch"], m["spin, k_xc_grad per spin"], m["DFT_ComputeXCGradient"]
            print(f"{head} fused / two launches (medians): {one[0] / two[0]:.3f}   spread of the two launches (max - min) / median: {two[1]:.3f}   "
                  f"fused / closed shell: {one[0] / closed[0]:.3f}")
            del s


if __name__ == "__main__":
    main()
