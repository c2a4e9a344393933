"""Times of the XC gradient kernels next to the sweep's, and of the host derivative integrals.

DFT_ComputeXCGradient and DFT_EvalAOHess against DFT_ComputeXC and DFT_EvalAO, alternating in ONE process, HIP events
around each call (as tools/triplet_time.py measures): the Benzene/def2-SVP shape (143 556 x 114, real shells and grid)
and 60 000 x 494 (Anthracene/def2-TZVP shells, the first 60 000 points of its grid).  Then the wall time of
integrals.grad2e / grad1e for Benzene/def2-SVP on the threads given.  Prints lines for profiles/xc_gradient_time.txt;
no threshold: a record.  Last, the two-electron term on the device (integrals.DeviceGrad2e.grad: upload, DFT_Grad2e, the
rows back, synchronised) against integrals.grad2e on the same D in the same process: warm, alternating, medians of --reps
wall times, and the largest per-atom difference between the two (lines for profiles/grad2e_time.txt).

    python tools/gradient_time.py [--reps 7] [--threads 16] [--skip-host] [--skip-xc]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-xc", action="store_true", help="only the derivative integrals: host, and device against host")
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

    for mol, bname, cap in () if args.skip_xc else (("Benzene", "def2-svp", None), ("Anthracene", "def2-tzvp", 60000)):
        path = os.path.join(inputs.DATA_DIR, mol + ".xyz")
        syms, xyz = basis.parse_xyz(path)
        sh = basis.build_shells(syms, xyz, bname)
        grids = grid_gen.Grids(syms, xyz, level=3)
        coords, w = np.asarray(grids.coords), np.asarray(grids.weights)
        if cap:
            coords, w = coords[:cap], w[:cap]
        ng, n = len(coords), sh.nao
        rng = np.random.default_rng(1)
        C = rng.standard_normal((n, max(1, n // 5)))
        C /= np.linalg.norm(C, axis=0)
        d_dm = torch.as_tensor(2.0 * C @ C.T, device=dev)
        d_c, d_w = torch.as_tensor(np.ascontiguousarray(coords), device=dev), torch.as_tensor(np.ascontiguousarray(w), device=dev)
        d_ao = torch.empty((ng, n), dtype=torch.float64, device=dev)
        d_gr = torch.empty((3, ng, n), dtype=torch.float64, device=dev)
        d_hs = torch.empty((6, ng, n), dtype=torch.float64, device=dev)
        d_v = torch.empty((n, n), dtype=torch.float64, device=dev)
        d_g = torch.empty((n, 3), dtype=torch.float64, device=dev)
        for functional in ("LDA", "GGA", "B3LYP"):
            s = q.DFTSolverWrapper(library_path(), functional)
            gga = functional != "LDA"
            calls = {
                "DFT_EvalAO (4 planes)": lambda: s.eval_ao(sh, d_c, ng, d_ao, d_gr),
                "DFT_EvalAOHess (6 planes)": lambda: s.eval_ao_hess(sh, d_c, ng, d_hs),
                "DFT_ComputeXC": lambda: s.compute_xc(ng, n, d_dm, d_ao, d_w, d_v, d_gr if gga else None),
                "DFT_ComputeXCGradient": lambda: s.compute_xc_gradient(ng, n, d_dm, d_ao, d_w, d_g, d_gr, d_hs if gga else None),
            }
            for fn in calls.values():      # warm-up: allocations, shell-table upload
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in calls}
            for _ in range(args.reps):      # alternating, so that clocks and cache state are shared
                for k, fn in calls.items():
                    ms[k].append(timed(fn))
            for k, v in ms.items():
                if functional != "GGA" and k.startswith("DFT_EvalAO"):
                    continue
                print(f"{mol}/{bname} {ng} x {n} {functional:5s} {k:28s} median {np.median(v) * 1e3:9.1f} us   min {min(v) * 1e3:9.1f} us   ({args.reps} reps)")
            del s
    if not args.skip_host:
        integrals.set_threads(args.threads)
        syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
        sh = basis.build_shells(syms, xyz, "def2-svp")
        rng = np.random.default_rng(2)
        C = rng.standard_normal((sh.nao, 21))
        D = 2.0 * C @ C.T
        z = np.array([basis.atomic_number(s) for s in syms], dtype=np.float64)
        t0 = time.time(); integrals.grad1e(sh, xyz, z, D, D); t1 = time.time()
        integrals.grad2e(sh, D, 0.2); t2 = time.time()
        integrals.int2e(sh); t3 = time.time()
        print(f"Benzene/def2-svp host, {args.threads} threads: qc_grad1e {t1 - t0:.3f} s   qc_grad2e (c_hf 0.2) {t2 - t1:.3f} s   qc_int2e (for scale) {t3 - t2:.3f} s")
        eng = integrals.DeviceGrad2e(sh)
        g_dev = eng.grad(D, 0.2)                    # warm-up: the LDS attribute, the first launches
        torch.cuda.synchronize()
        host_s, dev_s = [], []
        for _ in range(args.reps):                  # alternating; DeviceGrad2e.grad ends with the copy of the rows to the host
            t0 = time.perf_counter(); g_host = integrals.grad2e(sh, D, 0.2); t1 = time.perf_counter()
            g_dev = eng.grad(D, 0.2); torch.cuda.synchronize(); t2 = time.perf_counter()
            host_s.append(t1 - t0); dev_s.append(t2 - t1)
        d_D = torch.as_tensor(D, device=dev)
        kern = [timed(lambda: eng.per_shell(d_D, 0.2)) for _ in range(args.reps)]      # the kernels alone, HIP events
        h, d = float(np.median(host_s)), float(np.median(dev_s))
        print(f"Benzene/def2-svp grad2e (c_hf 0.2), same D, same process, {args.reps} alternating reps: host qc_grad2e ({args.threads} threads) median {h:.3f} s "
              f"(min {min(host_s):.3f})   device DeviceGrad2e.grad median {d * 1e3:.2f} ms (min {min(dev_s) * 1e3:.2f})   host / device {h / d:.1f}")
        print(f"Benzene/def2-svp DFT_Grad2e kernels alone (HIP events): median {np.median(kern):.2f} ms   min {min(kern):.2f} ms")
        print(f"Benzene/def2-svp grad2e largest per-atom |device - host| {np.abs(g_dev - g_host).max():.2e} (max|host| {np.abs(g_host).max():.2e})")
        eng.close()


if __name__ == "__main__":
    main()
