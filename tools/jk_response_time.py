"""Batched response J/K from Cholesky vectors (DFT_ComputeJKFactorizedResponse) against what response_parts does per
trial today (one J call and two K calls of DFT_ComputeJKFactorized), alternating in one process on one card, on
synthetic symmetric vectors of the Benzene/def2-SVP and Anthracene/def2-TZVP shapes; with --driver also a whole
`--excitations 10` run of Benzene B3LYP/def2-SVP on Cholesky vectors.

    python tools/jk_response_time.py [--out FILE] [--driver] [shape substring]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd.hostinfo import blas_threads  # noqa: E402

SHAPES = [("benzene def2-SVP", 114, 1600, 21), ("anthracene def2-TZVP", 494, 4874, 47)]
ROUNDS = 7


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", nargs="?", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--driver", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    _pin = blas_threads(); _pin.__enter__()
    dev = torch.device("cuda:0")
    f64 = torch.float64
    say(f"# {torch.cuda.get_device_name(0)}; median of {ROUNDS} alternating rounds, wall clock around a synchronised call, ms")
    for name, nao, naux, nocc in SHAPES:
        if args.shape not in name:
            continue
        g = torch.Generator(device=dev); g.manual_seed(1)
        L = torch.randn((naux, nao, nao), dtype=f64, device=dev, generator=g) * 0.1
        for p0 in range(0, naux, 256):                                # symmetric like real vectors, slice by slice
            L[p0:p0 + 256] = 0.5 * (L[p0:p0 + 256] + L[p0:p0 + 256].transpose(1, 2))
        A = torch.randn((nao, nocc), dtype=f64, device=dev, generator=g)
        B = torch.randn((8, nao, nocc), dtype=f64, device=dev, generator=g)
        cp, cm = ((A[None] + B) / 2 ** 0.5).contiguous(), ((A[None] - B) / 2 ** 0.5).contiguous()
        AB = torch.matmul(A[None], B.transpose(1, 2))
        D = (AB + AB.transpose(1, 2)).contiguous()
        J = torch.zeros((8, nao, nao), dtype=f64, device=dev); M = torch.zeros_like(J)
        J1 = torch.zeros((nao, nao), dtype=f64, device=dev); K1 = torch.zeros_like(J1); K2 = torch.zeros_like(J1)
        s = q.DFTSolverWrapper(q.library_path(), "B3LYP")

        def new(nvec, want_m=True):
            s.compute_jk_factorized_response(nao, naux, nocc, nvec, L, A, B, J, M if want_m else None)

        def old(nvec, want_k=True):
            for k in range(nvec):
                s.compute_jk_factorized(nao, naux, 0, L, D[k], None, J1, None)
                if want_k:
                    s.compute_jk_factorized(nao, naux, nocc, L, None, cp[k], None, K1)
                    s.compute_jk_factorized(nao, naux, nocc, L, None, cm[k], None, K2)

        new(8); old(1)                                                # workspace and code objects
        # the two agree: K[D+] = M + M^T = K[c+ c+^T] - K[c- c-^T], J[D+]
        old(1); torch.cuda.synchronize()
        kerr = float(((M[0] + M[0].T) - (K1 - K2)).abs().max() / (K1 - K2).abs().max())
        jerr = float((J[0] - J1).abs().max() / J1.abs().max())
        say(f"{name}: nao {nao}, {naux} vectors ({8.0 * naux * nao * nao / 1e9:.2f} GB), nocc {nocc}; new against old: J {jerr:.1e}, K {kerr:.1e}")
        for want_k, label in ((True, "J and K"), (False, "J alone")):
            for nvec in (1, 4, 8):
                tn, to = [], []
                for _ in range(ROUNDS):
                    tn.append(timed(lambda: new(nvec, want_k)))
                    to.append(timed(lambda: old(nvec, want_k)))
                a, b = statistics.median(tn), statistics.median(to)
                say(f"   {label:8s} nvec {nvec}: batched entry {a:9.3f}   per-trial calls {b:9.3f}   ratio {b / a:5.2f}   "
                    f"(spread {min(tn):.3f}-{max(tn):.3f} / {min(to):.3f}-{max(to):.3f})")
        s.set_option("profile", 1)
        new(8); torch.cuda.synchronize()
        say("   stages at nvec 8: " + "  ".join(f"{k} {v:.3f}" for k, v in s.timings()))
        del L, s
        torch.cuda.empty_cache()
    if args.driver:
        cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "Benzene", "--basis", "def2-svp", "--eri", "cholesky",
               "--excitations", "10"]
        t0 = time.perf_counter()
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
        say(f"driver `{' '.join(cmd[2:])}`: exit {p.returncode}, {time.perf_counter() - t0:.1f} s in all")
        keep = False
        for ln in p.stdout.splitlines():
            keep = keep or ln.startswith("Singlet excitations")
            if ln.startswith("{"):
                keep = False
            if keep or ln.startswith(("Total Time", "excitations iteration")):
                say("   " + ln)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
