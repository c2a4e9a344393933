"""What the triplet (spin-flip) response costs against the singlet one.

Part 1, kernels: DFT_FxcPrepareSpin (kind 1) against DFT_FxcPrepare and DFT_FxcApplyKind (kind 1) against DFT_FxcApply
(GGA) at the Benzene/def2-SVP headline shape (143 556 points, 114 functions) and at 494 functions, synthetic planes as
bench.py makes them.  Same process, same buffers, the four calls ALTERNATING after a warm-up; each timed with HIP events
on the solver's stream, medians and the 10 / 90 % points; then the library's own per-kernel events.

Part 2, whole driver (--driver): `dft.py B3LYP Benzene --basis def2-svp --eri cholesky --quirks 0 --excitations 5` with and
without --triplets, alternating child processes, wall time of each and the excitation section's share as the log prints it.

The expectation to confirm or refute: Apply costs what the singlet Apply costs (the same kernels); Prepare costs the
singlet Prepare plus the difference of the two table kernels -- four second-order evaluations of the energy, one launch
each, against two first-order evaluations of the potentials in one launch.

usage: python tools/triplet_time.py [--reps 200] [--warmup 30] [--shapes 143556x114x21,60000x494x80] [--driver] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import quantum_compute_dft_amd as q

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=200)
p.add_argument("--warmup", type=int, default=30)
p.add_argument("--shapes", default="143556x114x21,60000x494x80")
p.add_argument("--functional", default="GGA")
p.add_argument("--driver", action="store_true", help="also time the whole driver with and without --triplets")
p.add_argument("--driver-reps", type=int, default=3)
p.add_argument("--out", default=None, help="also write the report to this file")
args = p.parse_args()

assert torch.cuda.is_available(), "triplet_time.py measures on the GPU (there is no CPU fallback)"
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


for shape in args.shapes.split(","):
    ngrid, nao, nocc = (int(x) for x in shape.split("x"))
    g = torch.Generator(device=dev); g.manual_seed(20260128)          # bench.py's synth()
    ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
    C = 0.7 * torch.randn((nao, nocc), dtype=torch.float64, device=dev, generator=g)
    dm = (2.0 * C @ C.T).contiguous()
    a = torch.randn((nao, nao), dtype=torch.float64, device=dev, generator=g)
    dm1 = (0.01 * (a + a.T)).contiguous()
    s = q.DFTSolverWrapper(q.library_path(), args.functional)
    s.set_option("graph", 0)
    s.set_option("quirks", 0)
    d_gr = gr if s.needs_gradient else None
    v1, v2 = (torch.zeros((nao, nao), dtype=torch.float64, device=dev) for _ in range(2))
    calls = [("DFT_FxcPrepare", lambda: s.fxc_prepare(ngrid, nao, dm, ao, w, d_gr)),
             ("DFT_FxcPrepareSpin(1)", lambda: s.fxc_prepare_spin(ngrid, nao, dm, ao, w, d_gr, kind=1)),
             ("DFT_FxcApply", lambda: s.fxc_apply(ngrid, nao, dm1, ao, v1, d_gr)),
             ("DFT_FxcApplyKind(1)", lambda: s.fxc_apply_kind(ngrid, nao, dm1, ao, v2, d_gr, kind=1))]
    for _ in range(args.warmup):
        for _, c in calls:
            c()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for _ in calls]
    for r in range(args.reps):                                        # alternating: drift and neighbours hit every call alike
        for i, (_, c) in enumerate(calls):
            ev[i][r][0].record()
            c()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    say(f"{args.functional}, ngrid {ngrid}, nao {nao}: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call")
    med = []
    for (name, _), e in zip(calls, ev):
        t = 1e3 * np.array([a.elapsed_time(b) for a, b in e])
        med.append(float(np.median(t)))
        say(f"  {name:22s} median {np.median(t):9.2f} us  p10 {np.percentile(t, 10):9.2f}  p90 {np.percentile(t, 90):9.2f}")
    say(f"  Prepare: spin / singlet {med[1] / med[0]:.3f} (+{med[1] - med[0]:.2f} us);  Apply: kind 1 / singlet {med[3] / med[2]:.3f}")
    say("  per-kernel HIP events of the library (median of 30 calls, us):")
    s.set_option("profile", 1)
    for name, c in calls:
        acc = {}
        for _ in range(30):
            c()
            for k, ms in s.timings():
                acc.setdefault(k, []).append(ms)
        say(f"    {name:22s} " + "  ".join(f"{k} {1e3 * np.median(x):.2f}" for k, x in acc.items()))
    s.set_option("profile", 0)
    del ao, gr, s
    torch.cuda.empty_cache()

if args.driver:
    cmd = [sys.executable, "-m", "quantum_compute_dft_amd.dft", "B3LYP", "Benzene", "--basis", "def2-svp", "--eri", "cholesky",
           "--quirks", "0", "--excitations", "5"]
    wall = {"singlet": [], "triplet": []}
    for r in range(args.driver_reps):                                 # alternating child processes on the one card
        for name, extra in (("singlet", []), ("triplet", ["--triplets"])):
            t0 = time.time()
            run = subprocess.run(cmd + extra, cwd=ROOT, capture_output=True, text=True, timeout=900)
            wall[name].append(time.time() - t0)
            if run.returncode != 0:              # nothing more is started on the card after a failed run
                say(f"  driver {name} run failed with status {run.returncode}: {run.stdout[-500:]} {run.stderr[-500:]}")
                if args.out:
                    with open(args.out, "w") as fh:
                        fh.write("\n".join(lines) + "\n")
                sys.exit(1)
            if r == 0:
                for l in run.stdout.splitlines():
                    if "excitations (" in l or l.strip().startswith(("S", "T")) and "->" in l:
                        say("    " + l.strip())
    say("Whole driver, Benzene B3LYP/def2-SVP, Cholesky vectors, --excitations 5 (wall seconds per run, alternating): "
        + "; ".join(f"{k} {' '.join(f'{x:.2f}' for x in v)}" for k, v in wall.items()))

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
