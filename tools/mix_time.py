"""What a mix solver costs against the built-in GGA solver: DFT_ComputeXC at the Benzene/def2-SVP headline shape
(143 556 points, 114 functions, synthetic planes as bench.py makes them) for SOLVER_GGA, the PBE mix {pbe_x 1, pbe_c 1},
PBE0's {0.75 pbe_x, pbe_c 1}, and -- to show what the zero-weight skip saves -- a mix with all eight components.
Same process, same buffers, the solvers ALTERNATING call by call after a warm-up; medians and the 10 / 90 % points
of the per-call wall times (host clock around a call that returns after the device has published Exc), then the
library's own per-kernel HIP events.  Baseline = the built-in GGA solver of this same run.

usage: python tools/mix_time.py [--reps 400] [--warmup 50] [--ngrid 143556] [--nao 114]
Under `rocprofv3 --kernel-trace --stats -- python tools/mix_time.py --reps 100` the two pointwise kernels
(k_xc_points<1> and k_xc_points_mix<true>) appear in the kernel statistics; take wall times from a run without the profiler."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import quantum_compute_dft_amd as q
from quantum_compute_dft_amd.functionals import COMPONENTS, Functional

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=400)
p.add_argument("--warmup", type=int, default=50)
p.add_argument("--ngrid", type=int, default=143556)
p.add_argument("--nao", type=int, default=114)
args = p.parse_args()

assert torch.cuda.is_available(), "mix_time.py measures on the GPU (there is no CPU fallback)"
dev = torch.device("cuda:0")
ngrid, nao, nocc = args.ngrid, args.nao, 21
g = torch.Generator(device=dev); g.manual_seed(20260128)          # bench.py's synth()
ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
C = 0.7 * torch.randn((nao, nocc), dtype=torch.float64, device=dev, generator=g)
dm = (2.0 * C @ C.T).contiguous()


def mix(name, **wts):
    return q.DFTSolverWrapper(q.library_path(), Functional(name, {k: float(v) for k, v in wts.items()}, 0.0, None))


solvers = [("GGA built-in", q.DFTSolverWrapper(q.library_path(), "GGA")),
           ("PBE mix", mix("pbe-mix", pbe_x=1, pbe_c=1)),
           ("PBE0 mix", mix("pbe0-mix", pbe_x=0.75, pbe_c=1)),
           ("all eight", mix("all", **{c: 0.125 for c in COMPONENTS}))]
vs = [torch.zeros((nao, nao), dtype=torch.float64, device=dev) for _ in solvers]
calls = [lambda s=s, v=v: s.compute_xc(ngrid, nao, dm, ao, w, v, gr) for (_, s), v in zip(solvers, vs)]

exc = [None] * len(solvers)
for _ in range(args.warmup):
    for i, c in enumerate(calls):
        exc[i] = c()
torch.cuda.synchronize()
times = [[] for _ in solvers]
for _ in range(args.reps):                                        # alternating: drift and neighbours hit every solver alike
    for i, c in enumerate(calls):
        t0 = time.perf_counter()
        c()
        times[i].append(time.perf_counter() - t0)
torch.cuda.synchronize()

print(f"DFT_ComputeXC, ngrid {ngrid}, nao {nao}, {args.reps} alternating calls each after {args.warmup} warm-up calls; wall time per call")
base = float(np.median(times[0]))
for (name, s), t, e in zip(solvers, times, exc):
    t = 1e6 * np.array(t)
    print(f"  {name:13s} median {np.median(t):8.2f} us  p10 {np.percentile(t, 10):8.2f}  p90 {np.percentile(t, 90):8.2f}  "
          f"{np.median(t) / (1e6 * base):6.3f} x GGA built-in   Exc {e:.12f}")
d = (vs[1] - vs[0]).abs().max().item() / vs[0].abs().max().item()
print(f"  PBE mix against GGA built-in: |dExc|/|Exc| {abs(exc[1] - exc[0]) / abs(exc[0]):.2e}, max|dV|/max|V| {d:.2e}")

print("per-kernel HIP events of the library (median of 50 calls, us):")
for name, s in solvers:
    s.set_option("profile", 1)
for _ in range(5):
    for c in calls:
        c()
acc = [{} for _ in solvers]
for _ in range(50):
    for i, ((name, s), c) in enumerate(zip(solvers, calls)):
        c()
        for k, ms in s.timings():
            acc[i].setdefault(k, []).append(ms)
for (name, s), a in zip(solvers, acc):
    print(f"  {name:13s} " + "  ".join(f"{k} {1e3 * np.median(x):.2f}" for k, x in a.items()))
