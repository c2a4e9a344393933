"""What the linear response of Vxc costs against a ground-state sweep: DFT_FxcPrepare, DFT_FxcApply and DFT_ComputeXC
(GGA) at the Benzene/def2-SVP headline shape (143 556 points, 114 functions) and at 494 functions (the big path),
synthetic planes as bench.py makes them.  Same process, same buffers, the three calls ALTERNATING after a warm-up; each
timed with HIP events on the solver's stream (Prepare and Apply are asynchronous: a host clock would time the enqueue),
medians and the 10 / 90 % points; then the library's own per-kernel events.

The expectation to confirm or refute: Apply costs about one sweep (the same two passes over the planes), Prepare about
the density half of one plus the table.

usage: python tools/fxc_time.py [--reps 200] [--warmup 30] [--shapes 143556x114x21,60000x494x80]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import quantum_compute_dft_amd as q

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=200)
p.add_argument("--warmup", type=int, default=30)
p.add_argument("--shapes", default="143556x114x21,60000x494x80")
p.add_argument("--functional", default="GGA")
args = p.parse_args()

assert torch.cuda.is_available(), "fxc_time.py measures on the GPU (there is no CPU fallback)"
dev = torch.device("cuda:0")

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
    d_gr = gr if s.needs_gradient else None
    v, v1 = (torch.zeros((nao, nao), dtype=torch.float64, device=dev) for _ in range(2))
    calls = [("DFT_ComputeXC", lambda: s.compute_xc(ngrid, nao, dm, ao, w, v, d_gr)),
             ("DFT_FxcPrepare", lambda: s.fxc_prepare(ngrid, nao, dm, ao, w, d_gr)),
             ("DFT_FxcApply", lambda: s.fxc_apply(ngrid, nao, dm1, ao, v1, d_gr))]
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
    print(f"{args.functional}, ngrid {ngrid}, nao {nao}: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call")
    med = []
    for (name, _), e in zip(calls, ev):
        t = 1e3 * np.array([a.elapsed_time(b) for a, b in e])
        med.append(float(np.median(t)))
        print(f"  {name:15s} median {np.median(t):9.2f} us  p10 {np.percentile(t, 10):9.2f}  p90 {np.percentile(t, 90):9.2f}  {med[-1] / med[0]:6.3f} x DFT_ComputeXC")
    print("  per-kernel HIP events of the library (median of 30 calls, us):")
    s.set_option("profile", 1)
    for name, c in calls:
        acc = {}
        for _ in range(30):
            c()
            for k, ms in s.timings():
                acc.setdefault(k, []).append(ms)
        print(f"    {name:15s} " + "  ".join(f"{k} {1e3 * np.median(x):.2f}" for k, x in acc.items()))
    s.set_option("profile", 0)
    del ao, gr, s
    torch.cuda.empty_cache()
