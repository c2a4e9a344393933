"""What the open-shell response of Vxc (DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol) costs against the closed-shell one
(DFT_FxcPrepare / DFT_FxcApply), beside the ratio DFT_ComputeXCSpin / DFT_ComputeXC of the same run.

One process, synthetic planes as bench.py makes them, GGA at the Benzene/def2-SVP headline shape (143 556 points, 114
functions) and at 60 000 x 494.  After a warm-up the six calls ALTERNATE; each is bracketed by HIP events on the solver's
stream (the Apply and Prepare entries are asynchronous: the events time their kernels; the two sweeps are synchronous:
kernels and the host's wait for Exc), medians and the 10 / 90 % points; then the library's own per-kernel events of the two
new entries, and the register, occupancy and scratch lines of every new instantiation from lib/libdft.so.resources.json.

The expectations to confirm or refute: Apply is two density passes, two contraction passes and the coefficient kernel,
so about the ratio the two sweeps show in the same run, plus that kernel; Prepare is two density passes and 15 second-order
evaluations (and 10 copies) where the triplet table has 4.

usage: python tools/spin_response_time.py [--reps 100] [--warmup 20] [--shapes 143556x114x21,60000x494x80] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import quantum_compute_dft_amd as q
from quantum_compute_dft_amd.build import RESOURCES_PATH

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=100)
p.add_argument("--warmup", type=int, default=20)
p.add_argument("--shapes", default="143556x114x21,60000x494x80")
p.add_argument("--functional", default="GGA")
p.add_argument("--out", default=None, help="also write the report to this file")
args = p.parse_args()

assert torch.cuda.is_available(), "spin_response_time.py measures on the GPU (there is no CPU fallback)"
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
    Ca = 0.7 * torch.randn((nao, nocc), dtype=torch.float64, device=dev, generator=g)
    Cb = 0.7 * torch.randn((nao, max(nocc - 1, 1)), dtype=torch.float64, device=dev, generator=g)
    dm_a, dm_b = (Ca @ Ca.T).contiguous(), (Cb @ Cb.T).contiguous()
    dm = (dm_a + dm_b).contiguous()
    x = torch.randn((nao, nao), dtype=torch.float64, device=dev, generator=g)
    d1_a = (0.01 * (x + x.T)).contiguous()
    x = torch.randn((nao, nao), dtype=torch.float64, device=dev, generator=g)
    d1_b = (0.01 * (x + x.T)).contiguous()
    d1 = (d1_a + d1_b).contiguous()
    s = q.DFTSolverWrapper(q.library_path(), args.functional)
    s.set_option("graph", 0)
    s.set_option("quirks", 0)
    s.set_option("occ", 2)
    d_gr = gr if s.needs_gradient else None
    v, va, vb = (torch.zeros((nao, nao), dtype=torch.float64, device=dev) for _ in range(3))
    calls = [("DFT_ComputeXC", lambda: s.compute_xc(ngrid, nao, dm, ao, w, v, d_gr)),
             ("DFT_ComputeXCSpin", lambda: s.compute_xc_spin(ngrid, nao, dm_a, dm_b, ao, w, va, vb, d_gr)),
             ("DFT_FxcPrepare", lambda: s.fxc_prepare(ngrid, nao, dm, ao, w, d_gr)),
             ("DFT_FxcApply", lambda: s.fxc_apply(ngrid, nao, d1, ao, v, d_gr)),
             ("DFT_FxcPrepareSpinPol", lambda: s.fxc_prepare_spinpol(ngrid, nao, dm_a, dm_b, ao, w, d_gr)),
             ("DFT_FxcApplySpinPol", lambda: s.fxc_apply_spinpol(ngrid, nao, d1_a, d1_b, ao, va, vb, d_gr))]
    for _ in range(args.warmup):
        for _, c in calls:
            c()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for _ in calls]
    for r in range(args.reps):                                        # alternating: drift and neighbours hit all calls alike
        for i, (_, c) in enumerate(calls):
            ev[i][r][0].record()
            c()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    say(f"{args.functional}, ngrid {ngrid}, nao {nao}: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call")
    med = {}
    for (name, _), e in zip(calls, ev):
        t = 1e3 * np.array([a.elapsed_time(b) for a, b in e])
        med[name] = float(np.median(t))
        say(f"  {name:22s} median {np.median(t):9.2f} us  p10 {np.percentile(t, 10):9.2f}  p90 {np.percentile(t, 90):9.2f}")
    say(f"  DFT_ComputeXCSpin / DFT_ComputeXC      {med['DFT_ComputeXCSpin'] / med['DFT_ComputeXC']:.3f}")
    say(f"  DFT_FxcApplySpinPol / DFT_FxcApply     {med['DFT_FxcApplySpinPol'] / med['DFT_FxcApply']:.3f} (+{med['DFT_FxcApplySpinPol'] - med['DFT_FxcApply']:.2f} us)")
    say(f"  DFT_FxcPrepareSpinPol / DFT_FxcPrepare {med['DFT_FxcPrepareSpinPol'] / med['DFT_FxcPrepare']:.3f} (+{med['DFT_FxcPrepareSpinPol'] - med['DFT_FxcPrepare']:.2f} us)")
    say("  per-kernel HIP events of the library (median of 30 calls, us):")
    s.set_option("profile", 1)
    for name, c in calls[2:]:
        acc = {}
        for _ in range(30):
            c()
            for i, (k, ms) in enumerate(s.timings(32)):
                acc.setdefault((i, k), []).append(ms)
        say(f"    {name:22s} " + "  ".join(f"{k} {1e3 * np.median(t):.2f}" for (_, k), t in acc.items()))
    s.set_option("profile", 0)
    del ao, gr, s
    torch.cuda.empty_cache()

try:
    res = json.load(open(RESOURCES_PATH))
    for name, r in sorted(res.items()):
        if "k_fxc_table_pol" in name or "k_fxc_coef_pol" in name:
            say(f"{name.split('(')[0]}: {r['vgprs']} VGPRs, scratch {r['scratch']} bytes/lane, occupancy {r['occupancy']} waves/SIMD")
except OSError:
    say("no resource report beside the library")

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
