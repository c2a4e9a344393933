"""What the meta-GGA sweep (DFT_ComputeXCMeta, TPSS) costs against the GGA one (DFT_ComputeXC, dm form), stage by stage,
and which form of the tau term of the potential is faster: k_vxc_tau (option "meta_fused" = 1) or three runs of the
sweep's contraction (0).  The only decision these times make is the default of "meta_fused".

One process, synthetic planes as bench.py makes them, at the Benzene/def2-SVP headline shape (143 556 points, 114
functions) and at 60 000 x 494.  The three calls ALTERNATE after a warm-up; each is timed with HIP events on the solver's
stream, medians and the 10 / 90 % points; then the library's own per-stage events (DFT_GetTimings: "tau", "xc_points_meta",
"vxc_tau" beside the sweep's "rho", "vxc", "reduce_vxc"; in the plain form the three contractions appear as "fxc_vxc" /
"fxc_reduce"), and the new kernels' register and occupancy lines from lib/libdft.so.resources.json.

The expectation to confirm or refute: tau and the tau term are three products each where the GGA stage is one, so the
call should land near 3-4 x the GGA sweep.  All calls are synchronous, so an event pair brackets the call's kernels and
the host's wait for Exc.

usage: python tools/meta_time.py [--reps 30] [--warmup 10] [--shapes 143556x114x21,60000x494x80] [--out profiles/meta_time.txt]"""
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
p.add_argument("--reps", type=int, default=30)
p.add_argument("--warmup", type=int, default=10)
p.add_argument("--shapes", default="143556x114x21,60000x494x80")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_time.txt"), help="the report goes here too")
args = p.parse_args()
assert args.reps >= 20, "medians of at least 20"

assert torch.cuda.is_available(), "meta_time.py measures on the GPU (there is no CPU fallback)"
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def solver(functional, **opts):
    s = q.DFTSolverWrapper(q.library_path(), functional)
    for k, v in dict(graph=0, quirks=0, occ=2, **opts).items():
        s.set_option(k, v)
    return s


for shape in args.shapes.split(","):
    ngrid, nao, nocc = (int(x) for x in shape.split("x"))
    g = torch.Generator(device=dev); g.manual_seed(20260128)          # bench.py's synth()
    ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
    C = 0.7 * torch.randn((nao, nocc), dtype=torch.float64, device=dev, generator=g)
    dm = (2.0 * C @ C.T).contiguous()
    gga, fused, plain = solver("GGA"), solver("TPSS", meta_fused=1), solver("TPSS", meta_fused=0)
    v = [torch.zeros((nao, nao), dtype=torch.float64, device=dev) for _ in range(3)]
    calls = [("DFT_ComputeXC GGA", gga, lambda: gga.compute_xc(ngrid, nao, dm, ao, w, v[0], gr)),
             ("DFT_ComputeXCMeta TPSS, k_vxc_tau", fused, lambda: fused.compute_xc_meta(ngrid, nao, dm, ao, w, v[1], gr)),
             ("DFT_ComputeXCMeta TPSS, plain", plain, lambda: plain.compute_xc_meta(ngrid, nao, dm, ao, w, v[2], gr))]
    for _ in range(args.warmup):
        for _, _, c in calls:
            c()
    torch.cuda.synchronize()
    dv = float((v[1] - v[2]).abs().max() / v[2].abs().max())
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)] for _ in calls]
    for r in range(args.reps):                                        # alternating: drift and neighbours hit all calls alike
        for i, (_, _, c) in enumerate(calls):
            ev[i][r][0].record()
            c()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    say(f"ngrid {ngrid}, nao {nao}: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call "
        f"(the two forms of V differ by {dv:.1e} of max|V|)")
    med = []
    for (name, _, _), e in zip(calls, ev):
        t = 1e3 * np.array([a.elapsed_time(b) for a, b in e])
        med.append(float(np.median(t)))
        say(f"  {name:36s} median {np.median(t):10.2f} us  p10 {np.percentile(t, 10):10.2f}  p90 {np.percentile(t, 90):10.2f}")
    say(f"  meta / GGA {med[1] / med[0]:.2f} (k_vxc_tau)  {med[2] / med[0]:.2f} (plain);  k_vxc_tau form / plain form of the whole call {med[1] / med[2]:.3f}")
    say(f"  per-stage HIP events of the library (median of {args.reps} calls, alternating, us):")
    stage = {}
    for _, s, _ in calls:
        s.set_option("profile", 1)
    for _ in range(args.reps):
        for name, s, c in calls:
            c()
            for i, (k, ms) in enumerate(s.timings(32)):
                stage.setdefault(name, {}).setdefault((i, k), []).append(ms)
    tot = {}
    for name, _, _ in calls:
        tot[name] = {}
        for (_, k), x in stage[name].items():
            tot[name][k] = tot[name].get(k, 0.0) + 1e3 * float(np.median(x))
        say(f"    {name:36s} " + "  ".join(f"{k} {t:.2f}" for k, t in tot[name].items()))
    f, pl, gg = tot[calls[1][0]], tot[calls[2][0]], tot[calls[0][0]]
    tau_plain = pl.get("fxc_vxc", 0.0) + pl.get("fxc_reduce", 0.0)
    if f.get("vxc_tau") and tau_plain:
        say(f"  tau term of the potential: k_vxc_tau {f['vxc_tau']:.2f} us, plain form {tau_plain:.2f} us (three contractions and reduces; "
            f"the three adds are outside the stage events): ratio {f['vxc_tau'] / tau_plain:.3f}")
    if gg.get("rho") and f.get("tau"):
        say(f"  k_tau {f['tau']:.2f} us = {f['tau'] / gg['rho']:.2f} x the GGA density stage ({gg['rho']:.2f} us: rho and its gradient, four products); "
            f"pointwise {f.get('xc_points_meta', 0.0):.2f} us against {gg.get('xc_points', 0.0):.2f} us")
    del ao, gr, gga, fused, plain
    torch.cuda.empty_cache()

try:
    res = json.load(open(RESOURCES_PATH))
    for name, r in sorted(res.items()):
        if any(k in name for k in ("k_tau", "k_xc_points_meta", "k_vxc_tau")):
            say(f"{name.split('(')[0]}: {r['vgprs']} VGPRs, scratch {r['scratch']} bytes/lane, occupancy {r['occupancy']} waves/SIMD, LDS {r['lds']} bytes (static)")
except OSError:
    say("no resource report beside the library")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
