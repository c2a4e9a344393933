"""What the XC force of a meta-GGA (DFT_ComputeXCGradientMeta, TPSS) costs in its two forms -- k_xc_grad_meta<true>, one pass
over the ten planes (option "xcg_meta_fused" = 1), and the plain form, k_xc_grad on c0..c3 plus k_xc_grad_meta<false> for
the tau term (0) -- beside the GGA force (DFT_ComputeXCGradient, PBE at quirks 0).  The only decision these times make is
the default of "xcg_meta_fused": 1 only if the fused form beats the plain one at both shapes by more than the alternation
spread (p90 - p10 of the plain form's own times).

The expectation, written down before the first measurement: the fused form reads the same ten planes as the GGA force,
does 5/2 of its MFMA work (five products per load of the matrix against two), and adds one tau stage (k_tau: three
products) and a dearer pointwise kernel (three Dual evaluations of the spin-resolved bodies).  The plain form reads the
three gradient planes and the six Hessian planes a second time and stages the gradient rows twice, so the fused form
should win where the planes come from HBM (143 556 x 114); at 60 000 x 494 the K loop dominates, both do the same five
products per tile, and the lower occupancy of the five-tile kernel (one workgroup of 160 KB LDS per CU against two or
three) may cost it the lead.

One process, synthetic planes as bench.py makes them and random Hessian planes, at the Benzene/def2-SVP headline shape
(143 556 points, 114 functions) and at 60 000 x 494.  The calls ALTERNATE after a warm-up; each is timed with HIP events
on the solver's stream, medians and the 10 / 90 % points; then the library's own per-stage events (DFT_GetTimings) and the
new kernels' register and occupancy lines from lib/libdft.so.resources.json.

usage: python tools/xc_gradient_meta_time.py [--reps 30] [--warmup 10] [--shapes 143556x114x21,60000x494x80] [--out profiles/xc_gradient_meta_time.txt]"""
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
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "xc_gradient_meta_time.txt"), help="the report goes here too")
args = p.parse_args()
assert args.reps >= 20, "medians of at least 20"

assert torch.cuda.is_available(), "xc_gradient_meta_time.py measures on the GPU (there is no CPU fallback)"
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


def timed(calls):
    """Medians (us) and p10 / p90 of alternating calls, HIP events."""
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
    out = []
    for (name, _), e in zip(calls, ev):
        t = 1e3 * np.array([a.elapsed_time(b) for a, b in e])
        out.append((float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))))
        say(f"  {name:52s} median {out[-1][0]:10.2f} us  p10 {out[-1][1]:10.2f}  p90 {out[-1][2]:10.2f}")
    return out


verdicts = []
for shape in args.shapes.split(","):
    ngrid, nao, nocc = (int(x) for x in shape.split("x"))
    g = torch.Generator(device=dev); g.manual_seed(20260128)          # bench.py's synth()
    ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
    C = 0.7 * torch.randn((nao, nocc), dtype=torch.float64, device=dev, generator=g)
    hs = 0.3 * torch.randn((6, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    dm = (2.0 * C @ C.T).contiguous()
    fused, plain, gga = solver("TPSS", xcg_meta_fused=1), solver("TPSS", xcg_meta_fused=0), solver("PBE")
    out = [torch.zeros((nao, 3), dtype=torch.float64, device=dev) for _ in range(3)]
    say(f"ngrid {ngrid}, nao {nao}, {nocc} orbitals: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call")
    calls = [("DFT_ComputeXCGradientMeta TPSS, k_xc_grad_meta<true>", fused, lambda: fused.compute_xc_gradient_meta(ngrid, nao, dm, ao, w, out[0], gr, hs)),
             ("DFT_ComputeXCGradientMeta TPSS, plain form", plain, lambda: plain.compute_xc_gradient_meta(ngrid, nao, dm, ao, w, out[1], gr, hs)),
             ("DFT_ComputeXCGradient PBE", gga, lambda: gga.compute_xc_gradient(ngrid, nao, dm, ao, w, out[2], gr, hs))]
    m = timed([(n, c) for n, _, c in calls])
    dg = float((out[0] - out[1]).abs().max() / out[1].abs().max())
    spread = m[1][2] - m[1][1]
    wins = m[0][0] < m[1][0] - spread
    verdicts.append(wins)
    say(f"  fused / plain {m[0][0] / m[1][0]:.3f}; the plain form's own spread (p90 - p10) {spread:.2f} us: the fused form "
        f"{'beats' if wins else 'does not beat'} it by more than that; the two forms of G differ by {dg:.1e} of max|G|")
    say(f"  meta / GGA force: fused {m[0][0] / m[2][0]:.2f}  plain {m[1][0] / m[2][0]:.2f}")
    say(f"  per-stage HIP events of the library (median of {args.reps} calls, alternating, us):")
    stage = {}
    for _, s, _ in calls:
        s.set_option("profile", 1)
    for _ in range(args.reps):
        for name, s, c in calls:
            c()
            torch.cuda.synchronize()
            for i, (k, ms) in enumerate(s.timings(64)):
                stage.setdefault(name, {}).setdefault((i, k), []).append(ms)
    for name, _, _ in calls:
        tot = {}
        for (_, k), x in stage[name].items():
            tot[k] = tot.get(k, 0.0) + 1e3 * float(np.median(x))
        say(f"    {name:52s} " + "  ".join(f"{k} {x:.2f}" for k, x in tot.items()))
    del ao, gr, hs, fused, plain, gga
    torch.cuda.empty_cache()

say(f"default of xcg_meta_fused by the rule: {1 if verdicts and all(verdicts) else 0}")
try:
    res = json.load(open(RESOURCES_PATH))
    for name, r in sorted(res.items()):
        if any(k in name for k in ("k_xc_grad_meta", "k_xc_edens_meta", "k_xc_grad<true, 1>")):
            say(f"{name.split('(')[0]}: {r['vgprs']} VGPRs, scratch {r['scratch']} bytes/lane, occupancy {r['occupancy']} waves/SIMD, LDS {r['lds']} bytes (static)")
except OSError:
    say("no resource report beside the library")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
