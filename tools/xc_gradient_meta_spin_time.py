"""What the XC force of an open-shell meta-GGA (DFT_ComputeXCGradientMetaSpin, TPSS) costs in its two forms --
k_xc_grad_meta_spin, both spins in one pass over the ten planes (option "xcg_meta_spin_fused" = 1), and the plain form, per
spin k_xc_grad on c0..c3 plus k_xc_grad_meta<false> for the tau term (0) -- beside the closed-shell meta force at the total
density (DFT_ComputeXCGradientMeta, TPSS at dm_a + dm_b) and the open-shell GGA force (DFT_ComputeXCGradientSpin, PBE at
quirks 0).  The only decision these times make is the default of "xcg_meta_spin_fused": 1 only if the fused form beats the
plain one at both shapes by more than the alternation spread (p90 - p10 of the plain form's own times).

One process, synthetic planes as bench.py makes them and random Hessian planes, at the Benzene/def2-SVP headline shape
(143 556 points, 114 functions) and at 60 000 x 494.  The calls ALTERNATE after a warm-up; each is timed with HIP events
on the solver's stream, medians and the 10 / 90 % points; then the library's own per-stage events (DFT_GetTimings) and the
kernels' register and occupancy lines from lib/libdft.so.resources.json.  The report opens with EXPECTATION below.

usage: python tools/xc_gradient_meta_spin_time.py [--reps 30] [--warmup 10] [--shapes 143556x114x21x20,60000x494x80x79] [--out profiles/xc_gradient_meta_spin_time.txt]"""
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

# Written down before the first measurement, from profiles/xc_gradient_meta_time.txt (closed shell), profiles/meta_spin_time.txt
# (tau and the pointwise kernel of two spins) and profiles/xc_gradient_spin_time.txt.
EXPECTATION = """\
Expectation, written before the first run (us; 143 556 x 114 | 60 000 x 494), from the closed-shell and spin files:
  density stage      twice the closed shell's rho (99.9 | 722.1) and sym_dm (6.3 | 6.5):                   ~212 | ~1457
  tau                as k_tau_spin measured (profiles/meta_spin_time.txt, tau_spin):                        ~590 | ~8570
  pointwise          k_xc_points_meta_spin as in profiles/meta_spin_time.txt:                               ~222 | ~130
  contraction, fused the same ten planes as k_xc_grad_meta<true> (1290 | 8482) and twice its MFMA work; six staged tiles
                     for ten products against five for five, two B loads per A read, but 164 VGPRs (occupancy 3 against 4)
                     and, at 494, 2.5 chunks of K = 160 against 2.4 of 208 with one workgroup per CU either way:
                     between 1.5 x and 2 x the closed shell's:                                       1940-2580 | 12700-17000
  contraction, plain the closed shell's plain pair (1504 | 12705) once per spin:                          ~3010 | ~25400
  whole call         fused: 1.4-1.9 x DFT_ComputeXCGradientMeta (1845 | 16275), i.e.                  2600-3500 | 22800-30900;
                     the sum of the stages above is 2960-3600 | 22860-27160
  so the fused form should beat the plain one at both shapes, by more at 494 where the plain form stages the gradient rows
  four times and reads D_s twice as often per product."""

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=30)
p.add_argument("--warmup", type=int, default=10)
p.add_argument("--shapes", default="143556x114x21x20,60000x494x80x79")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "xc_gradient_meta_spin_time.txt"), help="the report goes here too")
args = p.parse_args()
assert args.reps >= 20, "medians of at least 20"

assert torch.cuda.is_available(), "xc_gradient_meta_spin_time.py measures on the GPU (there is no CPU fallback)"
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
        say(f"  {name:58s} median {out[-1][0]:10.2f} us  p10 {out[-1][1]:10.2f}  p90 {out[-1][2]:10.2f}")
    return out


say(EXPECTATION)
verdicts = []
for shape in args.shapes.split(","):
    ngrid, nao, na, nb = (int(x) for x in shape.split("x"))
    g = torch.Generator(device=dev); g.manual_seed(20260128)          # bench.py's synth()
    ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
    C = 0.7 * torch.randn((nao, na), dtype=torch.float64, device=dev, generator=g)
    hs = 0.3 * torch.randn((6, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    dm_a, dm_b = (C @ C.T).contiguous(), (C[:, :nb] @ C[:, :nb].T).contiguous()
    dm = (dm_a + dm_b).contiguous()
    fused, plain = solver("TPSS", xcg_meta_spin_fused=1), solver("TPSS", xcg_meta_spin_fused=0)
    closed, gga = solver("TPSS"), solver("PBE")
    out = [torch.zeros((nao, 3), dtype=torch.float64, device=dev) for _ in range(4)]
    say(f"ngrid {ngrid}, nao {nao}, {na} + {nb} orbitals: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call")
    calls = [("DFT_ComputeXCGradientMetaSpin TPSS, k_xc_grad_meta_spin", fused,
              lambda: fused.compute_xc_gradient_meta_spin(ngrid, nao, dm_a, dm_b, ao, w, out[0], gr, hs)),
             ("DFT_ComputeXCGradientMetaSpin TPSS, plain form", plain,
              lambda: plain.compute_xc_gradient_meta_spin(ngrid, nao, dm_a, dm_b, ao, w, out[1], gr, hs)),
             ("DFT_ComputeXCGradientMeta TPSS at dm_a + dm_b", closed, lambda: closed.compute_xc_gradient_meta(ngrid, nao, dm, ao, w, out[2], gr, hs)),
             ("DFT_ComputeXCGradientSpin PBE", gga, lambda: gga.compute_xc_gradient_spin(ngrid, nao, dm_a, dm_b, ao, w, out[3], gr, hs))]
    m = timed([(n, c) for n, _, c in calls])
    dg = float((out[0] - out[1]).abs().max() / out[1].abs().max())
    spread = m[1][2] - m[1][1]
    wins = m[0][0] < m[1][0] - spread
    verdicts.append(wins)
    say(f"  fused / plain {m[0][0] / m[1][0]:.3f}; the plain form's own spread (p90 - p10) {spread:.2f} us: the fused form "
        f"{'beats' if wins else 'does not beat'} it by more than that; the two forms of G differ by {dg:.1e} of max|G|")
    say(f"  two spins / closed-shell meta force: fused {m[0][0] / m[2][0]:.2f}  plain {m[1][0] / m[2][0]:.2f};  "
        f"meta / GGA force of two spins: fused {m[0][0] / m[3][0]:.2f}  plain {m[1][0] / m[3][0]:.2f}")
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
        say(f"    {name:58s} " + "  ".join(f"{k} {x:.2f}" for k, x in tot.items()))
    del ao, gr, hs, fused, plain, closed, gga
    torch.cuda.empty_cache()

say(f"default of xcg_meta_spin_fused by the rule: {1 if verdicts and all(verdicts) else 0}")
try:
    res = json.load(open(RESOURCES_PATH))
    for name, r in sorted(res.items()):
        if any(k in name for k in ("k_xc_grad_meta", "k_xc_edens_meta", "k_xc_grad<true, 1>", "k_xc_grad<true, 2>")):
            say(f"{name.split('(')[0]}: {r['vgprs']} VGPRs, scratch {r['scratch']} bytes/lane, occupancy {r['occupancy']} waves/SIMD, LDS {r['lds']} bytes (static)")
except OSError:
    say("no resource report beside the library")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
