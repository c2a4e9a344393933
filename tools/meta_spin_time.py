"""What the spin-resolved meta-GGA sweep (DFT_ComputeXCMetaSpin, TPSS) costs against the closed-shell one
(DFT_ComputeXCMeta), stage by stage, and whether the two-spin tau kernel (k_tau_spin, option "tau_spin_fused" = 1) beats
k_tau once per spin (0).  The only decision these times make is the default of "tau_spin_fused": 1 only if it beats the two
launches at both shapes by more than the spread (p90 - p10) of the two launches' own times.

One process, synthetic planes as bench.py makes them, at the Benzene/def2-SVP headline shape (143 556 points, 114
functions) and at 60 000 x 494.  The calls ALTERNATE after a warm-up; each is timed with HIP events on the solver's
stream, medians and the 10 / 90 % points; then the tau stage alone (DFT_ComputeTauSpin in both forms, DFT_ComputeTau), the
library's own per-stage events (DFT_GetTimings), and the new kernels' register and occupancy lines from
lib/libdft.so.resources.json.

The expectations to confirm or refute: about 2 x the closed-shell meta call (every stage runs twice), and the pointwise
kernel about 7/3 of k_xc_points_meta (seven Dual evaluations against three).

usage: python tools/meta_spin_time.py [--reps 30] [--warmup 10] [--shapes 143556x114x21x20,60000x494x80x79] [--out profiles/meta_spin_time.txt]"""
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
p.add_argument("--shapes", default="143556x114x21x20,60000x494x80x79")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "meta_spin_time.txt"), help="the report goes here too")
args = p.parse_args()
assert args.reps >= 20, "medians of at least 20"

assert torch.cuda.is_available(), "meta_spin_time.py measures on the GPU (there is no CPU fallback)"
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
        say(f"  {name:44s} median {out[-1][0]:10.2f} us  p10 {out[-1][1]:10.2f}  p90 {out[-1][2]:10.2f}")
    return out


verdicts = []
for shape in args.shapes.split(","):
    ngrid, nao, na, nb = (int(x) for x in shape.split("x"))
    g = torch.Generator(device=dev); g.manual_seed(20260128)          # bench.py's synth()
    ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
    Ca = 0.7 * torch.randn((nao, na), dtype=torch.float64, device=dev, generator=g)
    Cb = 0.7 * torch.randn((nao, nb), dtype=torch.float64, device=dev, generator=g)
    da, db = (Ca @ Ca.T).contiguous(), (Cb @ Cb.T).contiguous()
    dm = (da + db).contiguous()
    closed, plain, fused = solver("TPSS"), solver("TPSS", tau_spin_fused=0), solver("TPSS", tau_spin_fused=1)
    v = [torch.zeros((nao, nao), dtype=torch.float64, device=dev) for _ in range(5)]
    t = [torch.zeros((ngrid,), dtype=torch.float64, device=dev) for _ in range(5)]
    say(f"ngrid {ngrid}, nao {nao}, {na} + {nb} orbitals: {args.reps} alternating calls each after {args.warmup} warm-up calls; HIP-event time per call")
    calls = [("DFT_ComputeXCMeta TPSS", lambda: closed.compute_xc_meta(ngrid, nao, dm, ao, w, v[0], gr)),
             ("DFT_ComputeXCMetaSpin TPSS, k_tau x 2", lambda: plain.compute_xc_meta_spin(ngrid, nao, da, db, ao, w, v[1], v[2], gr)),
             ("DFT_ComputeXCMetaSpin TPSS, k_tau_spin", lambda: fused.compute_xc_meta_spin(ngrid, nao, da, db, ao, w, v[3], v[4], gr))]
    m = timed(calls)
    dv = float(max((v[1] - v[3]).abs().max(), (v[2] - v[4]).abs().max()) / max(v[1].abs().max(), v[2].abs().max()))
    say(f"  spin / closed shell {m[1][0] / m[0][0]:.2f} (k_tau x 2)  {m[2][0] / m[0][0]:.2f} (k_tau_spin); the two forms of V differ by {dv:.1e} of max|V|")
    say("  the tau stage alone (asynchronous entries; the event pair brackets the kernels):")
    calls = [("DFT_ComputeTau (one spin)", lambda: closed.compute_tau(ngrid, nao, da, gr, t[0])),
             ("DFT_ComputeTauSpin, k_tau x 2", lambda: plain.compute_tau_spin(ngrid, nao, da, db, gr, t[1], t[2])),
             ("DFT_ComputeTauSpin, k_tau_spin", lambda: fused.compute_tau_spin(ngrid, nao, da, db, gr, t[3], t[4]))]
    m = timed(calls)
    spread = m[1][2] - m[1][1]
    wins = m[2][0] < m[1][0] - spread
    verdicts.append(wins)
    say(f"  k_tau_spin / two k_tau launches {m[2][0] / m[1][0]:.3f}; the two launches' own spread (p90 - p10) {spread:.2f} us: "
        f"k_tau_spin {'beats' if wins else 'does not beat'} them by more than that")
    say(f"  per-stage HIP events of the library (median of {args.reps} calls, alternating, us):")
    stage = {}
    calls = [("DFT_ComputeXCMeta TPSS", closed, lambda: closed.compute_xc_meta(ngrid, nao, dm, ao, w, v[0], gr)),
             ("DFT_ComputeXCMetaSpin TPSS, k_tau x 2", plain, lambda: plain.compute_xc_meta_spin(ngrid, nao, da, db, ao, w, v[1], v[2], gr)),
             ("DFT_ComputeXCMetaSpin TPSS, k_tau_spin", fused, lambda: fused.compute_xc_meta_spin(ngrid, nao, da, db, ao, w, v[3], v[4], gr))]
    for _, s, _ in calls:
        s.set_option("profile", 1)
    for _ in range(args.reps):
        for name, s, c in calls:
            c()
            for i, (k, ms) in enumerate(s.timings(64)):
                stage.setdefault(name, {}).setdefault((i, k), []).append(ms)
    tot = {}
    for name, _, _ in calls:
        tot[name] = {}
        for (_, k), x in stage[name].items():
            tot[name][k] = tot[name].get(k, 0.0) + 1e3 * float(np.median(x))
        say(f"    {name:44s} " + "  ".join(f"{k} {x:.2f}" for k, x in tot[name].items()))
    c0, c1 = tot[calls[0][0]], tot[calls[1][0]]
    if c0.get("xc_points_meta") and c1.get("xc_points_meta_spin"):
        say(f"  pointwise: k_xc_points_meta_spin {c1['xc_points_meta_spin']:.2f} us = {c1['xc_points_meta_spin'] / c0['xc_points_meta']:.2f} x "
            f"k_xc_points_meta ({c0['xc_points_meta']:.2f} us); expected about 7/3")
    del ao, gr, closed, plain, fused
    torch.cuda.empty_cache()

say(f"default of tau_spin_fused by the rule: {1 if verdicts and all(verdicts) else 0}")
try:
    res = json.load(open(RESOURCES_PATH))
    for name, r in sorted(res.items()):
        if any(k in name for k in ("k_tau", "k_xc_points_meta")):
            say(f"{name.split('(')[0]}: {r['vgprs']} VGPRs, scratch {r['scratch']} bytes/lane, occupancy {r['occupancy']} waves/SIMD, LDS {r['lds']} bytes (static)")
except OSError:
    say("no resource report beside the library")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
