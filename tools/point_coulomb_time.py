"""Times the three device calls of the point-Coulomb engine (DFT_PointCoulombMatrix / DFT_PointCoulombContract /
DFT_PointCoulombField) on the Benzene/def2-SVP shells (114 functions) at 1e3, 1e4 and 1e5 points, next to the host engine on
the same inputs.  The field call is also given relative to the contraction on the same points (the same kernel structure
with the Hermite table one order lower); the two are timed alternately.
Device: HIP events around one call, warm-up calls first, median of the repeats.  Host: wall time of
integrals.point_coulomb_matrix / point_coulomb_contract / point_coulomb_field at the CPU share of this process, at --host-points points (the
host time is linear in the point count; the count used is printed).
usage: python tools/point_coulomb_time.py [--out FILE] [--host-points N]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from quantum_compute_dft_amd import basis, inputs, integrals
from quantum_compute_dft_amd.hostinfo import host_cpu_share

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--host-points", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeat", type=int, default=11)
args = ap.parse_args()

lines = []
def say(s):
    print(s, flush=True)
    lines.append(s)

dev = torch.device("cuda:0")
syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
shells = basis.build_shells(syms, xyz, "def2-svp")
rng = np.random.default_rng(1)
D = rng.standard_normal((shells.nao, shells.nao)); D = D + D.T
pc = integrals.PointCoulomb(shells)
d_D = torch.as_tensor(D, device=dev)
say(f"Benzene/def2-SVP: {shells.nao} functions, {shells.nshell} shells; device {torch.cuda.get_device_name(0)}; "
    f"device times: HIP events, {args.warmup} warm-up calls, median of {args.repeat}; host: {host_cpu_share()} threads, wall, median of 3")


def device_ms(call):
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def host_ms(call):
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); call(); ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


for n in (1000, 10000, 100000):
    pts = rng.uniform(-10.0, 10.0, (n, 3)) + xyz.mean(axis=0)
    w = rng.uniform(-1.0, 1.0, n)
    d_p, d_w = torch.as_tensor(pts, device=dev), torch.as_tensor(w, device=dev)
    out_M = torch.empty((shells.nao, shells.nao), dtype=torch.float64, device=dev)
    out_u = torch.empty(n, dtype=torch.float64, device=dev)
    out_G = torch.empty((n, 3), dtype=torch.float64, device=dev)
    m = device_ms(lambda: pc.matrix(d_p, d_w, out=out_M))
    c = device_ms(lambda: pc.contract(d_p, d_D, out=out_u))
    f = device_ms(lambda: pc.field(d_p, d_D, out=out_G))
    c2 = device_ms(lambda: pc.contract(d_p, d_D, out=out_u))      # contraction again after the field: the spread between c and c2
    nh = min(n, args.host_points)
    hm = host_ms(lambda: integrals.point_coulomb_matrix(shells, pts[:nh], w[:nh]))
    hc = host_ms(lambda: integrals.point_coulomb_contract(shells, pts[:nh], D))
    hf = host_ms(lambda: integrals.point_coulomb_field(shells, pts[:nh], D))
    say(f"npts {n:7d}  device matrix {m[0]:9.3f} ms (min {m[1]:.3f}, max {m[2]:.3f})  contract {c[0]:9.3f} ms (min {c[1]:.3f}, max {c[2]:.3f})  |  "
        f"host at {nh} points: matrix {hm:9.1f} ms, contract {hc:9.1f} ms -> scaled to {n}: {hm * n / nh:10.1f} / {hc * n / nh:10.1f} ms")
    say(f"npts {n:7d}  device field  {f[0]:9.3f} ms (min {f[1]:.3f}, max {f[2]:.3f})  = {f[0] / c[0]:.2f} x contract (contract again afterwards: {c2[0]:.3f} ms)  |  "
        f"host at {nh} points: field {hf:9.1f} ms -> scaled to {n}: {hf * n / nh:10.1f} ms")
pc.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
