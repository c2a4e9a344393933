"""In-process A/B of solver options on the synchronous DFT_ComputeXC: one solver per setting, the same device inputs,
interleaved rounds (A B A B ...), median of the per-round means.  Synthetic planes (SURVEY 8(d) recipe).
usage: python tools/option_ab.py [publish] [vxc_fringe] ...   (each option is flipped 0 / 1 on its own, the others stay default)
Shapes: Benzene/def2-SVP (GGA, 114, 143556), nao 98 at the same grid, H2O/def2-SVP (LDA and GGA, 24, 34310; these replay a
recorded graph by default, so they are timed with graph = 0 as well)."""
import sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import quantum_compute_dft_amd as q

SHAPES = [("benzene", "GGA", 143556, 114, {}), ("nao98", "GGA", 143556, 98, {}),
          ("h2o_lda", "LDA", 34310, 24, {}), ("h2o_gga", "GGA", 34310, 24, {}),
          ("h2o_lda_nograph", "LDA", 34310, 24, {"graph": 0}), ("h2o_gga_nograph", "GGA", 34310, 24, {"graph": 0})]
ROUNDS, CALLS = 15, 100
dev = torch.device("cuda:0")
options = sys.argv[1:] or ["publish"]
for name, xc, ngrid, nao, fixed in SHAPES:
    g = torch.Generator(device=dev); g.manual_seed(1)
    ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
    gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g) if xc != "LDA" else None
    w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
    c = 0.7 * np.sqrt(2.0) * torch.randn((nao, max(1, nao // 5)), dtype=torch.float64, device=dev, generator=g)
    dm = (c @ c.T).contiguous()
    v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
    for opt in options:
        solvers = []
        for val in (0, 1):
            s = q.DFTSolverWrapper(q.library_path(), xc)
            for k, x in fixed.items():
                s.set_option(k, x)
            s.set_option(opt, val)
            solvers.append(s)
        call = lambda s: s.compute_xc(ngrid, nao, dm, ao, w, v, gr)
        t_end = time.perf_counter() + 0.08          # clock ramp, untimed
        while time.perf_counter() < t_end:
            for s in solvers:
                e = call(s)
        times, used, exc = ([], []), [None, None], [None, None]
        for r in range(ROUNDS):
            for i, s in enumerate(solvers):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(CALLS):
                    exc[i] = call(s)
                times[i].append((time.perf_counter() - t0) / CALLS)
                used[i] = s.get_option("used_" + opt)
        m = [1e6 * np.median(t) for t in times]
        lo = [1e6 * np.min(t) for t in times]
        hi = [1e6 * np.max(t) for t in times]
        print(f"{name:16s} {xc:4s} nao {nao:3d} ngrid {ngrid:6d}  {opt}=0: {m[0]:7.2f} us [{lo[0]:.2f}, {hi[0]:.2f}] (used {used[0]:.0f})   "
              f"{opt}=1: {m[1]:7.2f} us [{lo[1]:.2f}, {hi[1]:.2f}] (used {used[1]:.0f})   delta {m[1] - m[0]:+6.2f} us   "
              f"exc equal: {exc[0] == exc[1]}", flush=True)
        del solvers
    del ao, gr
    torch.cuda.empty_cache()
