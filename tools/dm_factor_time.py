"""What option "dm_factor" costs and saves on the reference's call: the synchronous DFT_ComputeXC(dm) with the option at 0
and at 1, alternating in one process on one card, next to DFT_ComputeXCOcc with the true occupied orbitals, and the factor
kernels alone (HIP events of the library, DFT_GetTimings).  Synthetic planes (SURVEY 8(d) recipe, as tools/occ_time.py).
usage: python tools/dm_factor_time.py [--out FILE] [benzene|anthracene|c33 ...]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import quantum_compute_dft_amd as q

# config 5 (C33H56N7O17P3S, nao 1150, 250 occupied) at a tenth of its grid: the factorisation does not depend on the grid,
# the sweeps scale with it
SHAPES = {"benzene": ("GGA", 143556, 114, 21), "anthracene": ("B3LYP", 294868, 494, 47), "c33": ("B3LYP", 100000, 1150, 250),
          "h2o": ("LDA", 34310, 24, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table here (meant for profiles/dm_factor_time.txt)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("shapes", nargs="*", default=["benzene", "anthracene", "c33"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the GPU: there is nothing to measure without one"
    dev = torch.device("cuda:0")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# {torch.cuda.get_device_name(0)}; wall time per synchronous call (median of {args.rounds} interleaved rounds, [min, max]); events: median per call")
    for name in args.shapes:
        xc, ngrid, nao, nocc = SHAPES[name]
        g = torch.Generator(device=dev); g.manual_seed(1)
        ao = 0.4 * torch.randn((ngrid, nao), dtype=torch.float64, device=dev, generator=g)
        gr = 0.3 * torch.randn((3, ngrid, nao), dtype=torch.float64, device=dev, generator=g) if xc != "LDA" else None
        w = 0.05 * torch.rand((ngrid,), dtype=torch.float64, device=dev, generator=g)
        c = 0.7 * np.sqrt(2.0) * torch.randn((nao, nocc), dtype=torch.float64, device=dev, generator=g)
        dm = (c @ c.T).contiguous()
        v = torch.zeros((nao, nao), dtype=torch.float64, device=dev)
        solvers = {}
        for label, opt in (("dm_factor=0", 0), ("dm_factor=1", 1), ("XCOcc(cocc)", 0)):
            s = q.DFTSolverWrapper(q.library_path(), xc)
            s.set_option("dm_factor", opt)
            s.set_option("tiny", 0)
            solvers[label] = s
        calls = {"dm_factor=0": lambda: solvers["dm_factor=0"].compute_xc(ngrid, nao, dm, ao, w, v, gr),
                 "dm_factor=1": lambda: solvers["dm_factor=1"].compute_xc(ngrid, nao, dm, ao, w, v, gr),
                 "XCOcc(cocc)": lambda: solvers["XCOcc(cocc)"].compute_xc_occ(ngrid, nao, nocc, c, ao, w, v, gr, dm)}
        n = 50 if ngrid * nao < 3e7 else 8
        exc = {}
        for label, call in calls.items():               # warm-up: code objects, workspaces, clocks
            for _ in range(max(3, n // 2)):
                exc[label] = call()
        walls = {k: [] for k in calls}
        for _ in range(args.rounds):
            for label, call in calls.items():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(n):
                    call()
                torch.cuda.synchronize()
                walls[label].append((time.perf_counter() - t0) / n)
        s1 = solvers["dm_factor=1"]
        used, rank = int(s1.get_option("used_dm_factor")), int(s1.get_option("dm_factor_rank"))
        s1.set_option("profile", 1)
        acc = {}
        for _ in range(5):
            calls["dm_factor=1"]()
            for k, ms in s1.timings():
                acc.setdefault(k, []).append(ms)
        s1.set_option("profile", 0)
        say(f"{name}: {xc} ngrid {ngrid} nao {nao} nocc {nocc}; option 1 swept with the factor: {used}, rank found {rank}")
        for label in calls:
            t = 1e3 * np.array(walls[label])
            say(f"  {label:12s} {np.median(t):9.4f} ms  [{t.min():.4f}, {t.max():.4f}]   Exc {exc[label]:.12f}")
        say("  events of a dm_factor=1 call: " + "  ".join(f"{k} {1e3 * np.median(x):.1f}us" for k, x in acc.items()))
        del ao, gr, solvers, calls, s1
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
