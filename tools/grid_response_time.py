"""Times of the grid response of the nuclear gradient (lines for profiles/grid_response_time.txt; no threshold: a record).

1. The XC part of --gradient with and without --grid-response on Benzene B3LYP/def2-SVP (143 556 x 114, grid level 3, real
   shells and grid, a synthetic density matrix of 21 orbitals): scf.HipBackend.xc_gradient against xc_gradient +
   xc_grid_response, alternating in ONE process, wall time around each (both end synchronised, with their result on the
   host), and HIP events around the library calls the response adds on one atom block and on the whole grid.
2. DFT_BeckeWeightGradient alone, HIP events, at the Benzene grid (143 556 points x 12 atoms) and at the level-3 grid of
   C33H56N7O17P3S (about 1.44 M points x 117 atoms) with a synthetic f; beside it the forward pass of
   grid_gen.becke_weights in torch on the same card (wall time, its upload and download included).

    python tools/grid_response_time.py [--reps 5] [--skip-large]
"""
import argparse
import os
import sys
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bare_grid(syms, xyz, level):
    """(coords, owner, atomic weights) of the atomic grids, without the Becke partition."""
    from quantum_compute_dft_amd import basis, grid_gen
    pts, wts, own, cache = [], [], [], {}
    for ia, s in enumerate(syms):
        z = basis.atomic_number(s)
        if z not in cache:
            cache[z] = grid_gen.atomic_grid(z, level)
        p, w = cache[z]
        pts.append(p + xyz[ia]); wts.append(w); own.append(np.full(len(w), ia))
    return np.concatenate(pts), np.concatenate(own), np.concatenate(wts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    import torch
    import quantum_compute_dft_amd as q
    from quantum_compute_dft_amd import basis, grid_gen, inputs, integrals, scf
    from quantum_compute_dft_amd.build import library_path
    dev = torch.device("cuda:0")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b)

    def wall(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "Benzene.xyz"))
    sh = basis.build_shells(syms, xyz, "def2-svp")
    grids = grid_gen.Grids(syms, xyz, level=3, device="cuda")
    n, ng = sh.nao, grids.size
    S = integrals.int1e(sh, syms, xyz)[0]
    # what HipBackend reads of its input, without the two-electron integrals (nothing here contracts them)
    inp = types.SimpleNamespace(shells=sh, grids=grids, symbols=syms, atom_xyz=xyz, eri=None, chol=np.zeros((1, n, n)), chol_range=None,
                                nocc=21, S=S, Hcore=S)
    be = scf.HipBackend(inp, "B3LYP", library_path(), device_resident=False, fused_tail=False, eigensolver="exact")
    rng = np.random.default_rng(1)
    C = rng.standard_normal((n, 21))
    C /= np.linalg.norm(C, axis=0)
    dm = 2.0 * C @ C.T
    be.xc_gradient(dm); be.xc_grid_response(dm)          # warm-up: allocations, shell table, LDS attributes
    t_fix, t_resp = [], []
    for _ in range(args.reps):
        t_fix.append(wall(lambda: be.xc_gradient(dm)))
        t_resp.append(wall(lambda: be.xc_grid_response(dm)))
    print(f"Benzene/def2-svp {ng} x {n} B3LYP HipBackend.xc_gradient (--gradient, XC part)            median {np.median(t_fix):8.2f} ms  min {min(t_fix):8.2f} ms  ({args.reps} reps, wall)")
    print(f"Benzene/def2-svp {ng} x {n} B3LYP HipBackend.xc_grid_response (what --grid-response adds) median {np.median(t_resp):8.2f} ms  min {min(t_resp):8.2f} ms  ({len(syms)} atom blocks)")
    # the library calls behind it, HIP events: the whole grid, and the block of the first atom
    s = be.solver
    d_dm = be._dev(dm)
    own = np.asarray(grids.atom_index)
    hi = int(np.flatnonzero(np.diff(own))[0]) + 1
    d_e = torch.empty(ng, dtype=torch.float64, device=dev)
    d_g = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_hs = torch.empty((6, ng, n), dtype=torch.float64, device=dev)
    d_out = torch.empty((len(syms), 3), dtype=torch.float64, device=dev)
    d_own = torch.as_tensor(own.astype(np.int32), device=dev)
    d_f = torch.as_tensor(np.asarray(grids.atomic_weights) * rng.standard_normal(ng), device=dev)
    radii = grid_gen.bragg_radii_bohr([basis.atomic_number(x) for x in syms])
    gr_blk = be.d_gr[:, :hi].contiguous()
    calls = {
        f"DFT_ComputeXC whole grid (for scale)": lambda: s.compute_xc(ng, n, d_dm, be.d_ao, be.d_w, be.d_v, be.d_gr),
        f"DFT_EvalAOHess whole grid": lambda: s.eval_ao_hess(sh, be.d_coords, ng, d_hs),
        f"DFT_ComputeXCGradient whole grid": lambda: s.compute_xc_gradient(ng, n, d_dm, be.d_ao, be.d_w, d_g, be.d_gr, d_hs),
        f"DFT_ComputeXCEnergyDensity whole grid": lambda: s.compute_xc_energy_density(ng, n, d_dm, be.d_ao, d_e, be.d_gr),
        f"DFT_EvalAOHess block of atom 1 ({hi} rows)": lambda: s.eval_ao_hess(sh, be.d_coords[:hi], hi, d_hs),
        f"DFT_ComputeXCGradient block of atom 1": lambda: s.compute_xc_gradient(hi, n, d_dm, be.d_ao[:hi], be.d_w[:hi], d_g, gr_blk, d_hs),
        f"DFT_ComputeXCEnergyDensity block of atom 1": lambda: s.compute_xc_energy_density(hi, n, d_dm, be.d_ao[:hi], d_e, gr_blk),
        f"DFT_BeckeWeightGradient {ng} x {len(syms)} atoms": lambda: s.becke_weight_gradient(ng, xyz, radii, be.d_coords, d_own, d_f, d_out),
    }
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    for k, v in ms.items():
        print(f"Benzene/def2-svp B3LYP {k:52s} median {np.median(v) * 1e3:10.1f} us   min {min(v) * 1e3:10.1f} us   (HIP events)")
    z = [basis.atomic_number(x) for x in syms]
    tw = [wall(lambda: grid_gen.becke_weights(grids.coords, own, xyz, z, device="cuda")) for _ in range(args.reps)]
    print(f"Benzene grid_gen.becke_weights forward in torch on the card, {ng} x {len(syms)}: median {np.median(tw):8.2f} ms  min {min(tw):8.2f} ms (wall, with its copies)")
    be.close()
    del be, d_hs
    if args.skip_large:
        return
    syms, xyz = basis.parse_xyz(os.path.join(inputs.DATA_DIR, "C33H56N7O17P3S.xyz"))
    coords, own, w0 = bare_grid(syms, xyz, 3)
    ng, natm = len(own), len(syms)
    z = [basis.atomic_number(x) for x in syms]
    s = q.DFTSolverWrapper(library_path(), "LDA")
    d_c = torch.as_tensor(np.ascontiguousarray(coords), device=dev)
    d_own = torch.as_tensor(own.astype(np.int32), device=dev)
    d_f = torch.as_tensor(w0 * rng.standard_normal(ng), device=dev)
    d_out = torch.empty((natm, 3), dtype=torch.float64, device=dev)
    radii = grid_gen.bragg_radii_bohr(z)
    fn = lambda: s.becke_weight_gradient(ng, xyz, radii, d_c, d_own, d_f, d_out)      # noqa: E731
    fn(); torch.cuda.synchronize()
    v = [timed(fn) for _ in range(args.reps)]
    print(f"C33H56N7O17P3S DFT_BeckeWeightGradient {ng} x {natm} atoms, synthetic f: median {np.median(v):8.2f} ms  min {min(v):8.2f} ms  (HIP events)"
          f"  rows sum {float(d_out.sum(dim=0).abs().max()):.1e}  max {float(d_out.abs().max()):.2e}")
    tw = [wall(lambda: grid_gen.becke_weights(coords, own, xyz, z, device="cuda")) for _ in range(min(args.reps, 3))]
    print(f"C33H56N7O17P3S grid_gen.becke_weights forward in torch on the card, {ng} x {natm}: median {np.median(tw):8.2f} ms  min {min(tw):8.2f} ms (wall, with its copies)")


if __name__ == "__main__":
    main()
