"""`python -m quantum_compute_dft_amd.dft <LDA|GGA|B3LYP> <Molecule>` -- the reference's driver
surface (dft.py:101-297: same positionals, same printed lines) on the MI355X engine.  The functional may also be any
other name of functionals.TABLE (PBE0, BLYP, ...) or an expression such as "0.75*pbe_x + pbe_c + 0.25*hf".
Extra flags (defaults = what the reference hard-codes): --basis sto-3g, --grid-level 3, --quirks 1.
--point-charges FILE runs the molecule in the field of external point charges (rows `x y z q`); --esp-points FILE with
--esp-out FILE writes the electrostatic potential of the converged density at the given points and --field-out FILE its
electric field; --charge-forces-out FILE writes the forces of the molecule on the point charges.  --efield Fx Fy Fz runs
the SCF in a uniform field (a.u.); --dipole reports the dipole moment, --polarizability the static polarizability by
coupled-perturbed Kohn-Sham (response.py; the response of Vxc on the device)."""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

from . import functionals, inputs, scf


def _functional(spec):
    try:
        functionals.resolve(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return spec.strip().upper() if spec.strip().upper() in functionals.TABLE else spec.strip()


def read_point_rows(path, ncol, unit="angstrom"):
    """(n, ncol) float64 from a text file of rows `x y z [q ...]` (blank lines and #-comments skipped); the first three
    columns converted to bohr when `unit` is "angstrom" (the unit of the .xyz files), taken as they are for "bohr"."""
    import numpy as np
    from .basis import BOHR
    if unit not in ("angstrom", "bohr"):
        raise ValueError(f"unit {unit!r}: expected 'angstrom' or 'bohr'")
    rows = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            f = line.split("#", 1)[0].split()
            if not f:
                continue
            if len(f) != ncol:
                raise ValueError(f"{path}:{n}: expected {ncol} numbers per row, found {len(f)}")
            rows.append([float(x) for x in f])
    a = np.array(rows, dtype=np.float64).reshape(-1, ncol)
    if unit == "angstrom":
        a[:, :3] /= BOHR
    return a


def write_esp_rows(path, points_bohr, esp, unit="angstrom"):
    """Rows `x y z esp`: the coordinates back in `unit`, the potential in atomic units (Ha / e)."""
    from .basis import BOHR
    scale = BOHR if unit == "angstrom" else 1.0
    with open(path, "w") as fh:
        for (x, y, z), v in zip(points_bohr, esp):
            fh.write(f"{x * scale:.10f} {y * scale:.10f} {z * scale:.10f} {v:.12e}\n")


def write_field_rows(path, points_bohr, field, unit="angstrom"):
    """Rows `x y z Ex Ey Ez`: the coordinates back in `unit`, the field in atomic units (Ha / (e bohr))."""
    from .basis import BOHR
    scale = BOHR if unit == "angstrom" else 1.0
    with open(path, "w") as fh:
        for (x, y, z), e in zip(points_bohr, field):
            fh.write(f"{x * scale:.10f} {y * scale:.10f} {z * scale:.10f} {e[0]:.12e} {e[1]:.12e} {e[2]:.12e}\n")


def write_charge_force_rows(path, charges_bohr, forces, unit="angstrom"):
    """Rows `x y z q Fx Fy Fz`: the charges' coordinates back in `unit`, the forces in Ha / bohr."""
    from .basis import BOHR
    scale = BOHR if unit == "angstrom" else 1.0
    with open(path, "w") as fh:
        for (x, y, z, q), f in zip(charges_bohr, forces):
            fh.write(f"{x * scale:.10f} {y * scale:.10f} {z * scale:.10f} {q:.12e} {f[0]:.12e} {f[1]:.12e} {f[2]:.12e}\n")


def print_gradient(symbols, g, grid_response=False):
    """The table of atoms with dE/dR (Ha/bohr) and the net force the fixed quadrature leaves (none with the grid response)."""
    if grid_response:
        print("Nuclear gradient dE/dR (Ha/bohr), the derivative includes the grid (points and Becke weights follow the atoms):")
    else:
        print("Nuclear gradient dE/dR (Ha/bohr), at fixed quadrature points and weights:")
    for k, (s, r) in enumerate(zip(symbols, g), 1):
        print(f"  {k:3d} {s:2s} {r[0]:+16.10f} {r[1]:+16.10f} {r[2]:+16.10f}")
    print("  sum    " + " ".join(f"{x:+16.10f}" for x in g.sum(axis=0)) + f"   max|g| = {np.abs(g).max():.2e}  rms = {np.sqrt(np.mean(g * g)):.2e}")


def build_parser():
    """The driver's command line (main() adds the checks that span several options)."""
    p = argparse.ArgumentParser(description="Run DFT (LDA/GGA/B3LYP) using the MI355X HIP backend.")
    p.add_argument("functional", type=_functional,
                   help="Functional: LDA, GGA, B3LYP (the reference's three), another name of the table (" +
                        ", ".join(k for k, f in functionals.TABLE.items() if f.builtin_type is None) +
                        ") or an expression over " + ", ".join(functionals.COMPONENTS) + " and hf")
    p.add_argument("xyzfile", type=str, help="Molecule name (e.g., H2O)")
    p.add_argument("--basis", default="sto-3g")            # grid.py:45 hard-codes sto-3g
    p.add_argument("--basis-file", default=None, help="NWChem / Gaussian94 basis file (Basis Set Exchange export) to register "
                                                     "under the --basis name: tables not shipped here (def2-SVP P, S; def2-TZVP N, O ...)")
    p.add_argument("--grid-level", type=int, default=3)   # grid.py:59
    p.add_argument("--quirks", type=int, default=1, help="1: reference formulas as shipped; 0: corrected VWN5/PBE-c derivatives")
    p.add_argument("--lib", default=None, help="path of libdft.so")
    p.add_argument("--eri", default="auto", choices=["auto", "dense", "cholesky"],
                   help="dense: the nao^4 tensor of grid.py:65; cholesky: factorised J/K; auto: dense while it stays below 8 GB (nao <= 178)")
    p.add_argument("--chol-tol", type=float, default=1e-9)
    p.add_argument("--eigensolver", default="auto", choices=["auto", "rotate", "exact"],
                   help="exact: eigh(F, S) every cycle as dft.py:227; rotate: occupied-subspace rotation from the previous cycle's "
                        "orbitals, full solver as first cycle and fallback; auto (default): rotate from 80 basis functions, exact below")
    p.add_argument("--device-resident", type=int, default=-1,
                   help="1: Fock build, DIIS, eigh and the density stay in HBM (only scalars cross PCIe per cycle); "
                        "0: host loop (one pinned transfer each way per cycle); -1 (default): device from 200 basis functions")
    p.add_argument("--fused-tail", type=int, default=-1,
                   help="1: the host part of the cycle as kernels of libdft.so (DFT_ScfTailStep; one rank, nao <= 512, nocc <= 64), "
                        "0: the host / torch loops, -1 (default): fused where it applies")
    p.add_argument("--ao", default="resident", choices=["resident", "direct"],
                   help="resident: AO values and gradients of the whole grid stay in HBM (the reference's layout, dft.py:155,172); "
                        "direct: they are re-evaluated chunk by chunk inside every XC call (DFT_ComputeXCDirect), memory ~100 MB")
    p.add_argument("--xc-occ", type=int, default=None, choices=[0, 1],
                   help="1 (default; a meta-GGA: 0, it has no occupied-orbital form): the XC sweep's density step through the occupied orbitals (DFT_ComputeXCOcc, 4 nao nocc flops "
                        "per grid point); 0: the reference's call with the full density matrix (DFT_ComputeXC, dft.py:206)")
    p.add_argument("--dm-factor", action="store_true",
                   help="with --xc-occ 0: the reference's call, with the library factorising the density matrix on the device "
                        "(option dm_factor, DFT_FactorDensity) and sweeping through the factor where the occupied form pays; "
                        "acts in the synchronous DFT_ComputeXC of the host loop (--device-resident 0 --fused-tail 0 above 80 functions)")
    p.add_argument("--both-quirks", action="store_true",
                   help="LDA/GGA: run the SCF twice, with the reference's formulas as shipped (its CUDA path) and with the "
                        "corrected VWN5 / PBE-c derivatives (what PySCF's slater,vwn5 / PBE,PBE compute), and report both energies")
    p.add_argument("--point-charges", default=None, metavar="FILE",
                   help="external point charges, text rows `x y z q` (electrostatic embedding: they enter the core Hamiltonian and the "
                        "nuclear repulsion; their interaction among themselves is not included)")
    p.add_argument("--point-charges-unit", default="angstrom", choices=["angstrom", "bohr"],
                   help="unit of the coordinates in --point-charges and --esp-points (default: angstrom, the unit of the .xyz file)")
    p.add_argument("--esp-points", default=None, metavar="FILE", help="text rows `x y z`: points at which the electrostatic potential of the "
                                                                      "converged density is evaluated (needs --esp-out and / or --field-out)")
    p.add_argument("--esp-out", default=None, metavar="FILE", help="receives rows `x y z esp` (coordinates in the unit given, potential in Ha/e; "
                                                                  "nuclei and electrons of the molecule, without the external charges)")
    p.add_argument("--field-out", default=None, metavar="FILE", help="receives rows `x y z Ex Ey Ez` for the --esp-points (coordinates in the unit given, "
                                                                    "electric field in Ha/(e bohr); the molecule's field, without the external charges)")
    p.add_argument("--charge-forces-out", default=None, metavar="FILE",
                   help="receives rows `x y z q Fx Fy Fz`: the force of the molecule on every charge of --point-charges in Ha/bohr "
                        "(the charges' forces on each other are not included)")
    p.add_argument("--efield", type=float, nargs=3, default=None, metavar=("FX", "FY", "FZ"),
                   help="uniform external electric field in a.u.: the SCF runs in it (core Hamiltonian += F.r, nuclear term -= sum Z F.R)")
    p.add_argument("--dipole", action="store_true", help="dipole moment of the converged density (e bohr and debye)")
    p.add_argument("--polarizability", action="store_true",
                   help="static dipole polarizability by coupled-perturbed Kohn-Sham (the response of Vxc on the device: DFT_FxcPrepare / "
                        "DFT_FxcApply); one rank, --ao resident")
    p.add_argument("--excitations", type=int, default=0, metavar="N",
                   help="the N lowest singlet excitation energies and oscillator strengths by TDDFT (reduced-space iteration; J and K of all "
                        "trial vectors of an iteration in one DFT_ComputeJKFactorizedResponse call with Cholesky vectors); one rank, --ao resident")
    p.add_argument("--tda", action="store_true", help="with --excitations: the Tamm-Dancoff approximation instead of the full TDDFT problem")
    p.add_argument("--triplets", action="store_true",
                   help="with --excitations: the N lowest TRIPLET excitations (spin-flip XC kernel on the device: DFT_FxcPrepareSpin / "
                        "DFT_FxcApplyKind; no Coulomb response, oscillator strengths are zero); needs --quirks 0 with vwn5_c or pbe_c")
    p.add_argument("--spin", type=int, default=None, metavar="N",
                   help="N = nalpha - nbeta: an unrestricted (UKS) run with the spin-resolved XC sweep (DFT_ComputeXCSpin) and the host loop "
                        "(--spin 0 too); one rank, --ao resident; needs --quirks 0 with vwn5_c or pbe_c.  Without the flag: the closed shell")
    p.add_argument("--open-shell-response", action="store_true",
                   help="with --spin: allow --dipole, --polarizability (unrestricted CPKS) and --excitations (spin-conserving U-TDDFT / "
                        "U-TDA, rows U1 ...) from the unrestricted reference (the open-shell response of Vxc on the device: "
                        "DFT_FxcPrepareSpinPol / DFT_FxcApplySpinPol); --triplets stays refused")
    p.add_argument("--open-shell-meta", action="store_true",
                   help="with --spin and a meta-GGA (TPSS, TPSSh, expressions with tpss_x / tpss_c): run the unrestricted loop on the "
                        "spin-resolved meta-GGA sweep (DFT_ComputeXCMetaSpin: tau and the tau term of the potential per spin); without "
                        "the flag --spin refuses a meta-GGA.  Response and excitations of such a state are not built; its nuclear "
                        "gradient is, on request (--open-shell-meta-gradient)")
    p.add_argument("--open-shell-meta-gradient", action="store_true",
                   help="with --spin N --open-shell-meta --open-shell-gradient, --gradient / --optimize and a meta-GGA: the nuclear "
                        "gradient of the unrestricted meta-GGA state with the tau term of either spin in the XC force "
                        "(gradients.nuclear_gradient_uks(meta=True), DFT_ComputeXCGradientMetaSpin), in every step of --optimize too; "
                        "--grid-response and --grad2e are honoured.  Without the flag the gradient of such a state is refused")
    p.add_argument("--meta-gradient", action="store_true",
                   help="with --gradient / --optimize and a meta-GGA (TPSS, TPSSh, expressions with tpss_x / tpss_c): the closed-shell "
                        "nuclear gradient with the tau term of the XC force (gradients.nuclear_gradient(meta=True), "
                        "DFT_ComputeXCGradientMeta), in every step of --optimize too; --grid-response and --grad2e are honoured.  "
                        "Without the flag --gradient / --optimize refuse a meta-GGA.  Closed shell only: not with --spin")
    p.add_argument("--open-shell-gradient", action="store_true",
                   help="with --spin: let --gradient and --optimize run on the unrestricted state (gradients.nuclear_gradient_uks: the XC "
                        "term per spin by DFT_ComputeXCGradientSpin, the two-electron term with the spin density, DFT_Grad2eSpin under "
                        "--grad2e device); every step of --optimize goes through the unrestricted loop")
    p.add_argument("--gradient", action="store_true",
                   help="analytic nuclear gradient dE/dR of the converged closed-shell state (Ha/bohr), at fixed quadrature points and weights")
    p.add_argument("--optimize", action="store_true",
                   help="Cartesian BFGS geometry optimisation on that gradient (step cap 0.3 bohr; max|g| < 3e-4, rms < 2e-4 Ha/bohr); "
                        "writes <molecule>_opt.xyz")
    p.add_argument("--opt-max-steps", type=int, default=50, metavar="N", help="with --optimize: at most N steps")
    p.add_argument("--grad2e", default="host", choices=["host", "device"],
                   help="with --gradient / --optimize: where the two-electron term of the gradient is computed; host (default): "
                        "integrals.c::qc_grad2e on the CPU share; device: DFT_Grad2e (csrc/grad2e.hip; DFT_Grad2eSpin with --open-shell-gradient), in every step of --optimize too")
    p.add_argument("--grid-response", action="store_true",
                   help="with --gradient / --optimize: add the grid response to the gradient (term xc_grid: the motion of the quadrature "
                        "points with their atoms and the derivatives of the Becke weights, DFT_ComputeXCEnergyDensity and "
                        "DFT_BeckeWeightGradient), in every step of --optimize too; the gradient then sums to zero over the atoms at "
                        "any grid level.  Works with --open-shell-gradient and either --grad2e; one rank, no --efield")
    p.add_argument("--charge", type=int, default=0, metavar="Q", help="charge of the molecule (electrons = sum Z - Q); an odd count needs --spin")
    p.add_argument("--json", default=None, help="also append the run's one-line JSON record to this file")
    p.add_argument("--dist-backend", default="nccl", help="torch.distributed backend when launched with WORLD_SIZE > 1 (nccl = RCCL)")
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if bool(args.esp_points) != bool(args.esp_out or args.field_out):
        p.error("--esp-points goes with --esp-out and / or --field-out")
    if args.charge_forces_out and not args.point_charges:
        p.error("--charge-forces-out needs --point-charges")
    fn = functionals.resolve(args.functional)
    if args.open_shell_meta and args.spin is None:
        p.error("--open-shell-meta goes with --spin N (the closed shell of a meta-GGA needs no flag)")
    if args.open_shell_meta and not fn.needs_tau:
        p.error(f"--open-shell-meta is for a meta-GGA: {args.functional} carries no tpss_x / tpss_c weight; --spin N alone runs it")
    if args.meta_gradient:
        if not fn.needs_tau:
            p.error(f"--meta-gradient is for a meta-GGA: {args.functional} carries no tpss_x / tpss_c weight; --gradient / --optimize "
                    "alone run it")
        if args.spin is not None:
            p.error("--meta-gradient is the closed-shell gradient of a meta-GGA: the gradient of an unrestricted (--spin) meta-GGA "
                    "state is not built")
        if not (args.gradient or args.optimize):
            p.error("--meta-gradient goes with --gradient or --optimize")
    if args.open_shell_meta_gradient:
        if not fn.needs_tau:
            p.error(f"--open-shell-meta-gradient is for a meta-GGA: {args.functional} carries no tpss_x / tpss_c weight; "
                    "--open-shell-gradient alone runs it")
        missing = [flag for flag, on in (("--spin N", args.spin is not None), ("--open-shell-meta", args.open_shell_meta),
                                         ("--open-shell-gradient", args.open_shell_gradient),
                                         ("--gradient or --optimize", args.gradient or args.optimize)) if not on]
        if missing:
            p.error("--open-shell-meta-gradient goes with --spin N --open-shell-meta --open-shell-gradient and --gradient or --optimize: "
                    + ", ".join(missing) + (" is" if len(missing) == 1 else " are") + " missing")
    if fn.needs_tau:
        if args.spin is not None and not args.open_shell_meta:
            p.error(f"--spin: {args.functional} is a meta-GGA and the unrestricted loop is not built for meta-GGA functionals unless "
                    "--open-shell-meta asks for the spin-resolved meta-GGA sweep (DFT_ComputeXCMetaSpin)")
        for flag, on in (("--polarizability", args.polarizability), ("--excitations", args.excitations),
                         ("--gradient", args.gradient), ("--optimize", args.optimize),
                         ("--open-shell-response", args.open_shell_response), ("--open-shell-gradient", args.open_shell_gradient),
                         ("--grid-response", args.grid_response)):
            by_request = flag in ("--gradient", "--optimize", "--grid-response")
            uks_request = by_request or flag == "--open-shell-gradient"
            if on and not (by_request and args.meta_gradient) and not (uks_request and args.open_shell_meta_gradient):
                p.error(f"{flag}: {args.functional} is a meta-GGA and this feature is not built for meta-GGA functionals "
                        "(only the ground state is: closed shell, and open shell with --spin N --open-shell-meta)" +
                        ("; the nuclear gradient of the unrestricted state is too, but only on request: add "
                         "--open-shell-meta-gradient (DFT_ComputeXCGradientMetaSpin)" if uks_request and args.spin is not None else
                         "; the closed-shell nuclear gradient is too, but only on request: add --meta-gradient "
                         "(DFT_ComputeXCGradientMeta)" if by_request else ""))
    if args.xc_occ is None:
        args.xc_occ = None if fn.needs_tau else 1
    if args.polarizability and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.ao != "resident"):
        p.error("--polarizability runs on one rank with --ao resident")
    if args.excitations < 0 or (args.tda and not args.excitations):
        p.error("--excitations takes a positive number of roots; --tda goes with it")
    if args.triplets and not args.excitations:
        p.error("--triplets goes with --excitations N")
    if args.excitations and (int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.ao != "resident"):
        p.error("--excitations runs on one rank with --ao resident")

    if args.gradient or args.optimize:
        if args.spin is not None and not args.open_shell_gradient:
            p.error("--gradient / --optimize: an unrestricted (--spin) run has no analytic gradient here: the assembly is closed-shell "
                    "unless --open-shell-gradient asks for the gradient of the unrestricted state")
        if args.efield is not None:
            p.error("--gradient / --optimize: a run in a uniform electric field (--efield) is not supported")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.dm_factor:
            p.error("--gradient / --optimize run on one rank and without --dm-factor")
        if args.quirks and fn.uses_quirks:
            p.error("--gradient / --optimize: with quirks = 1 the shipped vwn5_c / pbe_c potentials are not the derivatives of their "
                    "energies, so the converged state is not stationary; run with --quirks 0")
        if args.opt_max_steps < 1:
            p.error("--opt-max-steps takes a positive number")
    uks = args.spin is not None
    if args.open_shell_response and not uks:
        p.error("--open-shell-response goes with --spin N")
    if args.open_shell_gradient and not uks:
        p.error("--open-shell-gradient goes with --spin N")
    if args.open_shell_gradient and not (args.gradient or args.optimize):
        p.error("--open-shell-gradient goes with --gradient or --optimize")
    if args.grid_response and not (args.gradient or args.optimize):
        p.error("--grid-response goes with --gradient or --optimize")
    if uks:
        if (args.excitations or args.polarizability or args.dipole) and not args.open_shell_response:
            p.error("--excitations, --polarizability and --dipole take a closed-shell reference: not available after an unrestricted (--spin) run "
                    "unless --open-shell-response asks for the response of the unrestricted reference")
        if args.triplets:
            p.error("--triplets is the spin-flip kernel of a closed-shell reference: not available after an unrestricted (--spin) run "
                    "(--open-shell-response gives the spin-conserving excitations only)")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1 or args.ao != "resident" or args.dm_factor:
            p.error("--spin (UKS) runs on one rank with --ao resident and without --dm-factor")
        if args.fused_tail > 0 or args.device_resident > 0:
            p.error("--spin (UKS) walks the host loop: not with --fused-tail 1 or --device-resident 1")
        if args.both_quirks:
            p.error("--spin (UKS) has one form of every functional (the derivatives of the energy): not with --both-quirks")
        if args.quirks and fn.uses_quirks:
            p.error("--spin (UKS): the spin-resolved potentials are the first derivatives of the energy, but with quirks = 1 the shipped "
                    "vwn5_c / pbe_c potentials are not the derivatives of their energies; run with --quirks 0")

    # one process per GPU: `python -m torch.distributed.run --nproc-per-node N -m quantum_compute_dft_amd.dft ...`
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    device = "cuda"
    if world > 1:
        import torch
        import torch.distributed as dist
        device = f"cuda:{int(os.environ.get('LOCAL_RANK', rank)) % max(1, torch.cuda.device_count())}"
        torch.cuda.set_device(device)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    if rank:  # rank 0 speaks
        sys.stdout = open(os.devnull, "w")

    atom_file = args.xyzfile if args.xyzfile.lower().endswith(".xyz") else args.xyzfile + ".xyz"
    atom_path = atom_file if os.path.exists(atom_file) else os.path.join(inputs.DATA_DIR, atom_file)
    if not os.path.exists(atom_path):
        print(f"Error: {atom_path} not found.")
        sys.exit(1)
    from .hostinfo import blas_threads
    _pool_pin = blas_threads()   # host BLAS/OpenMP pools on the CPU share from the first numpy call on (hostinfo.py)
    _pool_pin.__enter__()
    if args.basis_file:
        from . import basis as _b
        _b.load_basis_file(args.basis_file, args.basis)
        for _sym, _sh in _b._BASIS_SETS[args.basis.lower().replace("_", "-")].items():
            for _msg in _b.check_table(_sym, _sh):
                print("basis file check:", _msg)
    print(f"=== DFT Solver: {args.functional} | Molecule: {atom_file} ===")
    print("Building CPU data...")
    if args.eri == "auto":
        from . import basis as _basis
        _nao = _basis.build_shells(*_basis.parse_xyz(atom_path), args.basis).nao
        args.eri = "dense" if 8.0 * _nao ** 4 <= 8.0e9 else "cholesky"
    charges = read_point_rows(args.point_charges, 4, args.point_charges_unit) if args.point_charges else None
    try:
        inp = inputs.build(atom_path, args.basis, args.grid_level, device=device, eri_mode=args.eri, chol_tol=args.chol_tol, rank=rank, world=world,
                           point_charges=charges, efield=args.efield, charge=args.charge, spin=args.spin or 0)
    except ValueError as e:      # an odd electron count without --spin, a charge and spin that do not fit, a bad charge file
        print(f"Error: {e}")
        sys.exit(1)
    if uks:
        print(f"Unrestricted (UKS): charge {inp.charge}, spin (nalpha - nbeta) {inp.spin}: {inp.nalpha} alpha and {inp.nbeta} beta electrons")
    if args.efield is not None:
        print(f"Uniform external field: F = ({args.efield[0]:+.6f}, {args.efield[1]:+.6f}, {args.efield[2]:+.6f}) a.u.")
    if charges is not None:
        print(f"External point charges: {len(charges)} (total {charges[:, 3].sum():+.6f} e), nuclei-charges repulsion {inp.E_nuc_ext:.8f} Ha")
    print(f"System Info: NAO={inp.shells.nao}, Grid={inp.grids.size}, Occupied={inp.nocc}")
    print(f"Calculating AO Gradients ({args.functional} mode)..." if fn.needs_gradient else f"Skipping AO Gradients ({args.functional} mode).")
    print("Moving data to GPU...")
    try:
        backend = scf.HipBackend(inp, args.functional, args.lib, quirks=bool(args.quirks), rank=rank, world=world, device=device,
                                 device_resident=False if uks else None if args.device_resident < 0 else bool(args.device_resident),
                                 fused_tail=False if uks else None if args.fused_tail < 0 else bool(args.fused_tail),
                                 eigensolver="exact" if uks else args.eigensolver, ao_mode=args.ao, xc_occ=None if args.xc_occ is None else bool(args.xc_occ), dm_factor=args.dm_factor)
    except Exception as e:  # dft.py:149-153
        print(e)
        sys.exit(1)
    print(f"GPU Init Time: {backend.init_time:.4f}s" + (f"  ({world} ranks: grid block + Cholesky-vector slice per GPU)" if world > 1 else ""))
    res = scf.run_uks(inp, backend, args.functional, meta=args.open_shell_meta) if uks else scf.run_scf(inp, backend, args.functional)
    eig_stats = dict(backend.occ_solver.stats) if backend.occ_solver is not None else None   # of THIS run (the second one below adds to the counters)
    other = None
    if args.both_quirks and fn.uses_quirks:   # only VWN5 and PBE-c have two forms (B3LYP's four components are derivative-correct: one answer)
        backend.solver.set_option("quirks", 0 if args.quirks else 1)
        if backend.occ_solver is not None:
            backend.occ_solver.reset()            # fresh full solve: the second SCF does not start from the first one's rotation
        other = scf.run_scf(inp, backend, args.functional, log=None)
        backend.solver.set_option("quirks", 1 if args.quirks else 0)
    if res["converged"]:
        print("-" * 80); print("Converged!")
        print(f"Total Energy: {res['E_tot']:.8f} Ha"); print(f"E_one       : {res['E_one']:.8f} Ha")
        print(f"E_coul      : {res['E_coul']:.8f} Ha"); print(f"E_nuc       : {inp.E_nuc:.8f} Ha")
        print(f"E_xc_dft    : {res['E_xc']:.8f} Ha")
        if fn.c_hf != 0.0:
            print(f"E_ex_hf     : {res['E_ex_hf']:.8f} Ha")
        if uks:
            print(f"<S^2>       : {res['s_squared']:.6f}   (Sz (Sz + 1) = {0.25 * inp.spin * (inp.spin + 2):.6f})")
        print(f"Total Time  : {res['total_time']:.4f} s"); print("-" * 80)
        print("Kernel Statistics (Avg per iter):"); print(f"XC(Exc+Vxc) Time: {res['xc_ms_avg']:.4f} ms")
        print(f"Median per cycle after the first: XC {res['xc_ms']:.4f} ms, J/K {res['jk_ms']:.4f} ms ({args.eri} ERI), "
              f"whole SCF iteration {res['iter_ms']:.4f} ms ({res['cycles']} cycles)")
        if backend.occ_solver is not None:
            st = eig_stats
            print(f"Eigensolver: {st['rotated']} cycles by occupied-subspace rotation ({st['inner_steps']} fixed-point steps), {st['exact']} by full diagonalisation")
        eig_dev = "occupied-subspace rotation, hipSOLVER eigh as fallback," if backend.occ_solver is not None else "hipSOLVER eigh"
        print("Host part of the cycle: " + ("device-resident: Fock build, DIIS, occupied-subspace rotation, density and energy traces as kernels of "
                                            "libdft.so (DFT_ScfTailStep); full diagonalisations by " + ("hipSOLVER" if inp.shells.nao >= 400 else "host LAPACK") if getattr(backend, "tail", None) is not None else
                                            f"device-resident (Fock build, DIIS, {eig_dev} in HBM)" if backend.device_resident
                                            else "host LAPACK eigh; [dm|cocc] up and [J|K|Vxc] down in one pinned transfer each"))
        print("-" * 80)
    else:
        print("SCF Unconverged.")
    if other is not None:
        a, b = ("reference formulas as shipped", "corrected derivatives") if args.quirks else ("corrected derivatives", "reference formulas as shipped")
        print(f"Total Energy, {a:32s}: {res['E_tot']:.8f} Ha   (this run; --quirks {args.quirks})")
        print(f"Total Energy, {b:32s}: {other['E_tot']:.8f} Ha   (difference {res['E_tot'] - other['E_tot']:+.2e} Ha)")
    if args.esp_points and res["converged"] and not rank:
        from . import properties
        esp_pts = read_point_rows(args.esp_points, 3, args.point_charges_unit)
        if args.esp_out:
            write_esp_rows(args.esp_out, esp_pts, properties.electrostatic_potential(inp, res["dm"], esp_pts, device=device), args.point_charges_unit)
            print(f"Electrostatic potential at {len(esp_pts)} points written to {args.esp_out}")
        if args.field_out:
            write_field_rows(args.field_out, esp_pts, properties.electric_field(inp, res["dm"], esp_pts, device=device), args.point_charges_unit)
            print(f"Electric field at {len(esp_pts)} points written to {args.field_out}")
    charge_forces = None
    if charges is not None and res["converged"] and not rank:
        from . import properties
        charge_forces = properties.point_charge_forces(inp, res["dm"], device=device)
        if args.charge_forces_out:
            write_charge_force_rows(args.charge_forces_out, inp.point_charges, charge_forces, args.point_charges_unit)
            print(f"Forces on {len(charge_forces)} point charges written to {args.charge_forces_out}")
    dipole = polar = None
    if args.dipole and res["converged"] and not rank:
        from . import properties
        dipole = properties.dipole_moment(inp, res["dm"])
        print("Dipole moment (e bohr): " + " ".join(f"{x:+.8f}" for x in dipole) +
              "   (debye: " + " ".join(f"{x * properties.DEBYE_PER_AU:+.6f}" for x in dipole) + f"; |mu| = {np.linalg.norm(dipole) * properties.DEBYE_PER_AU:.6f} D)")
    if args.polarizability and res["converged"]:
        from . import response
        polar = response.polarizability(inp, res, backend, args.functional, log=print)
        print("Static polarizability (a.u.):")
        for row in polar["alpha"]:
            print("   " + " ".join(f"{x:+14.8f}" for x in row))
        print(f"Isotropic polarizability: {np.trace(polar['alpha']) / 3.0:.8f} a.u.  (CPKS iterations x, y, z: {polar['cpks_iterations']})")
    excited = None
    if args.excitations and res["converged"]:
        from . import excitations as _ex
        excited = _ex.excitations(inp, res, backend, args.functional, nroots=args.excitations, tda=args.tda, log=print, triplet=args.triplets)
        nocc_ = inp.nocc
        if uks:
            print(f"Unrestricted excitations ({'U-TDA' if args.tda else 'U-TDDFT'}, spin-conserving; {excited['iterations']} iterations, "
                  f"{excited['sigma_builds']} trial vectors" + ("" if excited["converged"] else "; NOT converged") + "):")
            print("  state        eV         nm          f    largest |X+Y|")
            nva = inp.shells.nao - inp.nalpha
            for n, (w, f_n, x) in enumerate(zip(excited["energies"], excited["oscillator_strengths"], excited["xpy"]), 1):
                k = int(np.argmax(np.abs(x)))
                if k < inp.nalpha * nva:
                    sp, (i, a), no = "alpha", divmod(k, nva), inp.nalpha
                else:
                    sp, (i, a), no = "beta", divmod(k - inp.nalpha * nva, inp.shells.nao - inp.nbeta), inp.nbeta
                print(f"  U{n:<4d} {w * _ex.HARTREE_EV:9.4f} {_ex.NM_PER_HARTREE / w:10.2f} {f_n:10.6f}    {sp} {i + 1} -> {no + a + 1} ({abs(x[k]):.3f})")
    if args.excitations and res["converged"] and not uks:
        print(f"{'Triplet' if args.triplets else 'Singlet'} excitations ({'TDA' if args.tda else 'TDDFT'}; {excited['iterations']} iterations, {excited['sigma_builds']} trial vectors"
              + ("" if excited["converged"] else "; NOT converged") + "):")
        print("  state        eV         nm          f    largest |X+Y|")
        mult = "T" if args.triplets else "S"
        for n, (w, f_n, x) in enumerate(zip(excited["energies"], excited["oscillator_strengths"], excited["xpy"]), 1):
            i, a = np.unravel_index(np.argmax(np.abs(x)), x.shape)
            print(f"  {mult}{n:<4d} {w * _ex.HARTREE_EV:9.4f} {_ex.NM_PER_HARTREE / w:10.2f} {f_n:10.6f}    {i + 1} -> {nocc_ + a + 1} ({abs(x[i, a]):.3f})")
    grad = grad_terms = opt = None
    if (args.gradient or args.optimize) and res["converged"]:
        from . import gradients, optimize
        nuclear_gradient = gradients.nuclear_gradient_uks if uks else gradients.nuclear_gradient
        grad_kw = dict(two_electron=args.grad2e, grid_response=True) if args.grid_response else dict(two_electron=args.grad2e)
        if args.meta_gradient or args.open_shell_meta_gradient:
            grad_kw["meta"] = True
        grad, grad_terms = nuclear_gradient(inp, res, backend, args.functional, **grad_kw)
        print_gradient(inp.symbols, grad, args.grid_response)
    if args.optimize and res["converged"]:
        def energy_and_gradient(xyz):
            inp_k = inputs.build(atom_path, args.basis, args.grid_level, device=device, verbose=False, eri_mode=args.eri, chol_tol=args.chol_tol,
                                 point_charges=charges, charge=args.charge, spin=args.spin or 0, atom_xyz=xyz)
            if uks:
                be_k = scf.HipBackend(inp_k, args.functional, args.lib, quirks=bool(args.quirks), device=device, device_resident=False,
                                      fused_tail=False, eigensolver="exact", ao_mode=args.ao, xc_occ=None if args.xc_occ is None else bool(args.xc_occ))
                res_k = scf.run_uks(inp_k, be_k, args.functional, log=None, meta=args.open_shell_meta)
            else:
                be_k = scf.HipBackend(inp_k, args.functional, args.lib, quirks=bool(args.quirks), device=device, eigensolver=args.eigensolver,
                                      ao_mode=args.ao, xc_occ=None if args.xc_occ is None else bool(args.xc_occ))
                res_k = scf.run_scf(inp_k, be_k, args.functional, log=None)
            if not res_k["converged"]:
                raise RuntimeError("--optimize: the SCF did not converge at a geometry of the optimisation")
            g_k = nuclear_gradient(inp_k, res_k, be_k, args.functional, **grad_kw)[0]
            be_k.close()
            return res_k["E_tot"], g_k
        opt = optimize.bfgs(energy_and_gradient, inp.atom_xyz, max_steps=args.opt_max_steps, log=print)
        opt_path = os.path.splitext(os.path.basename(atom_file))[0] + "_opt.xyz"
        optimize.write_xyz(opt_path, inp.symbols, opt["xyz"], f"{args.functional}/{args.basis} E = {opt['energy']:.10f} Ha after {opt['steps']} steps")
        print(f"Geometry optimisation {'converged' if opt['converged'] else 'NOT converged'} after {opt['steps']} steps "
              f"({opt['evaluations']} energies and gradients): E = {opt['energy']:.10f} Ha; geometry written to {opt_path}")
        print_gradient(inp.symbols, opt["gradient"], args.grid_response)
    import json
    record = {"functional": args.functional, "molecule": os.path.splitext(atom_file)[0], "basis": args.basis, "grid_level": args.grid_level,
              "nao": int(inp.shells.nao), "ngrid": int(inp.grids.size), "nocc": int(inp.nocc), "n_gpus": world, "eri": args.eri,
              "c_hf": fn.c_hf, "weights": fn.weights,
              "quirks": int(args.quirks), "converged": bool(res["converged"]), "cycles": int(res.get("cycles", 0)),
              "E_tot": res.get("E_tot"), "E_one": res.get("E_one"), "E_coul": res.get("E_coul"), "E_xc": res.get("E_xc"),
              "E_ex_hf": res.get("E_ex_hf"), "E_nuc": float(inp.E_nuc), "total_time_s": res.get("total_time"),
              "xc_ms_avg": res.get("xc_ms_avg"), "xc_ms": res.get("xc_ms"), "jk_ms": res.get("jk_ms"), "iter_ms": res.get("iter_ms"),
              "cycle_ms": res.get("cycle_ms"), "gpu_init_s": backend.init_time, "device_resident": bool(backend.device_resident), "loop": res.get("loop", "device" if backend.device_resident else "host"), "ao": args.ao, "eigensolver": args.eigensolver,
              "eigensolver_stats": eig_stats, "xc_occ": int(backend.xc_occ), "dm_factor": int(backend.dm_factor),
              "charge": int(inp.charge), "spin": int(inp.spin), "uks": bool(uks)}
    if uks:
        record["loop"] = "host-uks"
        record["nalpha"], record["nbeta"] = int(inp.nalpha), int(inp.nbeta)
        record["s_squared"] = res.get("s_squared")
    if charges is not None:
        record["n_point_charges"] = int(len(charges)); record["E_nuc_ext"] = float(inp.E_nuc_ext)
        record["point_charge_forces"] = charge_forces.tolist() if charge_forces is not None else None
    if args.efield is not None:
        record["efield"] = [float(x) for x in args.efield]
    if args.dipole:
        record["dipole"] = dipole.tolist() if dipole is not None else None
    if args.polarizability:
        record["polarizability"] = polar["alpha"].tolist() if polar is not None else None
        record["cpks_iterations"] = [int(x) for x in polar["cpks_iterations"]] if polar is not None else None
    if args.excitations:
        record["excitation_method"] = ("tda" if args.tda else "tddft") + ("-uks" if uks else "-triplet" if args.triplets else "")
        record["excitation_multiplicity"] = None if uks else 3 if args.triplets else 1
        record["excitation_energies"] = excited["energies"].tolist() if excited is not None else None
        record["oscillator_strengths"] = excited["oscillator_strengths"].tolist() if excited is not None else None
        record["excitation_iterations"] = int(excited["iterations"]) if excited is not None else None
    if args.gradient or args.optimize:
        record["gradient"] = grad.tolist() if grad is not None else None
        record["gradient_terms"] = {k: v.tolist() for k, v in grad_terms.items()} if grad_terms is not None else None
        record["net_force"] = grad.sum(axis=0).tolist() if grad is not None else None
        record["grad2e_engine"] = args.grad2e
        if args.grid_response:
            record["grid_response"] = True
    if args.optimize:
        record["opt_steps"] = int(opt["steps"]) if opt is not None else None
        record["opt_energies"] = opt["energies"] if opt is not None else None
        record["opt_converged"] = bool(opt["converged"]) if opt is not None else None
        record["opt_geometry_bohr"] = opt["xyz"].tolist() if opt is not None else None
    if other is not None:
        record["E_tot_other_quirks"] = other.get("E_tot"); record["other_quirks"] = 0 if args.quirks else 1
    line = json.dumps(record)
    print(line)                                  # one JSON line per run for a harness
    if args.json and not rank:
        with open(args.json, "a") as fh:
            fh.write(line + "\n")

    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    pyscf_xc = None if uks else {"LDA": "slater,vwn5", "GGA": "PBE,PBE", "B3LYP": "b3lyp"}.get(args.functional)
    if importlib.util.find_spec("pyscf") is None or rank or pyscf_xc is None:   # dft.py:272-297 needs PySCF; the three reference functionals only
        print("\nPySCF not importable here: reference cross-check skipped.")
        return res
    print("\nRunning PySCF reference calculation...")
    from pyscf import dft as pdft, gto
    mol = gto.Mole(); mol.atom = "".join(open(atom_path).readlines()[2:]); mol.basis = args.basis; mol.verbose = 0; mol.build()
    mf = pdft.RKS(mol); mf.grids.level = args.grid_level
    mf.xc = pyscf_xc
    t0 = time.time(); mf.kernel(); el = time.time() - t0
    print(f"PySCF ({mf.xc}) Energy : {mf.e_tot:.8f} Hartree")
    print(f"Difference             : {abs(mf.e_tot - res['E_tot']):.2e} Hartree")
    print(f"PySCF Time             : {el:.4f} s")
    return res


if __name__ == "__main__":
    main()
