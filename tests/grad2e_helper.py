"""Shared pieces of the two-electron-gradient tests (test_grad2e_cpu.py, test_gpu_grad2e.py, test_gpu_grad2e_spin.py,
test_gpu_grad2e_reference.py): the CH/def2-TZVP fragment that meets every angular class s-f on bra and ket, the same
molecule with its atoms in another order (and the density permuted with them), two molecules with enough shells for the
kernel's ket-slice loop to run several times per workgroup, the host engine's results -- computed once per case and
shared, never modified -- and the yardstick.

What CH/def2-TZVP does NOT reach: its d and f shells all sit on the carbon, so every quartet with three or four shells
of l >= 2 is a one-centre quartet (X_AB = X_CD = 0, P = Q, Boys argument exactly 0, every recurrence term that multiplies
a centre difference vanishes), and (ff|ff) from the one f shell has a derivative that is zero by parity.  The four-centre
classes are held against the 100-digit reference of tests/golden/grad_ref_g*.npz (test_grad_reference_cpu.py on the host,
test_gpu_grad2e_reference.py on the device).

The yardstick is the host engine's own rounding floor: `bar` = the largest per-atom difference, relative to max|g|,
between integrals.grad2e on a molecule and on the same molecule with the atoms listed in the other order (another order
of the same sums).  A comparison passes when  10 bar <= 1e-11  and  |device - host| <= max(10 bar, 1e-13) scale  with
scale = max|host| of the compared array."""
import functools
import os

import numpy as np

from quantum_compute_dft_amd import basis, integrals

_H2O = "O 0 0 0.1173; H 0 0.7572 -0.4692; H 0 -0.7572 -0.4692"          # Angstrom
# (symbols, coordinates in bohr, basis)
CH = (["C", "H"], [[0.10, -0.20, 0.05], [1.25, 0.90, 1.60]], "def2-tzvp")          # 15 shells, 37 functions, L up to 13
H2O_STO = (*basis.parse_xyz(_H2O), "sto-3g")
H2O_SVP = (*basis.parse_xyz(_H2O), "def2-svp")
H_ATOM = (["H"], [[0.3, -0.1, 0.2]], "sto-3g")
# More than 16 shells: the device kernel cuts the ket-pair list into nslice = ceil(32768 / nshell^2) < nket slices, so a
# workgroup's loop over its ket pairs runs several times (slice_counts).  Generic orientations, no atom on an axis.
C2H4_SVP = (["C", "C", "H", "H", "H", "H"],                                        # 24 shells, 48 functions, d on two centres
            [[0.6786, 0.7885, 0.5927], [-0.3786, -1.2885, -0.3927], [-0.2744, 1.8787, 2.0496], [2.5207, 1.4453, -0.0355],
             [-2.2207, -1.9453, 0.2355], [0.5744, -2.3787, -1.8496]], "def2-svp")
C2_TZVP = (["C", "C"], [[0.10, -0.20, 0.05], [1.204, 1.18, 1.522]], "def2-tzvp")   # 22 shells, 62 functions, 2.3 bohr, f on both
SLICE_CASES = {"C2H4/def2-SVP": C2H4_SVP, "C2/def2-TZVP": C2_TZVP}
SLICE_TARGET = 32768                                 # csrc/grad2e.hip, DFT_Grad2eOpen: the (bra pair, slice) count aimed at


def molecule(case, order=None):
    """(symbols, xyz, shells) of `case`, atoms in `order` (default: as written)."""
    syms, xyz = list(case[0]), np.asarray(case[1], dtype=np.float64)
    if order is not None:
        syms, xyz = [syms[k] for k in order], xyz[list(order)]
    return syms, xyz, basis.build_shells(syms, xyz, case[2])


def ao_permutation(shells, order):
    """perm with D_reordered = D[perm][:, perm]: the functions of `shells` (atoms as written) in the order in which the
    molecule with atoms `order` lists them."""
    ao, l, atom = np.asarray(shells.ao), np.asarray(shells.l), np.asarray(shells.atom)
    per_atom = {}
    for s in range(shells.nshell):
        per_atom.setdefault(int(atom[s]), []).extend(range(int(ao[s]), int(ao[s]) + 2 * int(l[s]) + 1))
    return np.array([i for a in order for i in per_atom[a]], dtype=np.int64)


def random_density(nao, seed=7):
    """The symmetric D of test_gradient_integrals_cpu._setup."""
    a = np.random.default_rng(seed).standard_normal((nao, nao))
    return 0.1 * (a + a.T)


def block_diagonal(shells, D):
    """D with every block between functions of different atoms set to exactly zero."""
    ao, l, atom = np.asarray(shells.ao), np.asarray(shells.l), np.asarray(shells.atom)
    owner = np.empty(shells.nao, dtype=np.int64)
    for s in range(shells.nshell):
        owner[ao[s]:ao[s] + 2 * l[s] + 1] = atom[s]
    return np.where(owner[:, None] == owner[None, :], D, 0.0)


def sum_per_atom(shells, rows):
    out = np.zeros((int(np.max(shells.atom)) + 1, 3))
    for s in range(shells.nshell):
        out[int(shells.atom[s])] += rows[s]
    return out


def host_pair(shells, D, c_hf):
    """(per shell, per atom) from the host engine."""
    return integrals.grad2e(shells, D, c_hf, per_shell=True), integrals.grad2e(shells, D, c_hf)


def reorder_bar(case, D, c_hf, g_atoms):
    """The yardstick for density D (atoms as written) whose host per-atom result is g_atoms."""
    syms, _, sh = molecule(case)
    order = list(range(len(syms)))[::-1]
    sh2 = molecule(case, order)[2]
    perm = ao_permutation(sh, order)
    g2 = integrals.grad2e(sh2, np.ascontiguousarray(D[np.ix_(perm, perm)]), c_hf)
    return float(np.abs(g2[::-1] - g_atoms).max() / np.abs(g_atoms).max())


def ch_case(c_hf, swapped=False, blocked=False):
    """The CH fragment with the random density (optionally block-diagonal per atom), atoms as written or swapped:
    dict(shells, D, per_shell, per_atom, bar), computed once.  `bar` is measured between the two orders of this very case."""
    return _ch_case(float(c_hf), bool(swapped), bool(blocked))


@functools.lru_cache(maxsize=None)
def _ch_case(c_hf, swapped, blocked):
    syms, _, sh0 = molecule(CH)
    D0 = random_density(sh0.nao)
    if blocked:
        D0 = block_diagonal(sh0, D0)
    order = [1, 0] if swapped else [0, 1]
    sh = molecule(CH, order)[2]
    perm = ao_permutation(sh0, order)
    D = np.ascontiguousarray(D0[np.ix_(perm, perm)])
    rows, atoms = host_pair(sh, D, c_hf)
    if swapped:
        other = ch_case(c_hf, False, blocked)
        bar = other["bar"]
    else:
        bar = reorder_bar(CH, D0, c_hf, atoms)
    for a in (D, rows, atoms):
        a.setflags(write=False)
    return dict(shells=sh, D=D, per_shell=rows, per_atom=atoms, bar=bar)


def slice_counts(nshell):
    """(nslice, nket, ket pairs per workgroup at least, at most) of DFT_Grad2eOpen for a molecule of `nshell` shells."""
    nket = nshell * (nshell + 1) // 2
    nslice = max(1, min(nket, -(-SLICE_TARGET // (nshell * nshell))))
    return nslice, nket, nket // nslice, -(-nket // nslice)


def slice_case(name, c_hf, blocked=False):
    """A molecule of SLICE_CASES with the random D and M (seeds 7, 23; optionally block-diagonal per atom), atoms as written:
    dict(shells, D, M, per_shell, per_atom, spin_per_shell, spin_per_atom, bar), host results, computed once.  `bar` is
    reorder_bar of this very case."""
    return _slice_case(name, float(c_hf), bool(blocked))


@functools.lru_cache(maxsize=None)
def _slice_case(name, c_hf, blocked):
    case = SLICE_CASES[name]
    sh = molecule(case)[2]
    D, M = random_density(sh.nao), random_density(sh.nao, seed=23)
    if blocked:
        D, M = np.ascontiguousarray(block_diagonal(sh, D)), np.ascontiguousarray(block_diagonal(sh, M))
    rows, atoms = host_pair(sh, D, c_hf)
    srows, satoms = integrals.grad2e_spin(sh, D, M, c_hf, per_shell=True), integrals.grad2e_spin(sh, D, M, c_hf)
    bar = reorder_bar(case, D, c_hf, atoms)
    for a in (D, M, rows, atoms, srows, satoms):
        a.setflags(write=False)
    return dict(shells=sh, D=D, M=M, per_shell=rows, per_atom=atoms, spin_per_shell=srows, spin_per_atom=satoms, bar=bar)


def record(label, bar, err):
    """One line per case into grad2e_parity.txt in the directory QCDFT_WRITE_PROFILES names (how profiles/grad2e_parity.txt
    was made); an ordinary test run only prints."""
    line = f"{label:72s} host reorder bar / max|g| {bar:9.2e}   |device - host| / max|host| {err:9.2e}"
    print(line)
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, "grad2e_parity.txt")
    os.makedirs(out_dir, exist_ok=True)
    old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
    head = [l for l in old if l.startswith("#")] or [
        "# Two-electron gradient term: device (DFT_Grad2e) against the host engine (qc_grad2e).  bar = the host's own spread between",
        "# the two orders of the atoms; a case passes when 10 bar <= 1e-11 and the difference is <= max(10 bar, 1e-13) of max|host|."]
    body = sorted([l for l in old if l and not l.startswith("#") and not l.startswith(f"{label:72s}")] + [line])
    with open(path, "w") as fh:
        fh.write("\n".join(head + body) + "\n")


def check(label, got, ref, bar):
    got, ref = np.asarray(got), np.asarray(ref)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max() / scale)
    record(label, bar, err)
    assert 10.0 * bar <= 1e-11, (label, bar)
    assert err <= max(10.0 * bar, 1e-13), (label, err, bar)
