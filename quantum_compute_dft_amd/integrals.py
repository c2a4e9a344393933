"""S, T, V, dense ERI and E_nuc for the SCF driver -- host-side counterpart of the PySCF calls at
grid.py:61-66 (`mol.intor('int1e_ovlp'|'int1e_kin'|'int1e_nuc'|'int2e')`, `mol.energy_nuc()`).
The arithmetic is csrc/integrals.c (McMurchie-Davidson, OpenMP), built in-tree with gcc.  Also the one-electron Coulomb
integrals at arbitrary points (external point charges, electrostatic potential): point_coulomb_matrix / point_coulomb_contract
on the host, PointCoulomb on the device, point_coulomb() choosing between them; and the gradient of the contraction
with respect to the point (electric field of a density): point_coulomb_field, PointCoulomb.field, point_field().

PARITY UNPINNED against PySCF/libcint (not installed); pinned offline by quadrature on the
Becke grid, textbook H2/STO-3G integrals and RHF energies (tests/test_integrals.py)."""
import ctypes
import os
import subprocess

import numpy as np

from .basis import atomic_number
from .build import CSRC, LIB_DIR, _stamp_ok, build_lock, compile_env, source_hash

_LIB_PATH = os.path.join(LIB_DIR, "libqcint.so")
_SRC = os.path.join(CSRC, "integrals.c")
_FLAGS = ["-O2", "-fPIC", "-shared", "-fopenmp", "-std=c11"]
_lib = None


def build_integrals(force=False):
    """gcc -> lib/libqcint.so.  Called by __graft_entry__.build() and the test fixtures only; the
    loader below never compiles (same contract as build.library_path)."""
    want = source_hash([_SRC], _FLAGS)
    if force or not _stamp_ok(_LIB_PATH, _LIB_PATH + ".srchash", want):
        with build_lock(_LIB_PATH):
            if force or not _stamp_ok(_LIB_PATH, _LIB_PATH + ".srchash", want):
                tmp = _LIB_PATH + f".tmp{os.getpid()}"
                subprocess.run(["gcc"] + _FLAGS + [_SRC, "-o", tmp, "-lm"], check=True, env=compile_env())
                os.replace(tmp, _LIB_PATH)
                with open(_LIB_PATH + ".srchash", "w") as fh:
                    fh.write(want + "\n")
    return _LIB_PATH


def integrals_library_path():
    if not _stamp_ok(_LIB_PATH, _LIB_PATH + ".srchash", source_hash([_SRC], _FLAGS)):
        raise RuntimeError(f"{_LIB_PATH} is missing or older than csrc/integrals.c: run `python __graft_entry__.py` first")
    return _LIB_PATH


def _load():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(integrals_library_path())
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        L.qc_int1e.restype = ctypes.c_int
        L.qc_int1e.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp]
        L.qc_dipole.restype = ctypes.c_int
        L.qc_dipole.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, dp, dp]
        L.qc_int2e.restype = ctypes.c_int
        L.qc_int2e.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, dp]
        L.qc_eri_open.restype = ctypes.c_void_p
        L.qc_eri_open.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ctypes.c_int]
        L.qc_eri_close.restype = None
        L.qc_eri_close.argtypes = [ctypes.c_void_p]
        L.qc_eri_diag.restype = ctypes.c_int
        L.qc_eri_diag.argtypes = [ctypes.c_void_p, dp]
        L.qc_eri_cols.restype = ctypes.c_int
        L.qc_eri_cols.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, dp]
        L.qc_eri_cols2.restype = ctypes.c_int
        L.qc_eri_cols2.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, dp, ctypes.c_int]
        L.qc_set_threads.restype = None
        L.qc_set_threads.argtypes = [ctypes.c_int]
        for f in (L.qc_point_matrix, L.qc_point_contract, L.qc_point_field, L.qc_point_field_matrix):
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ctypes.c_longlong, dp, dp, dp]
        L.qc_grad1e.restype = ctypes.c_int
        L.qc_grad1e.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ip, ctypes.c_int, ctypes.c_int, dp, dp, dp, dp, dp]
        L.qc_grad2e.restype = ctypes.c_int
        L.qc_grad2e.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ip, ctypes.c_int, dp, ctypes.c_double, dp]
        L.qc_grad2e_spin.restype = ctypes.c_int
        L.qc_grad2e_spin.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ip, ctypes.c_int, dp, dp, ctypes.c_double, dp]
        from .hostinfo import host_cpu_share
        L.qc_set_threads(host_cpu_share())
        _lib = L
    return _lib


def _args(sh):
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    keep = [np.ascontiguousarray(sh.xyz, dtype=np.float64), np.ascontiguousarray(sh.l, dtype=np.int32),
            np.ascontiguousarray(sh.nprim, dtype=np.int32), np.ascontiguousarray(sh.off, dtype=np.int32),
            np.ascontiguousarray(sh.ao, dtype=np.int32), np.ascontiguousarray(sh.exp, dtype=np.float64),
            np.ascontiguousarray(sh.coef, dtype=np.float64)]
    ptrs = [keep[0].ctypes.data_as(dp)] + [k.ctypes.data_as(ip) for k in keep[1:5]] + [k.ctypes.data_as(dp) for k in keep[5:]]
    return keep, ptrs


def set_threads(n):
    """Worker threads of the integral engine's OpenMP regions (default: this rank's CPU share, hostinfo.py)."""
    _load().qc_set_threads(int(n))


def int1e(shells, symbols, atom_xyz):
    """(S, T, V) as (nao, nao) arrays; V is the nuclear-attraction matrix (negative)."""
    keep, p = _args(shells)
    n = shells.nao
    S, T, V = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    axyz = np.ascontiguousarray(atom_xyz, dtype=np.float64)
    z = np.array([atomic_number(s) for s in symbols], dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = _load().qc_int1e(shells.nshell, *p, n, len(z), axyz.ctypes.data_as(dp), z.ctypes.data_as(dp),
                          S.ctypes.data_as(dp), T.ctypes.data_as(dp), V.ctypes.data_as(dp))
    if rc != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return S, T, V


def dipole(shells, origin=(0.0, 0.0, 0.0)):
    """D[k] = <mu| (r - origin)_k |nu> as a (3, nao, nao) array (bohr), s-f shells."""
    keep, p = _args(shells)
    n = shells.nao
    D = np.zeros((3, n, n))
    o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    dp = ctypes.POINTER(ctypes.c_double)
    if _load().qc_dipole(shells.nshell, *p, n, o.ctypes.data_as(dp), D.ctypes.data_as(dp)) != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return D


def int2e(shells):
    """Dense (nao, nao, nao, nao) electron-repulsion tensor, chemists' notation (ij|kl)."""
    keep, p = _args(shells)
    n = shells.nao
    eri = np.zeros((n, n, n, n))
    rc = _load().qc_int2e(shells.nshell, *p, n, eri.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if rc != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return eri


def _sym(m, what):
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or not np.allclose(m, m.T, rtol=0.0, atol=1e-10 * max(1.0, float(np.abs(m).max()))):
        raise ValueError(f"{what}: a symmetric (nao, nao) matrix is expected")
    return m


def grad1e(shells, centres, charges, dm, w):
    """The basis-centre derivatives of S, T and the point-Coulomb matrix V = -sum_c q_c / |r - R_c| over the charged
    `centres` (n, 3) with `charges` (n,) (the nuclei; the external charges of an embedded run too), contracted as they are
    made (qc_grad1e): (3, natm, 3) = [-tr(W dS/dR_A), tr(D dT/dR_A), tr(D dV/dR_A) without the operator part].  dm, w
    symmetric.  The shell-to-atom map is the shell table's."""
    keep, p = _args(shells)
    dm, w = _sym(dm, "dm"), _sym(w, "w")
    cen = np.ascontiguousarray(np.asarray(centres, dtype=np.float64).reshape(-1, 3))
    q = np.ascontiguousarray(charges, dtype=np.float64)
    if q.shape != (cen.shape[0],):
        raise ValueError("grad1e: one charge per centre")
    owner = np.ascontiguousarray(shells.atom, dtype=np.int32)
    natm = int(owner.max()) + 1
    out = np.zeros((3, natm, 3))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rc = _load().qc_grad1e(shells.nshell, *p, shells.nao, owner.ctypes.data_as(ip), natm, cen.shape[0], cen.ctypes.data_as(dp),
                           q.ctypes.data_as(dp), dm.ctypes.data_as(dp), w.ctypes.data_as(dp), out.ctypes.data_as(dp))
    if rc != 0:
        raise ValueError("grad1e: unsupported angular momentum (s-f) or a shell without an atom")
    return out


def _grad2e_call(name, shells, mats, c_hf, per_shell):
    """qc_grad2e / qc_grad2e_spin (`name`) on the symmetric matrices `mats`: the owner of every shell (its atom, or with
    `per_shell` the shell itself), the zeroed output, the call and its refusal."""
    keep, p = _args(shells)
    owner = np.arange(shells.nshell, dtype=np.int32) if per_shell else np.ascontiguousarray(shells.atom, dtype=np.int32)
    natm = int(owner.max()) + 1
    out = np.zeros((natm, 3))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    rc = getattr(_load(), "qc_" + name)(shells.nshell, *p, shells.nao, owner.ctypes.data_as(ip), natm,
                                        *(m.ctypes.data_as(dp) for m in mats), float(c_hf), out.ctypes.data_as(dp))
    if rc != 0:
        raise ValueError(f"{name}: unsupported angular momentum (s-f) or a shell without an atom")
    return out


def grad2e(shells, dm, c_hf=0.0, per_shell=False):
    """(natm, 3): d/dR_A of 1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum D_ac D_bd (ab|cd) for a symmetric dm (qc_grad2e): every
    derivative quartet contracted as it is made, the dense ERI never built, threads as set_threads says.
    `per_shell`: (nshell, 3) instead, the term of every shell's own centre (the same routine with every shell its own
    "atom"); the rows of an atom's shells add up to the atom's row."""
    return _grad2e_call("grad2e", shells, [_sym(dm, "dm")], c_hf, per_shell)


def grad2e_spin(shells, dm, ms, c_hf=0.0, per_shell=False):
    """(natm, 3): d/dR_A of 1/2 sum D_ab D_cd (ab|cd) - c_hf/4 sum (D_ac D_bd + M_ac M_bd) (ab|cd), the two-electron energy of
    an open-shell state with the total density dm = D_a + D_b and the spin density ms = D_a - D_b, both symmetric
    (qc_grad2e_spin): grad2e's pass over the derivative quartets with the extended density quartet.  `per_shell` as in
    grad2e."""
    dm, ms = _sym(dm, "dm"), _sym(ms, "ms")
    if ms.shape != dm.shape:
        raise ValueError("grad2e_spin: dm and ms must have the same shape")
    return _grad2e_call("grad2e_spin", shells, [dm, ms], c_hf, per_shell)


def energy_nuc(symbols, atom_xyz):
    z = np.array([atomic_number(s) for s in symbols], dtype=np.float64)
    xyz = np.asarray(atom_xyz, dtype=np.float64)
    e = 0.0
    for i in range(len(z)):
        for j in range(i):
            e += z[i] * z[j] / np.linalg.norm(xyz[i] - xyz[j])
    return e


class EriColumns:
    """Column-wise access to the ERI without the dense tensor (for the pivoted Cholesky
    factorisation of cholesky.py): `diag()` = (ij|ij), `cols(C, D)` = every (ij|kl) with k in shell
    C and l in shell D."""

    def __init__(self, shells):
        keep, p = _args(shells)
        self.shells, self.nao = shells, shells.nao
        self._h = _load().qc_eri_open(shells.nshell, *p, shells.nao, len(shells.exp))
        if not self._h:
            raise ValueError("integrals: angular momentum above f is not supported")

    def close(self):
        if getattr(self, "_h", None):
            _load().qc_eri_close(self._h)
            self._h = None

    __del__ = close

    def diag(self):
        d = np.zeros((self.nao, self.nao))
        _load().qc_eri_diag(self._h, d.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return d

    def cols(self, C, D, screen=1e-14, out=None, lower_only=False):
        """(nfC*nfD, nao, nao): entry [k*nfD + l] is the symmetric matrix (..|kl).  `out`: a C-contiguous float64
        buffer of nfC*nfD*nao^2 elements to write into (e.g. pinned memory), returned reshaped.  `lower_only`: only the
        elements [i][j] with i >= j are written (the rest stay zero); the caller mirrors them."""
        nf = (2 * int(self.shells.l[C]) + 1) * (2 * int(self.shells.l[D]) + 1)
        if out is None:
            out = np.empty((nf, self.nao, self.nao))
        else:
            assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"] and out.size == nf * self.nao * self.nao
        rc = _load().qc_eri_cols2(self._h, int(C), int(D), float(screen), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(bool(lower_only)))
        if rc != 0:
            raise RuntimeError("qc_eri_cols failed (diag() must be called first)")
        return out.reshape(nf, self.nao, self.nao)


def schwarz_bounds(shells, diag):
    """sqrt(max (ab|ab)) per shell pair a >= b, in the order a (a + 1) / 2 + b (what integrals.c keeps internally after
    qc_eri_diag), from the (nao, nao) diagonal `diag` of the ERI matrix."""
    ao0 = np.asarray(shells.ao, dtype=np.int64)
    blk = np.maximum.reduceat(np.maximum.reduceat(np.asarray(diag), ao0, axis=0), ao0, axis=1)     # (nshell, nshell) block maxima
    a, b = np.tril_indices(shells.nshell)                                                          # row-major: a (a + 1) / 2 + b
    return np.sqrt(np.maximum(blk[a, b], 0.0))


class DeviceEriColumns:
    """The same columns computed ON THE DEVICE (libdft.so: csrc/eri_cols.hip, DFT_EriColumns) into a torch tensor: the
    pivoted Cholesky factorisation keeps its algebra there, so the columns never cross PCIe.  `qmax`: schwarz_bounds()."""

    def __init__(self, shells, qmax, lib_path=None):
        from .build import library_path
        from .solver import load_library
        self.lib = load_library(lib_path or library_path())
        L = self.lib
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        L.DFT_EriColumnsOpen.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ctypes.c_int, dp]
        L.DFT_EriColumnsOpen.restype = ctypes.c_void_p
        L.DFT_EriColumns.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_uint64]
        L.DFT_EriColumns.restype = ctypes.c_int
        L.DFT_EriColumnsMany.argtypes = [ctypes.c_void_p, ctypes.c_int, ip, ip, ctypes.c_double, ctypes.c_uint64, ctypes.POINTER(ctypes.c_longlong)]
        L.DFT_EriColumnsMany.restype = ctypes.c_int
        L.DFT_EriColumnsLastError.argtypes = [ctypes.c_void_p]
        L.DFT_EriColumnsLastError.restype = ctypes.c_char_p
        L.DFT_EriColumnsClose.argtypes = [ctypes.c_void_p]
        L.DFT_EriColumnsClose.restype = None
        keep, p = _args(shells)
        q = np.ascontiguousarray(qmax, dtype=np.float64)
        assert q.shape == (shells.nshell * (shells.nshell + 1) // 2,)
        self.shells, self.nao = shells, shells.nao
        self._h = L.DFT_EriColumnsOpen(shells.nshell, *p, shells.nao, len(shells.exp), q.ctypes.data_as(dp))
        if not self._h:
            raise RuntimeError("DFT_EriColumnsOpen failed (no device, or angular momentum above f)")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.DFT_EriColumnsClose(self._h)
            self._h = None

    __del__ = close

    def cols(self, C, D, screen, out):
        """Fills the torch tensor `out` ((2 l_C + 1)(2 l_D + 1) x nao x nao doubles on the device; elements i >= j only) and
        returns it viewed as (nq, nao, nao).  Asynchronous on the null stream, like torch's own kernels."""
        nq = (2 * int(self.shells.l[C]) + 1) * (2 * int(self.shells.l[D]) + 1)
        assert out.is_cuda and out.is_contiguous() and out.numel() >= nq * self.nao * self.nao
        if self.lib.DFT_EriColumns(self._h, int(C), int(D), float(screen), ctypes.c_uint64(out.data_ptr())) != 0:
            raise RuntimeError("libdft: " + (self.lib.DFT_EriColumnsLastError(self._h) or b"").decode())
        return out.view(-1)[:nq * self.nao * self.nao].view(nq, self.nao, self.nao)

    def cols_many(self, pairs, screen, out):
        """The blocks of several ket shell pairs [(C, D), ...] back to back in `out` (their kernels run side by side on the
        device); returns `out` viewed as (sum of the blocks' rows, nao, nao)."""
        n2 = self.nao * self.nao
        nqs = [(2 * int(self.shells.l[C]) + 1) * (2 * int(self.shells.l[D]) + 1) for C, D in pairs]
        offs = np.concatenate([[0], np.cumsum(nqs)[:-1]]).astype(np.int64) * n2
        tot = int(sum(nqs))
        assert out.is_cuda and out.is_contiguous() and out.numel() >= tot * n2
        Cs = (ctypes.c_int * len(pairs))(*[int(C) for C, _ in pairs]); Ds = (ctypes.c_int * len(pairs))(*[int(D) for _, D in pairs])
        of = (ctypes.c_longlong * len(pairs))(*[int(x) for x in offs])
        if self.lib.DFT_EriColumnsMany(self._h, len(pairs), Cs, Ds, float(screen), ctypes.c_uint64(out.data_ptr()), of) != 0:
            raise RuntimeError("libdft: " + (self.lib.DFT_EriColumnsLastError(self._h) or b"").decode())
        return out.view(-1)[:tot * n2].view(tot, self.nao, self.nao)


class DeviceGrad2e:
    """grad2e ON THE DEVICE (libdft.so: csrc/grad2e.hip, DFT_Grad2e): the derivative quartets are made and contracted with
    the density there; (nshell, 3) doubles come back.  `per_shell(d_dm, c_hf)` works on torch tensors and is asynchronous
    on the null stream (or the one given to set_stream); `grad(dm, c_hf)` is the drop-in for grad2e()."""

    def __init__(self, shells, lib_path=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceGrad2e: no GPU device is available (the two-electron gradient kernel runs on the device only; "
                               "integrals.grad2e is the host engine)")
        from .build import library_path
        from .solver import load_library
        self.lib = load_library(lib_path or library_path())
        L = self.lib
        dp, ip, u64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_uint64
        L.DFT_Grad2eOpen.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ctypes.c_int]
        L.DFT_Grad2eOpen.restype = ctypes.c_void_p
        L.DFT_Grad2e.argtypes = [ctypes.c_void_p, u64, ctypes.c_double, u64]
        L.DFT_Grad2e.restype = ctypes.c_int
        L.DFT_Grad2eSpin.argtypes = [ctypes.c_void_p, u64, u64, ctypes.c_double, u64]
        L.DFT_Grad2eSpin.restype = ctypes.c_int
        L.DFT_Grad2eSetStream.argtypes = [ctypes.c_void_p, u64]
        L.DFT_Grad2eSetStream.restype = ctypes.c_int
        L.DFT_Grad2eLastError.argtypes = [ctypes.c_void_p]
        L.DFT_Grad2eLastError.restype = ctypes.c_char_p
        L.DFT_Grad2eClose.argtypes = [ctypes.c_void_p]
        L.DFT_Grad2eClose.restype = None
        keep, p = _args(shells)
        self.shells, self.nao, self.nshell = shells, shells.nao, shells.nshell
        self._h = L.DFT_Grad2eOpen(shells.nshell, *p, shells.nao, len(shells.exp))
        if not self._h:
            raise RuntimeError("DFT_Grad2eOpen failed (no GPU device, or angular momentum above f)")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.DFT_Grad2eClose(self._h)
            self._h = None

    __del__ = close

    def set_stream(self, stream):
        """`stream`: a torch.cuda.Stream, or None for the null stream."""
        self.lib.DFT_Grad2eSetStream(self._h, ctypes.c_uint64(stream.cuda_stream if stream is not None else 0))

    def per_shell(self, d_dm, c_hf=0.0, out=None):
        """(nshell, 3) torch tensor: the term of every shell's centre, for the symmetric (nao, nao) device tensor `d_dm`
        (its symmetry is the caller's business here: nothing crosses to the host).  Asynchronous."""
        import torch
        PointCoulomb._check(d_dm, (self.nao, self.nao), "dm")
        if out is None:
            out = torch.empty((self.nshell, 3), dtype=torch.float64, device=d_dm.device)
        PointCoulomb._check(out, (self.nshell, 3), "out")
        if self.lib.DFT_Grad2e(self._h, ctypes.c_uint64(d_dm.data_ptr()), float(c_hf), ctypes.c_uint64(out.data_ptr())) != 0:
            raise RuntimeError("libdft: " + (self.lib.DFT_Grad2eLastError(self._h) or b"").decode())
        return out

    def per_shell_spin(self, d_dm, d_ms, c_hf=0.0, out=None):
        """per_shell for an open-shell state (DFT_Grad2eSpin): `d_dm` the total density D_a + D_b, `d_ms` the spin density
        D_a - D_b, both symmetric (nao, nao) device tensors; one pass over the derivative integrals.  Asynchronous."""
        import torch
        PointCoulomb._check(d_dm, (self.nao, self.nao), "dm")
        PointCoulomb._check(d_ms, (self.nao, self.nao), "ms")
        if out is None:
            out = torch.empty((self.nshell, 3), dtype=torch.float64, device=d_dm.device)
        PointCoulomb._check(out, (self.nshell, 3), "out")
        if self.lib.DFT_Grad2eSpin(self._h, ctypes.c_uint64(d_dm.data_ptr()), ctypes.c_uint64(d_ms.data_ptr()), float(c_hf),
                                   ctypes.c_uint64(out.data_ptr())) != 0:
            raise RuntimeError("libdft: " + (self.lib.DFT_Grad2eLastError(self._h) or b"").decode())
        return out

    def _on_device(self, m, what):
        import torch
        if torch.is_tensor(m):
            d = m.to(dtype=torch.float64).contiguous()
            _sym(d.cpu().numpy(), what)
            return d
        return torch.as_tensor(_sym(m, what), device="cuda")

    def _per_atom(self, rows):
        owner = np.asarray(self.shells.atom, dtype=np.int64)
        out = np.zeros((int(owner.max()) + 1, 3))
        for s in range(self.nshell):
            out[owner[s]] += rows[s]
        return out

    def grad_spin(self, dm, ms, c_hf=0.0):
        """numpy (natm, 3), what grad2e_spin(shells, dm, ms, c_hf) returns: symmetric host arrays or device tensors."""
        return self._per_atom(self.per_shell_spin(self._on_device(dm, "dm"), self._on_device(ms, "ms"), c_hf).cpu().numpy())

    def grad(self, dm, c_hf=0.0):
        """numpy (natm, 3), what grad2e(shells, dm, c_hf) returns: `dm` a symmetric host array or device tensor; the shells'
        rows are added per atom on the host, in shell order."""
        return self._per_atom(self.per_shell(self._on_device(dm, "dm"), c_hf).cpu().numpy())



def _points(points):
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points: expected an (n, 3) array in bohr, got shape {pts.shape}")
    return pts


def point_coulomb_matrix(shells, points, weights):
    """M[mu, nu] = sum_c weights[c] <mu| 1/|r - points[c]| |nu> on the host (csrc/integrals.c::qc_point_matrix): the
    (nao, nao) matrix of point charges `weights` at `points` (n, 3) bohr, with the sign of the integral -- the potential of
    charges q that electrons feel is -M(q) (inp.V is -M(atom_xyz, Z)).  M == M.T bit for bit."""
    pts = _points(points)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (len(pts),):
        raise ValueError(f"weights: expected shape ({len(pts)},), got {w.shape}")
    keep, p = _args(shells)
    n = shells.nao
    M = np.zeros((n, n))
    dp = ctypes.POINTER(ctypes.c_double)
    if len(pts) and _load().qc_point_matrix(shells.nshell, *p, n, len(pts), pts.ctypes.data_as(dp), w.ctypes.data_as(dp), M.ctypes.data_as(dp)) != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return M


def point_coulomb_contract(shells, points, dm):
    """u[c] = sum_{mu nu} dm[mu, nu] <mu| 1/|r - points[c]| |nu> on the host (qc_point_contract), for any (nao, nao) matrix
    (it need not be symmetric).  For a density matrix: int rho(r) / |r - points[c]| dr."""
    pts = _points(points)
    n = shells.nao
    D = np.ascontiguousarray(dm, dtype=np.float64)
    if D.shape != (n, n):
        raise ValueError(f"dm: expected shape ({n}, {n}), got {D.shape}")
    keep, p = _args(shells)
    u = np.zeros(len(pts))
    dp = ctypes.POINTER(ctypes.c_double)
    if len(pts) and _load().qc_point_contract(shells.nshell, *p, n, len(pts), pts.ctypes.data_as(dp), D.ctypes.data_as(dp), u.ctypes.data_as(dp)) != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return u


def point_coulomb_field(shells, points, dm):
    """G[c, k] = sum_{mu nu} dm[mu, nu] d<mu| 1/|r - R| |nu> / dR_k at R = points[c], k = x, y, z, on the host
    (qc_point_field): (n, 3), the gradient of point_coulomb_contract's value with respect to the point, for any
    (nao, nao) matrix.  Exact -- the basis does not move with the point.  For a density matrix the electronic part of the
    electric field is +G (the electronic potential is -u)."""
    pts = _points(points)
    n = shells.nao
    D = np.ascontiguousarray(dm, dtype=np.float64)
    if D.shape != (n, n):
        raise ValueError(f"dm: expected shape ({n}, {n}), got {D.shape}")
    keep, p = _args(shells)
    G = np.zeros((len(pts), 3))
    dp = ctypes.POINTER(ctypes.c_double)
    if len(pts) and _load().qc_point_field(shells.nshell, *p, n, len(pts), pts.ctypes.data_as(dp), D.ctypes.data_as(dp), G.ctypes.data_as(dp)) != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return G


def point_coulomb_field_matrix(shells, points, weights):
    """(3, nao, nao): M[k, mu, nu] = sum_c weights[c] d<mu| 1/|r - R| |nu> / dR_k at R = points[c], on the host
    (qc_point_field_matrix) -- for one point of unit weight the derivative integrals themselves.  Host only (the device has
    the contraction): what point_coulomb_field and PointCoulomb.field are checked against.  M[k] == M[k].T bit for bit."""
    pts = _points(points)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (len(pts),):
        raise ValueError(f"weights: expected shape ({len(pts)},), got {w.shape}")
    keep, p = _args(shells)
    n = shells.nao
    M = np.zeros((3, n, n))
    dp = ctypes.POINTER(ctypes.c_double)
    if len(pts) and _load().qc_point_field_matrix(shells.nshell, *p, n, len(pts), pts.ctypes.data_as(dp), w.ctypes.data_as(dp), M.ctypes.data_as(dp)) != 0:
        raise ValueError("integrals: angular momentum above f is not supported")
    return M


class PointCoulomb:
    """The same operations ON THE DEVICE (libdft.so: csrc/point_coulomb.hip, DFT_PointCoulomb*) on torch tensors:
    `matrix(points, weights)` -> (nao, nao), `contract(points, dm)` -> (n,), `field(points, dm)` -> (n, 3).  Asynchronous on the null stream (or the one
    given to set_stream), like torch's own kernels; the tensors live on the device that was current at construction."""

    def __init__(self, shells, lib_path=None):
        from .build import library_path
        from .solver import load_library
        self.lib = load_library(lib_path or library_path())
        L = self.lib
        dp, ip, u64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_uint64
        L.DFT_PointCoulombOpen.argtypes = [ctypes.c_int, dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, ctypes.c_int]
        L.DFT_PointCoulombOpen.restype = ctypes.c_void_p
        L.DFT_PointCoulombMatrix.argtypes = [ctypes.c_void_p, ctypes.c_longlong, u64, u64, u64]
        L.DFT_PointCoulombMatrix.restype = ctypes.c_int
        L.DFT_PointCoulombContract.argtypes = [ctypes.c_void_p, ctypes.c_longlong, u64, u64, u64]
        L.DFT_PointCoulombContract.restype = ctypes.c_int
        L.DFT_PointCoulombField.argtypes = [ctypes.c_void_p, ctypes.c_longlong, u64, u64, u64]
        L.DFT_PointCoulombField.restype = ctypes.c_int
        L.DFT_PointCoulombSetStream.argtypes = [ctypes.c_void_p, u64]
        L.DFT_PointCoulombSetStream.restype = ctypes.c_int
        L.DFT_PointCoulombLastError.argtypes = [ctypes.c_void_p]
        L.DFT_PointCoulombLastError.restype = ctypes.c_char_p
        L.DFT_PointCoulombClose.argtypes = [ctypes.c_void_p]
        L.DFT_PointCoulombClose.restype = None
        keep, p = _args(shells)
        self.shells, self.nao = shells, shells.nao
        self._h = L.DFT_PointCoulombOpen(shells.nshell, *p, shells.nao, len(shells.exp))
        if not self._h:
            raise RuntimeError("DFT_PointCoulombOpen failed (no device, or angular momentum above f)")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.DFT_PointCoulombClose(self._h)
            self._h = None

    __del__ = close

    def _error(self):
        return RuntimeError("libdft: " + (self.lib.DFT_PointCoulombLastError(self._h) or b"").decode())

    def set_stream(self, stream):
        """`stream`: a torch.cuda.Stream, or None for the null stream."""
        self.lib.DFT_PointCoulombSetStream(self._h, ctypes.c_uint64(stream.cuda_stream if stream is not None else 0))

    @staticmethod
    def _check(t, shape, what):
        import torch
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError(f"{what}: expected a contiguous float64 device tensor of shape {shape}")

    def matrix(self, points, weights, out=None):
        import torch
        n = int(points.shape[0])
        self._check(points, (n, 3), "points"); self._check(weights, (n,), "weights")
        if out is None:
            out = torch.empty((self.nao, self.nao), dtype=torch.float64, device=points.device)
        self._check(out, (self.nao, self.nao), "out")
        if self.lib.DFT_PointCoulombMatrix(self._h, n, ctypes.c_uint64(points.data_ptr() if n else 0),
                                           ctypes.c_uint64(weights.data_ptr() if n else 0), ctypes.c_uint64(out.data_ptr())) != 0:
            raise self._error()
        return out

    def contract(self, points, dm, out=None):
        import torch
        n = int(points.shape[0])
        self._check(points, (n, 3), "points"); self._check(dm, (self.nao, self.nao), "dm")
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=points.device)
        self._check(out, (n,), "out")
        if self.lib.DFT_PointCoulombContract(self._h, n, ctypes.c_uint64(points.data_ptr() if n else 0), ctypes.c_uint64(dm.data_ptr()),
                                             ctypes.c_uint64(out.data_ptr() if n else 0)) != 0:
            raise self._error()
        return out

    def field(self, points, dm, out=None):
        import torch
        n = int(points.shape[0])
        self._check(points, (n, 3), "points"); self._check(dm, (self.nao, self.nao), "dm")
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float64, device=points.device)
        self._check(out, (n, 3), "out")
        if self.lib.DFT_PointCoulombField(self._h, n, ctypes.c_uint64(points.data_ptr() if n else 0), ctypes.c_uint64(dm.data_ptr()),
                                          ctypes.c_uint64(out.data_ptr() if n else 0)) != 0:
            raise self._error()
        return out


def point_coulomb(shells, points, weights=None, dm=None, device="cpu"):
    """The one entry the rest of the package calls: `weights` given -> the (nao, nao) matrix, `dm` given -> the values
    at the points; numpy in, numpy out.  On a CUDA device the kernels of libdft.so (PointCoulomb), otherwise the host
    engine -- there is no quiet fall-back from one to the other."""
    if (weights is None) == (dm is None):
        raise ValueError("point_coulomb: give either weights (matrix) or dm (contraction)")
    if not str(device).startswith("cuda"):
        return point_coulomb_matrix(shells, points, weights) if dm is None else point_coulomb_contract(shells, points, dm)
    import torch
    dev = torch.device(device)
    with torch.cuda.device(dev):
        pc = PointCoulomb(shells)
        try:
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
            pts = t(_points(points))
            res = pc.matrix(pts, t(weights)) if dm is None else pc.contract(pts, t(dm))
            return res.cpu().numpy()         # the copy waits for the kernels
        finally:
            pc.close()


def point_field(shells, points, dm, device="cpu"):
    """(n, 3) gradient of point_coulomb(dm=...)'s values with respect to the points; numpy in, numpy out.  On a CUDA
    device PointCoulomb.field, otherwise point_coulomb_field -- no quiet fall-back from one to the other."""
    if not str(device).startswith("cuda"):
        return point_coulomb_field(shells, points, dm)
    import torch
    dev = torch.device(device)
    with torch.cuda.device(dev):
        pc = PointCoulomb(shells)
        try:
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
            return pc.field(t(_points(points)), t(dm)).cpu().numpy()         # the copy waits for the kernels
        finally:
            pc.close()
