"""ctypes binding of libdft.so.

`DFTSolverWrapper` mirrors the reference class of the same name
(dft.py:15-95): same constructor arguments, same `compute_xc` /
`compute_coulomb` signatures and argument meaning, same error behaviour
(FileNotFoundError for a missing library, ValueError for an unknown functional,
RuntimeError when the C side returns a null solver).  Device arrays may be
torch tensors (`.data_ptr()`), CuPy arrays (`.data.ptr`, what the reference
passes) or plain integer device addresses.

Extensions beyond the reference class: compute_exchange / compute_jk /
eval_ao / set_option / timings, all thin calls into the extra C symbols; and the
functional may be any name or expression functionals.resolve() knows ("PBE0",
"0.75*pbe_x + pbe_c + 0.25*hf"): the three reference names keep their built-in
solver types, everything else becomes a mix solver (DFT_CreateSolverMix).
"""
import ctypes
import os

from . import functionals
from .build import LIB_PATH

_u64 = ctypes.c_uint64


def default_library_path():
    return LIB_PATH


def load_library(lib_path=None):
    """ctypes handle of libdft.so.  The process must end up with ONE HIP runtime: the array library
    that owns the device buffers (torch-ROCm here, CuPy-ROCm in the reference) bundles its own
    libamdhip64 and loads it by path, so it has to be imported BEFORE libdft.so, which then binds to
    that copy.  Loaded the other way round, libdft.so pulls in /opt/rocm's runtime, the process holds
    two, and whichever initialises second reports no device (measured on the MI355X box)."""
    try:
        import torch  # noqa: F401  (the device-buffer provider of this repo; brings the HIP runtime)
    except ImportError:
        pass
    return ctypes.CDLL(os.path.abspath(lib_path or default_library_path()))


def _ptr(a):
    """Raw device address of a torch tensor / CuPy array / int (0 for None)."""
    if a is None:
        return 0
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):
        return int(a.data_ptr())
    data = getattr(a, "data", None)
    if data is not None and hasattr(data, "ptr"):
        return int(data.ptr)
    raise TypeError(f"cannot take a device pointer from {type(a).__name__}")


class DFTSolverWrapper:
    TYPE_LDA = 0
    TYPE_GGA = 1
    TYPE_B3LYP = 2

    def __init__(self, lib_path=None, functional_type="lda"):
        lib_path = lib_path or LIB_PATH
        if not os.path.exists(lib_path):
            raise FileNotFoundError(f"Shared library not found at: {lib_path}")
        self.lib = load_library(lib_path)
        self.functional_type = functional_type.upper() if isinstance(functional_type, str) else functional_type.name
        # ValueError for an unknown name (dft.py:66-67), before anything is created
        self.functional = functionals.resolve(functional_type)
        self.c_hf = self.functional.c_hf                       # exact-exchange fraction the SCF loop applies
        self.needs_gradient = self.functional.needs_gradient   # ao_grad is required
        self.weights = self.functional.weight_vector()         # the eight coefficients, functionals.COMPONENTS order
        self.needs_tau = self.functional.needs_tau             # a meta-GGA: compute_xc_meta is its sweep
        self.meta_weights = self.functional.meta_weight_vector()
        L = self.lib
        # --- the four reference symbols, declared exactly as dft.py:27-50 does
        L.DFT_CreateSolver.argtypes = [ctypes.c_int]
        L.DFT_CreateSolver.restype = ctypes.c_void_p
        L.DFT_DestroySolver.argtypes = [ctypes.c_void_p]
        L.DFT_DestroySolver.restype = None
        L.DFT_ComputeXC.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                    _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXC.restype = ctypes.c_double
        L.DFT_ComputeCoulomb.argtypes = [ctypes.c_void_p, ctypes.c_int, _u64, _u64, _u64]
        L.DFT_ComputeCoulomb.restype = None
        # --- extensions
        L.DFT_ComputeXC64.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                      _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXC64.restype = ctypes.c_double
        L.DFT_ComputeXCAsync.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                         _u64, _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCAsync.restype = ctypes.c_int
        L.DFT_ComputeXCOcc.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                       _u64, _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCOcc.restype = ctypes.c_double
        L.DFT_ComputeXCOccAsync.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                            _u64, _u64, _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCOccAsync.restype = ctypes.c_int
        L.DFT_ComputeExchange.argtypes = [ctypes.c_void_p, ctypes.c_int, _u64, _u64, _u64]
        L.DFT_ComputeExchange.restype = None
        L.DFT_ComputeJK.argtypes = [ctypes.c_void_p, ctypes.c_int, _u64, _u64, _u64, _u64]
        L.DFT_ComputeJK.restype = None
        L.DFT_ComputeJKRows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _u64, _u64, _u64, _u64]
        L.DFT_ComputeJKRows.restype = ctypes.c_int
        L.DFT_ComputeJKFactorized.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeJKFactorized.restype = ctypes.c_int
        L.DFT_ComputeJKFactorizedResponse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                      _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeJKFactorizedResponse.restype = ctypes.c_int
        L.DFT_FactorDensity.argtypes = [ctypes.c_void_p, ctypes.c_int, _u64, ctypes.c_int, ctypes.c_double, _u64,
                                        ctypes.POINTER(ctypes.c_double)]
        L.DFT_FactorDensity.restype = ctypes.c_int
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        L.DFT_EvalAO.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                 dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, _u64, _u64, _u64]
        L.DFT_EvalAO.restype = ctypes.c_int
        L.DFT_ComputeXCDirect.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                          dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, ctypes.c_longlong]
        L.DFT_ComputeXCDirect.restype = ctypes.c_int
        L.DFT_SetOption.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]
        L.DFT_SetOption.restype = ctypes.c_int
        L.DFT_GetOption.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        L.DFT_GetOption.restype = ctypes.c_double
        L.DFT_SetStream.argtypes = [ctypes.c_void_p, _u64]
        L.DFT_SetStream.restype = ctypes.c_int
        L.DFT_GetLastError.argtypes = [ctypes.c_void_p]
        L.DFT_GetLastError.restype = ctypes.c_char_p
        L.DFT_GetTimings.argtypes = [ctypes.c_void_p, dp, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
        L.DFT_GetTimings.restype = ctypes.c_int
        L.DFT_GetVersion.argtypes = []
        L.DFT_GetVersion.restype = ctypes.c_int
        L.DFT_CreateSolverMix.argtypes = [dp, ctypes.c_int]
        L.DFT_CreateSolverMix.restype = ctypes.c_void_p
        L.DFT_GetMix.argtypes = [ctypes.c_void_p, dp, ctypes.c_int]
        L.DFT_GetMix.restype = ctypes.c_int
        L.DFT_FxcPrepare.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _u64, _u64, _u64, _u64, _u64]
        L.DFT_FxcPrepare.restype = ctypes.c_int
        L.DFT_FxcApply.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64]
        L.DFT_FxcApply.restype = ctypes.c_int
        L.DFT_FxcPrepareSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, ctypes.c_int]
        L.DFT_FxcPrepareSpin.restype = ctypes.c_int
        L.DFT_FxcApplyKind.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, ctypes.c_int]
        L.DFT_FxcApplyKind.restype = ctypes.c_int
        L.DFT_ComputeXCSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, _u64, _u64, dp]
        L.DFT_ComputeXCSpin.restype = ctypes.c_int
        L.DFT_FxcPrepareSpinPol.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64]
        L.DFT_FxcPrepareSpinPol.restype = ctypes.c_int
        L.DFT_FxcApplySpinPol.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, _u64]
        L.DFT_FxcApplySpinPol.restype = ctypes.c_int
        L.DFT_FxcSpinPolTable.argtypes = [ctypes.c_void_p, _u64, ctypes.c_longlong]
        L.DFT_FxcSpinPolTable.restype = ctypes.c_int
        L.DFT_EvalAOHess.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                     dp, ip, ip, ip, ip, dp, dp, ctypes.c_int, _u64, _u64]
        L.DFT_EvalAOHess.restype = ctypes.c_int
        L.DFT_ComputeXCGradient.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCGradient.restype = ctypes.c_int
        L.DFT_ComputeXCGradientSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCGradientSpin.restype = ctypes.c_int
        L.DFT_ComputeXCEnergyDensity.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCEnergyDensity.restype = ctypes.c_int
        L.DFT_ComputeXCEnergyDensitySpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64]
        L.DFT_ComputeXCEnergyDensitySpin.restype = ctypes.c_int
        L.DFT_BeckeWeightGradient.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, dp, dp, _u64, _u64, _u64, _u64, _u64]
        L.DFT_BeckeWeightGradient.restype = ctypes.c_int

        if self.needs_tau:
            # added without a change of DFT_GetVersion: the symbols are looked up, a library without them cannot serve a meta-GGA
            if not hasattr(L, "DFT_CreateSolverMeta"):
                raise RuntimeError(f"{lib_path} has no DFT_CreateSolverMeta: it cannot run the meta-GGA {self.functional_type}")
            self._declare_meta()
            self.solver = L.DFT_CreateSolverMeta((ctypes.c_double * len(self.weights))(*self.weights), len(self.weights),
                                                 (ctypes.c_double * len(self.meta_weights))(*self.meta_weights), len(self.meta_weights))
        elif self.functional.builtin_type is not None:
            self.solver = L.DFT_CreateSolver(self.functional.builtin_type)
        else:
            self.solver = L.DFT_CreateSolverMix((ctypes.c_double * len(self.weights))(*self.weights), len(self.weights))
        if not self.solver:
            raise RuntimeError("Failed to create C++ DFT Solver instance.")

    def _declare_meta(self):
        L, dp = self.lib, ctypes.POINTER(ctypes.c_double)
        L.DFT_CreateSolverMeta.argtypes = [dp, ctypes.c_int, dp, ctypes.c_int]
        L.DFT_CreateSolverMeta.restype = ctypes.c_void_p
        L.DFT_GetMeta.argtypes = [ctypes.c_void_p, dp, ctypes.c_int]
        L.DFT_GetMeta.restype = ctypes.c_int
        L.DFT_ComputeTau.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64]
        L.DFT_ComputeTau.restype = ctypes.c_int
        L.DFT_ComputeXCMeta.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, _u64, _u64, _u64, _u64, _u64, dp]
        L.DFT_ComputeXCMeta.restype = ctypes.c_int

    def _declare_meta_spin(self):
        L, dp = self.lib, ctypes.POINTER(ctypes.c_double)
        # added without a change of DFT_GetVersion: a library without them cannot serve an open-shell meta-GGA
        if not hasattr(L, "DFT_ComputeXCMetaSpin") or not hasattr(L, "DFT_ComputeTauSpin"):
            raise RuntimeError("the library has no DFT_ComputeTauSpin / DFT_ComputeXCMetaSpin: it cannot run an open-shell meta-GGA")
        L.DFT_ComputeTauSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [_u64] * 5
        L.DFT_ComputeTauSpin.restype = ctypes.c_int
        L.DFT_ComputeXCMetaSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [_u64] * 7 + [dp]
        L.DFT_ComputeXCMetaSpin.restype = ctypes.c_int

    def __del__(self):
        if hasattr(self, "lib") and hasattr(self, "solver") and self.solver:
            self.lib.DFT_DestroySolver(self.solver)
            self.solver = None

    # ---- reference surface (dft.py:69-95) -------------------------------
    def compute_xc(self, ngrid, nao, d_dm, d_ao, d_weights, d_vxc, d_ao_grad=None):
        energy = self.lib.DFT_ComputeXC64(
            self.solver, int(ngrid), int(nao),
            _u64(_ptr(d_dm)), _u64(_ptr(d_ao)), _u64(_ptr(d_ao_grad)),
            _u64(_ptr(d_weights)), _u64(_ptr(d_vxc)))
        self._check()
        return energy

    def compute_coulomb(self, nao, d_eri, d_dm, d_J):
        self.lib.DFT_ComputeCoulomb(self.solver, int(nao), _u64(_ptr(d_eri)),
                                    _u64(_ptr(d_dm)), _u64(_ptr(d_J)))
        self._check()

    # ---- extensions -------------------------------------------------------
    def compute_xc_async(self, ngrid, nao, d_dm, d_ao, d_weights, d_vxc, d_exc, d_ao_grad=None):
        rc = self.lib.DFT_ComputeXCAsync(
            self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm)), _u64(_ptr(d_ao)),
            _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)), _u64(_ptr(d_vxc)), _u64(_ptr(d_exc)))
        self._check()
        return rc

    def compute_xc_occ(self, ngrid, nao, nocc, d_cocc, d_ao, d_weights, d_vxc, d_ao_grad=None, d_dm=None):
        """compute_xc with the occupied orbitals: d_cocc (nao, nocc), dm = cocc cocc^T (sqrt(2) C_occ for the closed-shell
        dm of dft.py:181-182).  Same Exc / Vxc as compute_xc(dm); the density step costs 4 nao nocc instead of 2 nao^2 flops
        per grid point where that is less.  d_dm is optional (used where the dm kernels are the better path)."""
        energy = self.lib.DFT_ComputeXCOcc(
            self.solver, int(ngrid), int(nao), int(nocc), _u64(_ptr(d_cocc)), _u64(_ptr(d_dm)), _u64(_ptr(d_ao)),
            _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)), _u64(_ptr(d_vxc)))
        self._check()
        return energy

    def compute_xc_occ_async(self, ngrid, nao, nocc, d_cocc, d_ao, d_weights, d_vxc, d_exc, d_ao_grad=None, d_dm=None):
        rc = self.lib.DFT_ComputeXCOccAsync(
            self.solver, int(ngrid), int(nao), int(nocc), _u64(_ptr(d_cocc)), _u64(_ptr(d_dm)), _u64(_ptr(d_ao)),
            _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)), _u64(_ptr(d_vxc)), _u64(_ptr(d_exc)))
        self._check()
        return rc

    def compute_exchange(self, nao, d_eri, d_dm, d_K):
        self.lib.DFT_ComputeExchange(self.solver, int(nao), _u64(_ptr(d_eri)),
                                     _u64(_ptr(d_dm)), _u64(_ptr(d_K)))
        self._check()

    def compute_jk(self, nao, d_eri, d_dm, d_J, d_K):
        self.lib.DFT_ComputeJK(self.solver, int(nao), _u64(_ptr(d_eri)), _u64(_ptr(d_dm)),
                               _u64(_ptr(d_J)), _u64(_ptr(d_K)))
        self._check()

    def compute_jk_rows(self, nao, i_lo, i_hi, d_eri_rows, d_dm, d_J, d_K):
        """J, K from ERI rows (i, j), i_lo <= i < i_hi; d_eri_rows is that row block (first row (i_lo, 0)).
        Partial J over all columns, rows [i_lo, i_hi) of K: the shares of all blocks add up (all-reduce)."""
        rc = self.lib.DFT_ComputeJKRows(self.solver, int(nao), int(i_lo), int(i_hi), _u64(_ptr(d_eri_rows)),
                                        _u64(_ptr(d_dm)), _u64(_ptr(d_J)), _u64(_ptr(d_K)))
        self._check()
        return rc

    def compute_jk_factorized(self, nao, naux, nocc, d_chol, d_dm, d_cocc, d_J, d_K):
        """J, K from Cholesky vectors d_chol (naux, nao, nao); dm = cocc cocc^T, cocc (nao, nocc).
        d_J / d_K (and the input only the other one needs) may be None."""
        rc = self.lib.DFT_ComputeJKFactorized(self.solver, int(nao), int(naux), int(nocc), _u64(_ptr(d_chol)),
                                              _u64(_ptr(d_dm)), _u64(_ptr(d_cocc)), _u64(_ptr(d_J)), _u64(_ptr(d_K)))
        self._check()
        return rc

    def compute_jk_factorized_response(self, nao, naux, nocc, nvec, d_chol, d_a, d_b, d_J, d_M):
        """Response J and M of nvec trial densities D_k = A B_k^T + B_k A^T from Cholesky vectors
        (DFT_ComputeJKFactorizedResponse): d_a (nao, nocc), d_b (nvec, nao, nocc); d_J (nvec, nao, nao) receives J[D_k],
        d_M (nvec, nao, nao) the unsymmetrised M_k with K[A B_k^T +- B_k A^T] = M_k +- M_k^T.  Either output may be None.
        One half transform of A and, for J, one pass over the vectors per eight trials, whatever nvec."""
        rc = self.lib.DFT_ComputeJKFactorizedResponse(self.solver, int(nao), int(naux), int(nocc), int(nvec), _u64(_ptr(d_chol)),
                                                      _u64(_ptr(d_a)), _u64(_ptr(d_b)), _u64(_ptr(d_J)), _u64(_ptr(d_M)))
        self._check()
        return rc

    def factor_density(self, d_dm, max_rank=None, tol=None):
        """dm = L L^T on the device (DFT_FactorDensity): (L, rank) with L a (nao, rank) torch tensor on d_dm's device -- the
        `d_cocc` of compute_xc_occ / compute_jk_factorized -- or None when dm is no such product with rank <= max_rank
        (default nao // 2); `self.factor_info` then says why ({steps, last residual / scale, reason, scale})."""
        import torch
        nao = int(d_dm.shape[0])
        cap = min(nao, int(max_rank)) if max_rank and max_rank > 0 else max(nao // 2, 1)
        buf = torch.empty(nao * cap, dtype=torch.float64, device=d_dm.device)
        info = (ctypes.c_double * 4)()
        rank = self.lib.DFT_FactorDensity(self.solver, nao, _u64(_ptr(d_dm)), cap, float(tol) if tol else 0.0, _u64(_ptr(buf)), info)
        self.factor_info = list(info)
        if rank < 0:
            self._check()
            raise RuntimeError("libdft: DFT_FactorDensity failed")
        if rank == 0:
            return None
        return buf[:nao * rank].view(nao, rank), rank

    @staticmethod
    def _shell_args(shells):
        """(keep-alive arrays, ctypes arguments) of a basis.ShellTable for DFT_EvalAO / DFT_ComputeXCDirect."""
        import numpy as np
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        arrs = [np.ascontiguousarray(shells.xyz, dtype=np.float64)] + \
               [np.ascontiguousarray(a, dtype=np.int32) for a in (shells.l, shells.nprim, shells.off, shells.ao)] + \
               [np.ascontiguousarray(shells.exp, dtype=np.float64), np.ascontiguousarray(shells.coef, dtype=np.float64)]
        args = [int(shells.nao), int(len(arrs[1])), arrs[0].ctypes.data_as(dp)] + [a.ctypes.data_as(ip) for a in arrs[1:5]] + \
               [arrs[5].ctypes.data_as(dp), arrs[6].ctypes.data_as(dp), int(len(arrs[5]))]
        return arrs, args

    def eval_ao(self, shells, d_coords, ngrid, d_ao, d_ao_grad=None):
        """shells: a basis.ShellTable (host numpy arrays, see basis.py)."""
        keep, args = self._shell_args(shells)
        rc = self.lib.DFT_EvalAO(self.solver, int(ngrid), *args, _u64(_ptr(d_coords)), _u64(_ptr(d_ao)), _u64(_ptr(d_ao_grad)))
        self._check()
        return rc

    def compute_xc_direct(self, shells, ngrid, d_coords, d_weights, d_dm, d_vxc, d_exc, chunk_points=0):
        """AO -> rho -> XC -> Vxc without resident AO planes (DFT_ComputeXCDirect): results in d_vxc / d_exc once the
        solver's stream has drained (asynchronous, like compute_xc_async)."""
        keep, args = self._shell_args(shells)
        rc = self.lib.DFT_ComputeXCDirect(self.solver, int(ngrid), *args, _u64(_ptr(d_coords)), _u64(_ptr(d_weights)),
                                          _u64(_ptr(d_dm)), _u64(_ptr(d_vxc)), _u64(_ptr(d_exc)), int(chunk_points))
        self._check()
        return rc

    def fxc_prepare(self, ngrid, nao, d_dm0, d_ao, d_weights, d_ao_grad=None, d_cocc=None, nocc=0):
        """First half of the linear response of Vxc (DFT_FxcPrepare): the ground-state density step and the derivative
        table of the functional, kept in the solver.  d_cocc (nao, nocc) with dm0 = cocc cocc^T takes the occupied-orbital
        density step under compute_xc_occ's rule; d_dm0 may then be None."""
        rc = self.lib.DFT_FxcPrepare(self.solver, int(ngrid), int(nao), int(nocc), _u64(_ptr(d_cocc)), _u64(_ptr(d_dm0)),
                                     _u64(_ptr(d_ao)), _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)))
        self._check()
        return rc

    def fxc_apply(self, ngrid, nao, d_dm1, d_ao, d_v1, d_ao_grad=None):
        """V1 = d/dt compute_xc(dm0 + t dm1).vxc at t = 0 into d_v1 (DFT_FxcApply), in the convention compute_xc writes
        Vxc in; asynchronous on the solver's stream.  Any number of calls after one fxc_prepare."""
        rc = self.lib.DFT_FxcApply(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm1)), _u64(_ptr(d_ao)),
                                   _u64(_ptr(d_ao_grad)), _u64(_ptr(d_v1)))
        self._check()
        return rc

    def fxc_prepare_spin(self, ngrid, nao, d_dm0, d_ao, d_weights, d_ao_grad=None, d_cocc=None, nocc=0, kind=1):
        """fxc_prepare for the tables of the spin-resolved energy bodies (DFT_FxcPrepareSpin), into the slot of `kind`:
        1 the spin-flip (triplet) response, 2 the singlet response through the same bodies.  Independent of quirks; an
        fxc_prepare table is left alone."""
        rc = self.lib.DFT_FxcPrepareSpin(self.solver, int(ngrid), int(nao), int(nocc), _u64(_ptr(d_cocc)), _u64(_ptr(d_dm0)),
                                         _u64(_ptr(d_ao)), _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)), int(kind))
        self._check()
        return rc

    def fxc_apply_kind(self, ngrid, nao, d_dm1, d_ao, d_v1, d_ao_grad=None, kind=1):
        """fxc_apply with the table chosen (DFT_FxcApplyKind): 0 fxc_prepare's, 1 / 2 the slots of fxc_prepare_spin."""
        rc = self.lib.DFT_FxcApplyKind(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm1)), _u64(_ptr(d_ao)),
                                       _u64(_ptr(d_ao_grad)), _u64(_ptr(d_v1)), int(kind))
        self._check()
        return rc

    def compute_xc_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao, d_weights, d_vxc_a, d_vxc_b, d_ao_grad=None):
        """Exc of the spin density matrices d_dm_a / d_dm_b (DFT_ComputeXCSpin); the potentials of the two spins go to d_vxc_a /
        d_vxc_b in compute_xc's convention for the functional.  The first derivatives of the spin-resolved energy bodies:
        with option quirks = 1 a functional with vwn5_c or pbe_c is refused (RuntimeError).  Synchronous."""
        exc = ctypes.c_double(float("nan"))
        self.lib.DFT_ComputeXCSpin(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm_a)), _u64(_ptr(d_dm_b)), _u64(_ptr(d_ao)),
                                   _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)), _u64(_ptr(d_vxc_a)), _u64(_ptr(d_vxc_b)),
                                   ctypes.byref(exc))
        self._check()
        return exc.value

    def compute_tau(self, ngrid, nao, d_dm, d_ao_grad, d_tau):
        """tau (ngrid) of d_dm from the three gradient planes d_ao_grad (3, ngrid, nao) into d_tau (DFT_ComputeTau); any
        solver; asynchronous on the solver's stream."""
        self._declare_meta()
        rc = self.lib.DFT_ComputeTau(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm)), _u64(_ptr(d_ao_grad)), _u64(_ptr(d_tau)))
        self._check()
        return rc

    def compute_xc_meta(self, ngrid, nao, d_dm, d_ao, d_weights, d_vxc, d_ao_grad=None):
        """Exc of a meta-GGA solver (DFT_ComputeXCMeta); d_vxc receives V in the mix solver's one-sided convention plus the
        whole tau term: (V + V^T)/2 is dExc/dD.  With option quirks = 1 a functional with vwn5_c or pbe_c is refused, as by
        compute_xc_spin.  Synchronous."""
        self._declare_meta()
        exc = ctypes.c_double(float("nan"))
        self.lib.DFT_ComputeXCMeta(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm)), _u64(_ptr(d_ao)), _u64(_ptr(d_weights)),
                                   _u64(_ptr(d_ao_grad)), _u64(_ptr(d_vxc)), ctypes.byref(exc))
        self._check()
        return exc.value

    def compute_tau_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao_grad, d_tau_a, d_tau_b):
        """tau of each spin's matrix into d_tau_a / d_tau_b (DFT_ComputeTauSpin): one two-spin kernel with option
        tau_spin_fused = 1, compute_tau's kernel once per spin with 0; any solver; asynchronous on the solver's stream."""
        self._declare_meta_spin()
        rc = self.lib.DFT_ComputeTauSpin(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm_a)), _u64(_ptr(d_dm_b)), _u64(_ptr(d_ao_grad)),
                                         _u64(_ptr(d_tau_a)), _u64(_ptr(d_tau_b)))
        self._check()
        return rc

    def compute_xc_meta_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao, d_weights, d_vxc_a, d_vxc_b, d_ao_grad=None):
        """Exc of a meta-GGA solver at the spin density matrices d_dm_a / d_dm_b (DFT_ComputeXCMetaSpin); d_vxc_s receives V_s in
        the mix solver's one-sided convention plus the whole tau term of spin s: (V_s + V_s^T)/2 is dExc/dD_s.  Refusals as
        compute_xc_meta's (RuntimeError).  Synchronous."""
        self._declare_meta_spin()
        exc = ctypes.c_double(float("nan"))
        self.lib.DFT_ComputeXCMetaSpin(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm_a)), _u64(_ptr(d_dm_b)), _u64(_ptr(d_ao)),
                                       _u64(_ptr(d_weights)), _u64(_ptr(d_ao_grad)), _u64(_ptr(d_vxc_a)), _u64(_ptr(d_vxc_b)),
                                       ctypes.byref(exc))
        self._check()
        return exc.value

    def meta(self):
        """The solver's meta weights as the library reports them (DFT_GetMeta)."""
        self._declare_meta()
        out = (ctypes.c_double * len(functionals.META_COMPONENTS))()
        if self.lib.DFT_GetMeta(self.solver, out, len(out)) != 0:
            raise RuntimeError("DFT_GetMeta failed")
        return list(out)

    def fxc_prepare_spinpol(self, ngrid, nao, d_dm0_a, d_dm0_b, d_ao, d_weights, d_ao_grad=None):
        """First half of the open-shell response of Vxc (DFT_FxcPrepareSpinPol): the densities of the two spins and the
        second-derivative table of the spin-resolved energy bodies at any polarisation, kept in a slot of its own.  With
        option quirks = 1 a functional with vwn5_c or pbe_c is refused, as by compute_xc_spin."""
        rc = self.lib.DFT_FxcPrepareSpinPol(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm0_a)), _u64(_ptr(d_dm0_b)),
                                            _u64(_ptr(d_ao)), _u64(_ptr(d_ao_grad)), _u64(_ptr(d_weights)))
        self._check()
        return rc

    def fxc_apply_spinpol(self, ngrid, nao, d_dm1_a, d_dm1_b, d_ao, d_v1_a, d_v1_b, d_ao_grad=None):
        """V1_s = d/dt compute_xc_spin(dm0_a + t dm1_a, dm0_b + t dm1_b).vxc_s at t = 0 into d_v1_a / d_v1_b
        (DFT_FxcApplySpinPol), in compute_xc_spin's conventions; asynchronous on the solver's stream.  Any number of calls
        after one fxc_prepare_spinpol."""
        rc = self.lib.DFT_FxcApplySpinPol(self.solver, int(ngrid), int(nao), _u64(_ptr(d_dm1_a)), _u64(_ptr(d_dm1_b)),
                                          _u64(_ptr(d_ao)), _u64(_ptr(d_ao_grad)), _u64(_ptr(d_v1_a)), _u64(_ptr(d_v1_b)))
        self._check()
        return rc

    def fxc_spinpol_table(self, ngrid, device):
        """(planes, ngrid) torch tensor: a copy of the table fxc_prepare_spinpol left (DFT_FxcSpinPolTable; for the tests)."""
        import torch
        buf = torch.empty(28 * int(ngrid), dtype=torch.float64, device=device)
        planes = self.lib.DFT_FxcSpinPolTable(self.solver, _u64(_ptr(buf)), buf.numel())
        self._check()
        torch.cuda.synchronize()
        return buf[:planes * int(ngrid)].view(planes, int(ngrid))

    def eval_ao_hess(self, shells, d_coords, ngrid, d_hess):
        """The six second-derivative AO planes xx, xy, xz, yy, yz, zz into d_hess (6, ngrid, nao) (DFT_EvalAOHess), in
        eval_ao's conventions; asynchronous on the solver's stream."""
        keep, args = self._shell_args(shells)
        rc = self.lib.DFT_EvalAOHess(self.solver, int(ngrid), *args, _u64(_ptr(d_coords)), _u64(_ptr(d_hess)))
        self._check()
        return rc

    def _xc_gradient(self, fn, dms, ngrid, nao, d_ao, d_weights, d_out, d_ao_grad, d_ao_hess):
        """The four gradient entries: `fn` takes the matrices `dms`, then ao, the weights, ao_grad, ao_hess and the output."""
        rc = fn(self.solver, int(ngrid), int(nao), *(_u64(_ptr(d)) for d in (*dms, d_ao, d_weights, d_ao_grad, d_ao_hess, d_out)))
        self._check()
        return rc

    def _xc_energy_density(self, fn, dms, ngrid, nao, d_ao, d_e_out, d_ao_grad):
        """The four energy-density entries: `fn` takes the matrices `dms`, then ao, ao_grad and the output."""
        rc = fn(self.solver, int(ngrid), int(nao), *(_u64(_ptr(d)) for d in (*dms, d_ao, d_ao_grad, d_e_out)))
        self._check()
        return rc

    def compute_xc_gradient(self, ngrid, nao, d_dm, d_ao, d_weights, d_out, d_ao_grad=None, d_ao_hess=None):
        """G (nao, 3) into d_out (DFT_ComputeXCGradient): the derivative of compute_xc's Exc by the centre of every basis
        function at fixed points and weights; asynchronous on the solver's stream.  d_ao_hess may be None for an
        LDA-class functional."""
        return self._xc_gradient(self.lib.DFT_ComputeXCGradient, [d_dm], ngrid, nao, d_ao, d_weights, d_out, d_ao_grad, d_ao_hess)

    def compute_xc_gradient_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao, d_weights, d_out, d_ao_grad=None, d_ao_hess=None):
        """G (nao, 3) into d_out (DFT_ComputeXCGradientSpin): the derivative of compute_xc_spin's Exc by the centre of every
        basis function at fixed points and weights; asynchronous on the solver's stream.  d_ao_hess may be None for an
        LDA-class functional.  With option quirks = 1 a functional with vwn5_c or pbe_c is refused, as by compute_xc_spin."""
        return self._xc_gradient(self.lib.DFT_ComputeXCGradientSpin, [d_dm_a, d_dm_b], ngrid, nao, d_ao, d_weights, d_out, d_ao_grad, d_ao_hess)

    def compute_xc_energy_density(self, ngrid, nao, d_dm, d_ao, d_e_out, d_ao_grad=None):
        """e_g, the energy per volume of the functional at the density of d_dm, into d_e_out (ngrid) without the weight
        (DFT_ComputeXCEnergyDensity): sum_g w_g e_g is compute_xc's Exc.  The body, cut-offs, quirks and mix weights of the
        sweep's pointwise kernel; asynchronous on the solver's stream."""
        return self._xc_energy_density(self.lib.DFT_ComputeXCEnergyDensity, [d_dm], ngrid, nao, d_ao, d_e_out, d_ao_grad)

    def compute_xc_energy_density_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao, d_e_out, d_ao_grad=None):
        """e_g of the spin density matrices d_dm_a / d_dm_b into d_e_out (DFT_ComputeXCEnergyDensitySpin): sum_g w_g e_g is
        compute_xc_spin's Exc.  With option quirks = 1 a functional with vwn5_c or pbe_c is refused, as by compute_xc_spin."""
        return self._xc_energy_density(self.lib.DFT_ComputeXCEnergyDensitySpin, [d_dm_a, d_dm_b], ngrid, nao, d_ao, d_e_out, d_ao_grad)

    def _declare_meta_gradient(self):
        L = self.lib
        # added without a change of DFT_GetVersion: a library without them cannot serve the gradient of a meta-GGA
        if not hasattr(L, "DFT_ComputeXCGradientMeta") or not hasattr(L, "DFT_ComputeXCEnergyDensityMeta"):
            raise RuntimeError("the library has no DFT_ComputeXCGradientMeta / DFT_ComputeXCEnergyDensityMeta: it cannot run the "
                               "nuclear gradient of a meta-GGA")
        L.DFT_ComputeXCGradientMeta.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [_u64] * 6
        L.DFT_ComputeXCGradientMeta.restype = ctypes.c_int
        L.DFT_ComputeXCEnergyDensityMeta.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [_u64] * 4
        L.DFT_ComputeXCEnergyDensityMeta.restype = ctypes.c_int
        return L

    def compute_xc_gradient_meta(self, ngrid, nao, d_dm, d_ao, d_weights, d_out, d_ao_grad=None, d_ao_hess=None):
        """G (nao, 3) into d_out (DFT_ComputeXCGradientMeta): the derivative of compute_xc_meta's Exc by the centre of every
        basis function at fixed points and weights, the tau term included (gradients.xc_gradient_meta_host is its host
        counterpart); a solver with meta weights, d_ao_grad and d_ao_hess always.  Option xcg_meta_fused chooses the one-pass
        kernel (1) or the plain form (0).  Asynchronous on the solver's stream."""
        return self._xc_gradient(self._declare_meta_gradient().DFT_ComputeXCGradientMeta, [d_dm], ngrid, nao, d_ao, d_weights, d_out, d_ao_grad, d_ao_hess)

    def compute_xc_energy_density_meta(self, ngrid, nao, d_dm, d_ao, d_e_out, d_ao_grad=None):
        """e_g of a meta-GGA at the density and tau of d_dm into d_e_out (ngrid) without the weight
        (DFT_ComputeXCEnergyDensityMeta): sum_g w_g e_g is compute_xc_meta's Exc.  Asynchronous on the solver's stream."""
        return self._xc_energy_density(self._declare_meta_gradient().DFT_ComputeXCEnergyDensityMeta, [d_dm], ngrid, nao, d_ao, d_e_out, d_ao_grad)

    def _declare_meta_spin_gradient(self):
        L = self.lib
        # added without a change of DFT_GetVersion: a library without them cannot serve the gradient of an open-shell meta-GGA
        if not hasattr(L, "DFT_ComputeXCGradientMetaSpin") or not hasattr(L, "DFT_ComputeXCEnergyDensityMetaSpin"):
            raise RuntimeError("the library has no DFT_ComputeXCGradientMetaSpin / DFT_ComputeXCEnergyDensityMetaSpin: it cannot run "
                               "the nuclear gradient of an open-shell meta-GGA")
        L.DFT_ComputeXCGradientMetaSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [_u64] * 7
        L.DFT_ComputeXCGradientMetaSpin.restype = ctypes.c_int
        L.DFT_ComputeXCEnergyDensityMetaSpin.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [_u64] * 5
        L.DFT_ComputeXCEnergyDensityMetaSpin.restype = ctypes.c_int
        return L

    def compute_xc_gradient_meta_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao, d_weights, d_out, d_ao_grad=None, d_ao_hess=None):
        """G (nao, 3) into d_out (DFT_ComputeXCGradientMetaSpin): the derivative of compute_xc_meta_spin's Exc by the centre of
        every basis function at fixed points and weights, the tau term of either spin included
        (gradients.xc_gradient_meta_spin_host is its host counterpart); a solver with meta weights, d_ao_grad and d_ao_hess
        always.  Option xcg_meta_spin_fused chooses the one-pass kernel (1) or the plain form (0).  Asynchronous on the
        solver's stream."""
        return self._xc_gradient(self._declare_meta_spin_gradient().DFT_ComputeXCGradientMetaSpin, [d_dm_a, d_dm_b], ngrid, nao, d_ao,
                                 d_weights, d_out, d_ao_grad, d_ao_hess)

    def compute_xc_energy_density_meta_spin(self, ngrid, nao, d_dm_a, d_dm_b, d_ao, d_e_out, d_ao_grad=None):
        """e_g of a meta-GGA at the spin densities and taus of d_dm_a / d_dm_b into d_e_out (ngrid) without the weight
        (DFT_ComputeXCEnergyDensityMetaSpin): sum_g w_g e_g is compute_xc_meta_spin's Exc.  Asynchronous on the solver's stream."""
        return self._xc_energy_density(self._declare_meta_spin_gradient().DFT_ComputeXCEnergyDensityMetaSpin, [d_dm_a, d_dm_b], ngrid, nao,
                                       d_ao, d_e_out, d_ao_grad)

    def becke_weight_gradient(self, ngrid, atom_xyz, atom_radius, d_coords, d_owner, d_f, d_out, d_cell_out=None):
        """sum_g f_g D_B cell_g into d_out (natm, 3) (DFT_BeckeWeightGradient; grid_gen.becke_weight_gradient_host is its
        host counterpart): atom_xyz (natm, 3) and atom_radius (natm; grid_gen.bragg_radii_bohr) are host arrays, d_coords
        (ngrid, 3) fp64, d_owner (ngrid) int32 in [0, natm), d_f (ngrid) fp64 device arrays; d_cell_out (ngrid) receives the
        cell function when given.  Asynchronous on the solver's stream."""
        import numpy as np
        dp = ctypes.POINTER(ctypes.c_double)
        xyz = np.ascontiguousarray(atom_xyz, dtype=np.float64).reshape(-1, 3)
        rad = np.ascontiguousarray(atom_radius, dtype=np.float64).reshape(-1)
        if rad.shape[0] != xyz.shape[0]:
            raise ValueError(f"becke_weight_gradient: {xyz.shape[0]} atoms but {rad.shape[0]} radii")
        rc = self.lib.DFT_BeckeWeightGradient(self.solver, int(ngrid), int(xyz.shape[0]), xyz.ctypes.data_as(dp), rad.ctypes.data_as(dp),
                                              _u64(_ptr(d_coords)), _u64(_ptr(d_owner)), _u64(_ptr(d_f)), _u64(_ptr(d_cell_out)),
                                              _u64(_ptr(d_out)))
        self._check()
        return rc

    def mix(self):
        """The solver's weights as the library reports them (DFT_GetMix; for a built-in type: its equivalent mix)."""
        out = (ctypes.c_double * len(functionals.COMPONENTS))()
        if self.lib.DFT_GetMix(self.solver, out, len(out)) != 0:
            raise RuntimeError("DFT_GetMix failed")
        return list(out)

    def set_option(self, key, value):
        if self.lib.DFT_SetOption(self.solver, key.encode(), float(value)) != 0:
            raise KeyError(key)

    def get_option(self, key):
        """Read-back of an option, or of what the library did with it ("publish_probe", "publish_live", "used_publish")."""
        v = self.lib.DFT_GetOption(self.solver, key.encode())
        if v != v:
            raise KeyError(key)
        return v

    def set_stream(self, hip_stream):
        self.lib.DFT_SetStream(self.solver, _u64(int(hip_stream)))

    def last_error(self):
        return (self.lib.DFT_GetLastError(self.solver) or b"").decode()

    def timings(self, max_entries=16):
        ms = (ctypes.c_double * max_entries)()
        names = (ctypes.c_char_p * max_entries)()
        n = self.lib.DFT_GetTimings(self.solver, ms, names, max_entries)
        return [(names[i].decode(), ms[i]) for i in range(n)]

    def _check(self):
        err = self.lib.DFT_GetLastError(self.solver)
        if err:
            raise RuntimeError("libdft: " + err.decode())
