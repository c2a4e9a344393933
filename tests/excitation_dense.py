"""Dense reference for the excitation tests: A+B and A-B as matrices from an excitations.ResponseOperators applied to
every unit vector, and their solution by LAPACK (tests/test_excitations_cpu.py, tests/test_gpu_excitations.py)."""
import numpy as np


def dense_matrices(ops):
    """(A+B, A-B) as (N, N) matrices, N = nocc nvirt: column n is the operator on unit vector n."""
    nocc, nvirt = ops.gap.shape
    N = nocc * nvirt
    P, Q = ops.apply(np.eye(N).reshape(N, nocc, nvirt))
    return P.reshape(N, N).T.copy(), Q.reshape(N, N).T.copy()


def dense_solution(ops, ApB, AmB, tda):
    """(w ascending, f) of the whole spectrum: TDA eigh((A+B + A-B)/2); TDDFT (A-B)^1/2 (A+B) (A-B)^1/2 T = w^2 T,
    X+Y = (A-B)^1/2 T / sqrt(w); f = 2/3 w |sqrt(2) dip . (X+Y)|^2."""
    ApB, AmB = 0.5 * (ApB + ApB.T), 0.5 * (AmB + AmB.T)
    if tda:
        w, xpy = np.linalg.eigh(0.5 * (ApB + AmB))
    else:
        s, U = np.linalg.eigh(AmB)
        assert s[0] > 0.0
        S = (U * np.sqrt(s)) @ U.T
        w2, T = np.linalg.eigh(S @ ApB @ S)
        w = np.sqrt(w2)
        xpy = (S @ T) / np.sqrt(w)[None, :]
    mu = np.sqrt(2.0) * ops.dip.reshape(3, -1) @ xpy
    return w, (2.0 / 3.0) * w * np.einsum("kn,kn->n", mu, mu)
