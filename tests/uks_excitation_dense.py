"""Dense reference for the open-shell excitation tests, modelled on excitation_dense.py: A+B and A-B as matrices from an
excitations.UksResponseOperators applied to every unit vector of its stacked space, and their solution by LAPACK
(tests/test_spin_response_cpu.py, tests/test_gpu_spin_response.py)."""
import numpy as np


def dense_matrices(ops):
    """(A+B, A-B) as (N, N) matrices, N = ops.size: column n is the operator on unit vector n."""
    P, Q = ops.apply(np.eye(ops.size))
    return P.T.copy(), Q.T.copy()


def dense_solution(ops, ApB, AmB, tda):
    """(w ascending, f) of the whole spectrum: TDA eigh((A+B + A-B)/2); TDDFT (A-B)^1/2 (A+B) (A-B)^1/2 T = w^2 T,
    X+Y = (A-B)^1/2 T / sqrt(w); f = 2/3 w |dip . (X+Y)|^2 (both spins are in the vector: no sqrt(2))."""
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
    mu = ops.dip_flat @ xpy
    return w, (2.0 / 3.0) * w * np.einsum("kn,kn->n", mu, mu)
