"""Cartesian BFGS geometry optimiser on the analytic nuclear gradient (gradients.nuclear_gradient).

`bfgs(fun, xyz0)` minimises E over the 3 natm Cartesian coordinates (bohr) with fun(xyz) -> (E, g (natm, 3)): the inverse
Hessian starts as the identity (1 bohr^2 / Ha, on the soft side of a bond stretch, so first steps are short of the
quadratic one rather than beyond it) and takes the standard BFGS update when the step has positive curvature; no atom
moves further than `step_cap` in a step; a step that raises the energy is halved (at most four times) before it is
taken.  Converged at max|g| < gmax and rms(g) < grms, the customary 3e-4 / 2e-4 Ha / bohr.  No internal coordinates, no
constraints, no symmetry: rigid translations and rotations are left to the gradient, which has (almost) no component
along them -- the gradient is the derivative at fixed quadrature points, so its net force is not exactly zero
(README), and the thresholds have to stay well above it.
"""
import numpy as np

GMAX, GRMS, STEP_CAP = 3e-4, 2e-4, 0.3
BOHR = 0.52917721092


def converged(g, gmax=GMAX, grms=GRMS):
    g = np.asarray(g, dtype=np.float64)
    return bool(np.abs(g).max() < gmax and np.sqrt(np.mean(g * g)) < grms)


def bfgs(fun, xyz0, max_steps=50, gmax=GMAX, grms=GRMS, step_cap=STEP_CAP, log=None):
    """{"xyz" (natm, 3), "energy", "gradient", "energies" [E of every accepted geometry, the first included], "steps",
    "evaluations", "converged"}."""
    x = np.array(xyz0, dtype=np.float64)
    shape, n = x.shape, x.size
    Hinv = np.eye(n)
    E, g = fun(x)
    g = np.asarray(g, dtype=np.float64)
    energies, evals, steps = [float(E)], 1, 0
    if log:
        log(f"opt step {0:3d}: E = {E:.10f} Ha   max|g| = {np.abs(g).max():.2e}   rms = {np.sqrt(np.mean(g * g)):.2e}")
    while not converged(g, gmax, grms) and steps < max_steps:
        p = -(Hinv @ g.reshape(n)).reshape(shape)
        if float(np.sum(p * g)) >= 0.0:       # not a descent direction: the update went bad, start over from steepest descent
            Hinv = np.eye(n)
            p = -g.copy()
        longest = float(np.linalg.norm(p, axis=1).max())
        if longest > step_cap:
            p *= step_cap / longest
        for _ in range(5):
            En, gn = fun(x + p)
            evals += 1
            if En <= E + 1e-9:
                break
            p *= 0.5
        gn = np.asarray(gn, dtype=np.float64)
        s, y = p.reshape(n), (gn - g).reshape(n)
        sy = float(s @ y)
        if sy > 1e-10:
            Hy = Hinv @ y
            Hinv = Hinv + (1.0 + float(y @ Hy) / sy) * np.outer(s, s) / sy - (np.outer(Hy, s) + np.outer(s, Hy)) / sy
        x, E, g = x + p, En, gn
        steps += 1
        energies.append(float(E))
        if log:
            log(f"opt step {steps:3d}: E = {E:.10f} Ha   max|g| = {np.abs(g).max():.2e}   rms = {np.sqrt(np.mean(g * g)):.2e}   "
                f"longest move {np.linalg.norm(p, axis=1).max():.4f} bohr")
    return {"xyz": x, "energy": float(E), "gradient": g, "energies": energies, "steps": steps, "evaluations": evals,
            "converged": converged(g, gmax, grms)}


def write_xyz(path, symbols, xyz_bohr, comment=""):
    """The geometry as an .xyz file (Angstrom), readable by basis.parse_xyz."""
    with open(path, "w") as fh:
        fh.write(f"{len(symbols)}\n{comment}\n")
        for s, r in zip(symbols, np.asarray(xyz_bohr, dtype=np.float64) * BOHR):
            fh.write(f"{s:2s} {r[0]:18.12f} {r[1]:18.12f} {r[2]:18.12f}\n")
