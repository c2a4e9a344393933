"""Reader of tests/golden/grad_ref_g{1,2,3}.npz (written by tests/golden/make_grad_reference.py from
oracle/eri_reference.py): four shells on four centres, fixed symmetric D, M, W, and the 100-digit centre derivatives of
the two-electron energy and of the one-electron traces, rounded to double.  Needs neither mpmath nor the oracle package.

Bound of every comparison with these fixtures (tests/test_grad_reference_cpu.py, tests/test_gpu_grad2e_reference.py):

    |got - ref| <= BOUND * max|ref| of the compared (4, 3) array,    BOUND = eri_fixtures.BOUND = 1e-12.

Measured figures of both engines: profiles/grad2e_reference_parity.txt."""
import functools
import os

import numpy as np

import eri_fixtures as F

BOUND = F.BOUND
FAMILIES = ("g1", "g2", "g3")
PROFILE = "grad2e_reference_parity.txt"


@functools.lru_cache(maxsize=None)
def family(name, reverse=False):
    """dict of family `name`, its shells as stored or (`reverse`) listed in the opposite order with D, M, W permuted and
    the reference rows reordered with them: sh (basis.ShellTable), D, M, W, c_hf (2,), g2e (2, 4, 3), g2e_spin (2, 4, 3),
    g1e (3, 4, 3), charge_xyz, charge_z, meta; part_quartets, part_values as stored (shell numbers of the file's order).
    Read-only arrays, shared between the tests."""
    d = F._load(f"grad_ref_{name}.npz")
    n = len(d["l"])
    order = list(range(n))[::-1] if reverse else list(range(n))
    poff = np.concatenate([[0], np.cumsum(d["nprim"])])
    aoff = np.concatenate([[0], np.cumsum(2 * d["l"] + 1)])
    prim = np.concatenate([np.arange(poff[s], poff[s + 1]) for s in order])
    ao = np.concatenate([np.arange(aoff[s], aoff[s + 1]) for s in order])
    sh = F.shell_table(d["centre"][order], d["l"][order], d["nprim"][order], d["exp"][prim], d["coef"][prim])
    out = dict(sh=sh, c_hf=d["c_hf"], charge_xyz=d["charge_xyz"], charge_z=d["charge_z"], meta=d["meta"], name=name, reverse=reverse,
               part_quartets=d["part_quartets"], part_values=d["part_values"])
    for k in "DMW":
        out[k] = np.ascontiguousarray(d[k][np.ix_(ao, ao)])
    for k in ("g2e", "g2e_spin", "g1e"):
        out[k] = np.ascontiguousarray(d[k][:, order])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def label(f, what):
    return f"{f['name']}{' reversed' if f['reverse'] else ''} {what}"


def record(tag, what, ref, err):
    """One line per comparison into grad2e_reference_parity.txt in the directory QCDFT_WRITE_PROFILES names (how
    profiles/grad2e_reference_parity.txt was made); an ordinary test run only prints."""
    line = f"{tag + ' ' + what:60s} max|ref| {ref:9.2e}   |engine - ref| / max|ref| {err:9.2e}"
    print(line)
    out_dir = os.environ.get("QCDFT_WRITE_PROFILES")
    if not out_dir:
        return
    path = os.path.join(out_dir, PROFILE)
    try:
        os.makedirs(out_dir, exist_ok=True)
        old = [l.rstrip("\n") for l in open(path)] if os.path.exists(path) else []
        head = [l for l in old if l.startswith("#")] or [
            "# Derivative integrals against the 100-digit reference of tests/golden/grad_ref_g{1,2,3}.npz (oracle/eri_reference.py):",
            "# cpu = csrc/integrals.c (tests/test_grad_reference_cpu.py), gpu = csrc/grad2e.hip (tests/test_gpu_grad2e_reference.py);",
            "# the tests' bound is 1e-12 of max|ref|.  Lines marked (ref = host): the device against the host engine on the two",
            "# molecules whose ket-slice loop runs several times per workgroup; bound max(10 bar, 1e-13), bar in grad2e_parity.txt.",
            "# Written with QCDFT_WRITE_PROFILES=profiles."]
        body = [l for l in old if l and not l.startswith("#") and not l.startswith(f"{tag + ' ' + what:60s}")]
        with open(path, "w") as fh:
            fh.write("\n".join(head + sorted(body + [line])) + "\n")
    except OSError:
        pass


def check(tag, what, got, ref):
    """Asserts |got - ref| <= BOUND max|ref| over the whole array; returns the measured error / max|ref|."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max() / scale)
    record(tag, what, scale, err)
    assert scale > 0.0 and err <= BOUND, (what, err)
    return err
