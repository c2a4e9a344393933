"""The device-resident end of an SCF cycle (csrc/scf_tail.hip, DFT_ScfTail*) against the host loop's own numpy classes
(scf.CDIIS, scf.OccupiedRotation) on the same inputs, and the fused loop against the host loop on a real molecule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

import quantum_compute_dft_amd as q  # noqa: E402
from quantum_compute_dft_amd import scf, scf_tail  # noqa: E402

# largest per-cycle |E_tot(fused) - E_tot(host)| allowed; measured on an MI355X: 5.7e-8, 8.9e-8 and 4.6e-7 Ha
CYCLE_GAP = {("Benzene", "GGA"): 5e-7, ("Benzene", "B3LYP"): 5e-7, ("Anthracene", "B3LYP"): 2.5e-6}


def _problem(n, no, seed, c_hf):
    """A Fock-like problem with a gap: S near 1, H with a split spectrum, small symmetric J / K and a non-symmetric Vxc."""
    rng = np.random.default_rng(seed)
    B = 0.1 * rng.standard_normal((n, n))
    S = np.eye(n) + 0.5 * (B + B.T) / np.sqrt(n)
    s, V = np.linalg.eigh(S)
    X = V / np.sqrt(s)
    lev = np.concatenate([np.sort(rng.uniform(-10.0, -0.5, no)), np.sort(rng.uniform(0.2, 4.0, n - no))])
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    Xi = np.linalg.inv(X)
    H = Xi.T @ (Q * lev) @ Q.T @ Xi          # X^T H X has the spectrum `lev`
    H = 0.5 * (H + H.T)
    sym = lambda a: 0.5 * (a + a.T)
    mats = [(0.02 * sym(rng.standard_normal((n, n))), 0.02 * sym(rng.standard_normal((n, n))), 0.02 * rng.standard_normal((n, n))) for _ in range(12)]
    return S, X, H, mats


def _host_cycle(S, H, J, K, V, c_hf, dm, cocc, diis, rot, tol):
    """dft.py:212-236 as scf._run_scf does it."""
    F = H + J + 0.5 * (V + V.T) - (0.5 * c_hf * K if c_hf else 0.0)
    F = diis.update(S, dm, F, cocc=cocc)
    e, C = rot.occupied(F, tol)
    cn = np.sqrt(2.0) * np.asarray(C)
    dn = cn @ cn.T
    return F, dn, cn, (np.sum(dn * H), 0.5 * np.sum(dn * J), -0.25 * c_hf * np.sum(dn * K) if c_hf else 0.0, np.linalg.norm(dn - dm))


@pytest.mark.parametrize("n,no,c_hf", [(30, 7, 0.0), (114, 21, 0.0), (114, 21, 0.2), (128, 32, 0.2), (17, 1, 0.0), (45, 30, 0.2),
                                       (150, 20, 0.2), (246, 47, 0.2), (130, 64, 0.0), (300, 33, 0.0),    # these and the next: operands in memory
                                       (129, 32, 0.0), (127, 33, 0.2), (512, 48, 0.0), (6, 2, 0.0), (33, 32, 0.2)])
def test_tail_steps_match_the_host_classes(n, no, c_hf):
    import torch
    dev = torch.device("cuda:0")
    S, X, H, mats = _problem(n, no, 100 + n + no, c_hf)
    lib = q.load_library(q.library_path())
    tail = scf_tail.ScfTail(lib, H, S, no, dev)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    # cycle 0: the full diagonalisation of H (both sides start from the same basis)
    from scipy.linalg import eigh
    e0, Cp = eigh(X.T @ H @ X, driver="evd")
    U0 = X @ Cp
    rot = scf.OccupiedRotation(S, no, None)
    rot.U = U0.copy()
    diis = scf.CDIIS()
    tail.basis.copy_(t(U0))
    cocc = np.sqrt(2.0) * U0[:, :no]
    dm = cocc @ cocc.T
    d_dm, d_cocc = t(dm), t(cocc)
    d_exc = torch.zeros(1, dtype=torch.float64, device=dev)
    for cyc, (J, K, V) in enumerate(mats):
        tol = 1e-10
        d_exc.fill_(-1.25 - cyc)
        Fh, dn, cn, (e1, e2, e3, dd) = _host_cycle(S, H, J, K, V, c_hf, dm, cocc, diis, rot, tol)
        d_J, d_K, d_V = t(J), (t(K) if c_hf else None), t(V)
        tail.step(True, c_hf, tol, d_J, d_K, d_V, d_dm, d_cocc, canon_tol=1e-6, d_exc=d_exc)
        o = tail.wait()
        assert o[4] == scf_tail.STATUS_DONE, (cyc, o)
        assert o[7] == -1.25 - cyc                                                         # the sweep's Exc travels with the step's scalars
        scale = np.abs(Fh).max()
        assert np.abs(tail.fock.cpu().numpy() - Fh).max() <= 1e-11 * scale, cyc           # Fock assembly + DIIS
        got_dm = d_dm.cpu().numpy()
        assert np.abs(got_dm - dn).max() <= 2e-9, (cyc, np.abs(got_dm - dn).max())         # the rotated occupied space (fixed point to 1e-10)
        c_got = d_cocc.cpu().numpy()
        assert np.abs(c_got @ c_got.T - got_dm).max() <= 1e-12                            # dm = cocc cocc^T
        Ub = tail.basis.cpu().numpy()
        assert np.abs(Ub.T @ S @ Ub - np.eye(n)).max() <= 1e-11                           # the basis stays S-orthonormal
        assert np.abs(np.sqrt(2.0) * Ub[:, :no] - c_got).max() <= 1e-13
        Aoo = Ub[:, :no].T @ Fh @ Ub[:, :no]
        assert np.abs(Aoo - np.diag(np.diag(Aoo))).max() <= 1e-7                          # ... and canonical in the occupied block
        assert np.abs(np.diag(Aoo) - tail.mo_energy.cpu().numpy()[:no]).max() <= 1e-9
        for got, ref in zip(o[:4], (e1, e2, e3, dd)):
            assert abs(got - ref) <= 1e-9 * max(1.0, abs(ref)), (cyc, o, (e1, e2, e3, dd))
        assert o[5] >= 1
        # both sides continue from THEIR OWN state (they agree to ~1e-10: the trajectories stay together)
        dm, cocc = dn, cn
    tail.close()


def _first_order_step(U, F, no):
    """max |K0| of the rotation's first-order step -A_vo / (a_v - a_o), A = U^T F U (both kernels refuse above 0.5)."""
    A = U.T @ F @ U
    d = np.diag(A)
    return np.abs(A[:no, no:] / (d[no:][None, :] - d[:no][:, None])).max()


@pytest.mark.parametrize("n,no", [(40, 9),                                    # k_tail_rot: operands in LDS
                                  (150, 20), (127, 33), (512, 64)])           # k_rb_*: above 128 functions or 32 occupied
def test_status_paths_diis_only_finish_and_singular_system(n, no):
    import torch
    from scipy.linalg import eigh
    dev = torch.device("cuda:0")
    c_hf = 0.2
    S, X, H, mats = _problem(n, no, 5, c_hf)
    lib = q.load_library(q.library_path())
    tail = scf_tail.ScfTail(lib, H, S, no, dev)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    e0, Cp = eigh(X.T @ H @ X, driver="evd")
    U0 = X @ Cp
    cocc = np.sqrt(2.0) * U0[:, :no]
    dm = cocc @ cocc.T
    d_dm, d_cocc = t(dm), t(cocc)
    J, K, V = mats[0]
    d_J, d_K, d_V = t(J), t(K), t(V)
    # DIIS only: status 1, the Fock matrix is there, nothing else changed
    tail.step(False, c_hf, 1e-10, d_J, d_K, d_V, d_dm, d_cocc)
    o = tail.wait()
    assert o[4] == scf_tail.STATUS_DIAGONALISE
    F = H + J + 0.5 * (V + V.T) - 0.5 * c_hf * K
    assert np.abs(tail.fock.cpu().numpy() - F).max() <= 1e-13 * np.abs(F).max()
    assert np.array_equal(d_dm.cpu().numpy(), dm) and np.array_equal(d_cocc.cpu().numpy(), cocc)
    # the caller diagonalises and finishes
    e1, Cp1 = eigh(X.T @ F @ X, driver="evd")
    U1 = X @ Cp1
    tail.basis.copy_(t(U1))
    tail.finish(c_hf, d_J, d_K, d_dm, d_cocc)
    o = tail.wait()
    cn = np.sqrt(2.0) * U1[:, :no]
    dn = cn @ cn.T
    assert o[4] == scf_tail.STATUS_DONE
    assert np.abs(d_dm.cpu().numpy() - dn).max() <= 1e-13 and np.abs(d_cocc.cpu().numpy() - cn).max() <= 1e-15
    for got, ref in zip(o[:4], (np.sum(dn * H), 0.5 * np.sum(dn * J), -0.25 * c_hf * np.sum(dn * K), np.linalg.norm(dn - dm))):
        assert abs(got - ref) <= 1e-11 * max(1.0, abs(ref))
    # a rotation that must be refused: a Fock matrix far from the basis (first-order step above 0.5)
    Jbig = J + 3.0 * (lambda a: a + a.T)(np.random.default_rng(1).standard_normal((n, n)))
    assert _first_order_step(U1, H + Jbig + 0.5 * (V + V.T) - 0.5 * c_hf * K, no) > 0.5    # the construction holds at this n too
    before = tail.basis.clone()
    tail.reset()                                   # no history: DIIS would otherwise extrapolate the outlier away
    tail.step(True, c_hf, 1e-10, t(Jbig), d_K, d_V, d_dm, d_cocc)
    o = tail.wait()
    assert o[4] == scf_tail.STATUS_DIAGONALISE and torch.equal(tail.basis, before)
    # the same (F, e) pair twice in the ring: a singular Pulay system -> status 2 -> coefficients from the host
    tail.reset()
    d_dm2, d_cocc2 = t(dn), t(cn)
    tail.step(False, c_hf, 1e-10, d_J, d_K, d_V, d_dm2, d_cocc2)
    assert tail.wait()[4] == scf_tail.STATUS_DIAGONALISE
    tail.step(False, c_hf, 1e-10, d_J, d_K, d_V, d_dm2, d_cocc2)
    o = tail.wait()
    assert o[4] == scf_tail.STATUS_SINGULAR, o
    cf = tail.pulay_coefficients_on_host()
    assert abs(cf.sum() - 1.0) <= 1e-12
    tail.step(False, c_hf, 1e-10, d_J, d_K, d_V, d_dm2, d_cocc2, coef=cf, repeat=True)
    o = tail.wait()
    assert o[4] == scf_tail.STATUS_DIAGONALISE
    assert np.abs(tail.fock.cpu().numpy() - F).max() <= 1e-12 * np.abs(F).max()      # any weights summing to 1 of two equal matrices
    tail.close()
    assert scf_tail.supported(114, 21) and scf_tail.supported(494, 47) and not scf_tail.supported(1150, 250)


def _waits_needed(steps, hint, more):
    """Waits of one step whose fixed point takes `steps` steps when `hint` are queued with it and `more` per continuation."""
    return 1 if steps <= hint else 1 + -(-(steps - hint) // more)


class _SplitRun:
    """One ScfTail driven through the C entry points, without ScfTail.wait()'s continuation and hint logic: every step queues
    `hint` fixed-point steps (the library clamps it to [1, 60]), every status 3 is continued by DFT_ScfTailMore(`more`).  Counts
    the waits of each step."""

    def __init__(self, lib, H, S, no, U0, dev, hint, more):
        import torch
        self.torch, self.lib, self.hint, self.more = torch, lib, hint, more
        self.queued = min(max(hint, 1), 60)
        self.tail = scf_tail.ScfTail(lib, H, S, no, dev)
        self.tail.basis.copy_(torch.as_tensor(U0, device=dev))
        cocc = np.sqrt(2.0) * U0[:, :no]
        self.d_dm = torch.as_tensor(cocc @ cocc.T, device=dev)
        self.d_cocc = torch.as_tensor(cocc, device=dev)
        self.d_exc = torch.zeros(1, dtype=torch.float64, device=dev)
        self.waits, self.split_parities = [], set()

    def _wait(self):
        assert self.lib.DFT_ScfTailWait(self.tail._h, self.tail._out) == 0
        return list(self.tail._out)

    def cycle(self, c_hf, tol, d_J, d_K, d_V, exc, max_inner=60):
        tail, h = self.tail, self.tail._h
        assert self.lib.DFT_ScfTailSetStepsHint(h, self.hint) == 0
        self.d_exc.fill_(exc)
        dm0, cocc0 = self.d_dm.clone(), self.d_cocc.clone()
        tail.step(True, c_hf, tol, d_J, d_K, d_V, self.d_dm, self.d_cocc, canon_tol=1e-6, max_inner=max_inner, d_exc=self.d_exc)
        o, waits, done = self._wait(), 1, self.queued
        while o[4] == scf_tail.STATUS_MORE:                # a partial wait: the step has not touched dm / cocc
            assert self.torch.equal(self.d_dm, dm0) and self.torch.equal(self.d_cocc, cocc0)
            self.split_parities.add(done % 2)              # the K / K2 buffer the iteration stands in at the split
            rc = self.lib.DFT_ScfTailMore(h, self.more, d_J.data_ptr(), 0 if d_K is None else d_K.data_ptr(), self.d_dm.data_ptr(),
                                          self.d_cocc.data_ptr(), self.d_exc.data_ptr())
            assert rc == 0
            o, waits, done = self._wait(), waits + 1, done + self.more
            assert waits <= 61
        assert waits == _waits_needed(int(o[5]), self.queued, self.more), (waits, o)   # ... and every wait before the last reported 3
        self.waits.append(waits)
        return o

    def state(self):
        t = self.tail
        return [x.clone() for x in (t.fock, t.basis, t.mo_energy, self.d_dm, self.d_cocc)]


def _assert_same_step(o, st, o_ref, st_ref, what):
    import torch
    assert o[4] == o_ref[4] and o[5] == o_ref[5], (what, o, o_ref)                  # final status, fixed-point steps
    assert o[:4] == o_ref[:4] and o[7] == o_ref[7], (what, o, o_ref)                # the energy traces, |dm' - dm|, Exc
    for name, x, y in zip(("fock", "basis", "mo_energy", "dm", "cocc"), st, st_ref):
        assert torch.equal(x, y), (what, name, (x - y).abs().max().item())


@pytest.mark.parametrize("n,no", [(129, 32), (150, 20), (246, 47), (300, 33), (512, 64)])
@pytest.mark.parametrize("c_hf", [0.0, 0.2])
def test_split_step_equals_the_unsplit_step(n, no, c_hf):
    """The memory-resident rotation queues its fixed-point steps as launches of their own; a step that runs out of them ends in
    status 3 and DFT_ScfTailMore continues it.  The same kernels run in the same order whichever way the steps are split, so the
    results are equal bit for bit: (a) every step queued at once, (b) one step at a time, (c) 2, then 3 per continuation (splits
    after 2, 5, 8, ... steps: the iteration stands in either K buffer).  (b) also against the host classes."""
    import torch
    from scipy.linalg import eigh
    dev = torch.device("cuda:0")
    S, X, H, mats = _problem(n, no, 100 + n + no, c_hf)
    lib = q.load_library(q.library_path())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    e0, Cp = eigh(X.T @ H @ X, driver="evd")
    U0 = X @ Cp
    runs = {k: _SplitRun(lib, H, S, no, U0, dev, hint, more) for k, hint, more in (("a", 60, 1), ("b", 1, 1), ("c", 2, 3))}
    rot = scf.OccupiedRotation(S, no, None)
    rot.U = U0.copy()
    diis = scf.CDIIS()
    cocc = np.sqrt(2.0) * U0[:, :no]
    dm = cocc @ cocc.T
    for cyc, (J, K, V) in enumerate(mats[:4]):
        tol = 1e-10
        d_J, d_K, d_V = t(J), (t(K) if c_hf else None), t(V)
        out = {k: (r.cycle(c_hf, tol, d_J, d_K, d_V, -1.25 - cyc), r.state()) for k, r in runs.items()}
        o_a, st_a = out["a"]
        assert o_a[4] == scf_tail.STATUS_DONE and o_a[5] >= 1 and o_a[7] == -1.25 - cyc, (cyc, o_a)
        for k in ("b", "c"):
            _assert_same_step(*out[k], o_a, st_a, (k, cyc))
        # (b) against scf.CDIIS / scf.OccupiedRotation, tolerances of test_tail_steps_match_the_host_classes
        Fh, dn, cn, ref = _host_cycle(S, H, J, K, V, c_hf, dm, cocc, diis, rot, tol)
        o, (F, Ub, e, got_dm, c_got) = out["b"]
        F, Ub, got_dm, c_got = (x.cpu().numpy() for x in (F, Ub, got_dm, c_got))
        assert np.abs(F - Fh).max() <= 1e-11 * np.abs(Fh).max(), cyc
        assert np.abs(got_dm - dn).max() <= 2e-9, (cyc, np.abs(got_dm - dn).max())
        assert np.abs(c_got @ c_got.T - got_dm).max() <= 1e-12
        assert np.abs(Ub.T @ S @ Ub - np.eye(n)).max() <= 1e-11
        assert np.abs(np.sqrt(2.0) * Ub[:, :no] - c_got).max() <= 1e-13
        Aoo = Ub[:, :no].T @ Fh @ Ub[:, :no]
        assert np.abs(Aoo - np.diag(np.diag(Aoo))).max() <= 1e-7
        assert np.abs(np.diag(Aoo) - e.cpu().numpy()[:no]).max() <= 1e-9
        for got, r in zip(o[:4], ref):
            assert abs(got - r) <= 1e-9 * max(1.0, abs(r)), (cyc, o, ref)
        dm, cocc = dn, cn
    assert runs["a"].waits == [1] * 4
    assert max(runs["b"].waits) >= 2 and max(runs["c"].waits) >= 2           # continuations happened: not a vacuous pass
    assert runs["b"].split_parities == {0, 1} and runs["c"].split_parities == {0, 1}, (runs["b"].waits, runs["c"].waits)
    for r in runs.values():
        r.tail.close()


@pytest.mark.parametrize("n,no,c_hf", [(150, 20, 0.2), (246, 47, 0.0), (512, 64, 0.2)])
def test_max_inner_runs_out_across_continuations(n, no, c_hf):
    """Fewer fixed-point steps allowed than the step needs: status 1 (the caller diagonalises) whether the steps ran in one go or
    across continuations, after exactly `max_inner` steps, with dm / cocc / the basis untouched and the same Fock matrix."""
    import torch
    from scipy.linalg import eigh
    dev = torch.device("cuda:0")
    S, X, H, mats = _problem(n, no, 7 + n, c_hf)
    lib = q.load_library(q.library_path())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    e0, Cp = eigh(X.T @ H @ X, driver="evd")
    U0 = X @ Cp
    J, K, V = mats[0]
    d_J, d_K, d_V = t(J), (t(K) if c_hf else None), t(V)
    probe = _SplitRun(lib, H, S, no, U0, dev, 60, 1)
    need = int(probe.cycle(c_hf, 1e-10, d_J, d_K, d_V, 0.5)[5])
    probe.tail.close()
    assert need >= 4, need
    max_inner = need - 1
    ref = None
    for hint, more in ((60, 1), (1, 1), (2, 3), (max_inner, 1)):
        r = _SplitRun(lib, H, S, no, U0, dev, hint, more)
        before = r.state()
        o = r.cycle(c_hf, 1e-10, d_J, d_K, d_V, 0.5, max_inner=max_inner)
        st = r.state()
        assert o[4] == scf_tail.STATUS_DIAGONALISE and o[5] == max_inner, (hint, o)
        assert r.waits == [_waits_needed(max_inner, hint, more)]
        dm0, cocc0 = before[3].cpu().numpy(), before[4].cpu().numpy()
        assert np.array_equal(st[3].cpu().numpy(), dm0) and np.array_equal(st[4].cpu().numpy(), cocc0), hint
        assert torch.equal(st[1], before[1]), hint                                      # the basis stays
        if ref is None:
            ref = (o, st)
        else:
            assert o == ref[0] and torch.equal(st[0], ref[1][0]), hint                # same scalars, same Fock matrix
        r.tail.close()


def test_continuation_and_hint_api_edges():
    """DFT_ScfTailMore only continues a memory-resident step and needs nsteps >= 1; DFT_ScfTailSetStepsHint clamps to [1, 60]
    (below 1: one step per launch group; above 60: everything in one go, the same results)."""
    import ctypes
    import torch
    from scipy.linalg import eigh
    dev = torch.device("cuda:0")
    lib = q.load_library(q.library_path())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    # the LDS kernel has nothing to continue
    S, X, H, mats = _problem(40, 9, 3, 0.2)
    small = scf_tail.ScfTail(lib, H, S, 9, dev)
    J, K, V = (t(m) for m in mats[0])
    dm, cocc = t(np.eye(40)), t(np.eye(40)[:, :9])
    ex = torch.zeros(1, dtype=torch.float64, device=dev)
    more = lambda h, k: lib.DFT_ScfTailMore(h, k, J.data_ptr(), K.data_ptr(), dm.data_ptr(), cocc.data_ptr(), ex.data_ptr())
    assert more(small._h, 1) == -1 and more(small._h, 8) == -1
    assert more(None, 1) == -1 and lib.DFT_ScfTailSetStepsHint(None, 4) == -1
    small.close()
    # the memory-resident one: nsteps < 1 is refused; hints outside [1, 60] act as the nearest end
    n, no, c_hf = 200, 24, 0.2
    S, X, H, mats = _problem(n, no, 11, c_hf)
    e0, Cp = eigh(X.T @ H @ X, driver="evd")
    U0 = X @ Cp
    J, K, V = mats[0]
    d_J, d_K, d_V = t(J), t(K), t(V)
    big = scf_tail.ScfTail(lib, H, S, no, dev)
    dm, cocc = t(np.eye(n)), t(np.eye(n)[:, :no])
    for k in (0, -1, -60):
        assert lib.DFT_ScfTailMore(big._h, k, d_J.data_ptr(), d_K.data_ptr(), dm.data_ptr(), cocc.data_ptr(), ex.data_ptr()) == -1
    big.close()
    ref = None
    for hint in (60, 61, 1000, 1, 0, -5):
        r = _SplitRun(lib, H, S, no, U0, dev, hint, 1)
        o = r.cycle(c_hf, 1e-10, d_J, d_K, d_V, 0.25)
        st = r.state()
        assert o[4] == scf_tail.STATUS_DONE and o[5] >= 2, (hint, o)
        assert r.waits == [1 if hint >= 60 else int(o[5])], (hint, r.waits)        # hint <= 1: a wait per fixed-point step
        if ref is None:
            ref = (o, st)
        else:
            _assert_same_step(o, st, *ref, hint)
        r.tail.close()


@pytest.fixture(scope="module")
def molecules():
    """inputs.build(name, def2-SVP, grid level 3) and a fused-loop HipBackend per (name, functional, eri), each made once here."""
    import torch
    from quantum_compute_dft_amd import inputs
    dev = torch.device("cuda:0")
    built, backends = {}, {}

    def get(name, eri, functional=None):
        if (name, eri) not in built:
            built[name, eri] = inputs.build(name, "def2-svp", 3, device=dev, verbose=False, eri_mode=eri, chol_tol=1e-8)
        inp = built[name, eri]
        if functional is None:
            return inp
        if (name, eri, functional) not in backends:
            backends[name, eri, functional] = scf.HipBackend(inp, functional, device=dev)
        return inp, backends[name, eri, functional]

    yield get
    backends.clear(); built.clear()


def _fused_run(inp, be, functional, prequeue, hint_cap=scf_tail.STEPS_HINT_CAP, max_inner=60):
    """One fused-loop SCF from the same start: the steps hint back at its initial value (capped), the given knobs, then restored.
    max_inner None: each rotation may take no more fixed-point steps than the last one that went through."""
    tail = be.tail
    be.prequeue, tail.hint_cap, tail.max_inner = prequeue, hint_cap, 60 if max_inner is None else max_inner
    if max_inner is None:
        wait = tail.wait

        def tightening_wait():
            o = wait()
            if o[4] == scf_tail.STATUS_DONE and o[5] > 0:
                tail.max_inner = o[5]
            return o
        tail.wait = tightening_wait
    try:
        tail.set_steps_hint(min(scf_tail.STEPS_HINT, hint_cap))
        be.occ_solver.reset()
        return scf.run_scf(inp, be, functional, log=None)
    finally:
        be.prequeue, tail.hint_cap, tail.max_inner = True, scf_tail.STEPS_HINT_CAP, 60
        tail.__dict__.pop("wait", None)


# (molecule, functional, eri, cap of the steps hint, max_inner): Benzene/def2-SVP is 114 functions / 21 occupied (LDS rotation
# kernel), Anthracene 246 / 47 (memory-resident: its fixed-point steps are launches of their own, continued after status 3)
_PREQUEUE_CASES = {
    "benzene-gga-dense": ("Benzene", "GGA", "dense", scf_tail.STEPS_HINT_CAP, 60),
    "anthracene-b3lyp": ("Anthracene", "B3LYP", "cholesky", scf_tail.STEPS_HINT_CAP, 60),
    "anthracene-b3lyp-hint1": ("Anthracene", "B3LYP", "cholesky", 1, 60),               # a continuation in most cycles
    # rotations refused mid-run, right after one that went through (parts queued ahead).  A fixed small max_inner does not get
    # there on Anthracene: a refusal is followed by a full diagonalisation, after which the rotations need ever fewer steps
    # (measured: max_inner 1 to 8 refuse 2 to 3 cycles in a row, then none).  A max_inner that follows the last rotation does:
    # the default run's steps go 9 6 5 4 2 2 2 3 ...
    "anthracene-b3lyp-max-inner": ("Anthracene", "B3LYP", "cholesky", scf_tail.STEPS_HINT_CAP, None),
}


@pytest.mark.parametrize("case", list(_PREQUEUE_CASES))
def test_prequeued_parts_change_no_result(case, molecules):
    """With one rank the fused loop queues cycle k+1's J / K and XC sweep behind cycle k's tail, before it has seen the tail's
    status.  When the tail does not write the new density in that step -- a refused rotation (status 1), or a memory-resident
    rotation continued by DFT_ScfTailMore (status 3) -- those parts read the old one and must be queued again.  Either way the
    loop computes what it computes with nothing queued ahead: the same cycles, bit for bit."""
    name, functional, eri, hint_cap, max_inner = _PREQUEUE_CASES[case]
    inp, be = molecules(name, eri, functional)
    r_on = _fused_run(inp, be, functional, True, hint_cap, max_inner)
    r_off = _fused_run(inp, be, functional, False, hint_cap, max_inner)
    assert r_on["loop"] == "fused" and r_off["loop"] == "fused"
    diff = [(k + 1, a[0] - b[0], a[1] - b[1]) for k, (a, b) in enumerate(zip(r_on["per_cycle"], r_off["per_cycle"])) if a != b]
    assert not diff, f"(cycle, dE_tot, d|ddm|) with parts queued ahead against none: {diff[:4]}"
    assert r_on["cycles"] == r_off["cycles"] and r_on["converged"] and r_off["converged"], (r_on["cycles"], r_off["cycles"])
    assert np.array_equal(r_on["dm"], r_off["dm"]) and np.array_equal(r_on["mo_energy"], r_off["mo_energy"])
    assert not any(ahead for *_, ahead in r_off["tail_log"])
    log = r_on["tail_log"]
    continued = sum(1 for s in log if s[3]); continued_ahead = sum(1 for s in log if s[3] and s[4])
    refused = sum(1 for s in log if s[0] == scf_tail.STATUS_DIAGONALISE); refused_ahead = sum(1 for s in log if s[0] == 1 and s[4])
    print(f"{case}: {r_on['cycles']} cycles, {continued} continued ({continued_ahead} with parts queued ahead), "
          f"{refused} refused ({refused_ahead} with parts queued ahead)")
    if name == "Benzene":
        assert continued == 0                                                          # the LDS kernel runs every step in one launch
    if hint_cap == 1:
        assert continued_ahead >= 1
    if max_inner is None:
        assert refused_ahead >= 1


@pytest.mark.parametrize("molecule,functional,eri", [("Benzene", "GGA", "dense"), ("Benzene", "B3LYP", "cholesky"), ("Anthracene", "B3LYP", "cholesky")])
def test_fused_loop_matches_the_host_loop(molecule, functional, eri, molecules):
    """Same molecule, same thresholds (dft.py:243): the loop with its host part on the device against the host loop."""
    import torch
    dev = torch.device("cuda:0")
    inp = molecules(molecule, eri)
    host = scf.HipBackend(inp, functional, device=dev, device_resident=False)      # Anthracene (246 functions, 47 occupied): the memory-resident rotation kernel
    assert host.tail is None
    r_host = scf.run_scf(inp, host, functional, log=None)
    fused = scf.HipBackend(inp, functional, device=dev)
    assert fused.tail is not None
    r_fused = scf.run_scf(inp, fused, functional, log=None)
    assert r_host["converged"] and r_fused["converged"] and r_fused["loop"] == "fused"
    assert abs(r_host["E_tot"] - r_fused["E_tot"]) <= 2e-8, (r_host["E_tot"], r_fused["E_tot"])
    assert abs(r_host["cycles"] - r_fused["cycles"]) <= 1
    assert np.abs(r_host["dm"] - r_fused["dm"]).max() <= 1e-5
    assert np.abs(np.asarray(r_host["mo_energy"]) - np.asarray(r_fused["mo_energy"])).max() <= 1e-5
    # every cycle, not only the last: a cycle built from the previous density's J / K / Vxc is off by about its |dE| (1e-4 to
    # 1e-2 Ha early on).  The rotation's tolerance adapts to the last |ddm| (up to 1e-5), so early cycles differ slightly.
    gaps = [abs(a[0] - b[0]) for a, b in zip(r_host["per_cycle"], r_fused["per_cycle"])]
    assert len(gaps) >= r_fused["cycles"] - 1 and max(gaps) <= CYCLE_GAP[molecule, functional], gaps
    st = fused.occ_solver.stats
    assert st["rotated"] >= r_fused["cycles"] // 2 and st["exact"] >= 1
    # a second run on the same backend starts afresh
    fused.occ_solver.reset()
    r2 = scf.run_scf(inp, fused, functional, log=None)
    assert r2["converged"] and abs(r2["E_tot"] - r_fused["E_tot"]) <= 1e-9 and r2["cycles"] == r_fused["cycles"]
