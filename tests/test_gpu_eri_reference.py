"""DFT_EriColumns / DFT_EriColumnsMany (csrc/eri_cols.hip) against the independent high-precision reference stored in
tests/golden/eri_ref_z{1,2,3}.npz (oracle/eri_reference.py: another formulation, mpmath's incomplete gamma function,
its own harmonics and normalisation; tests/test_eri_reference_cpu.py holds the evidence that the reference is right and
compares the host engine with the same files).  Reads only tests/golden/; needs no mpmath.

  Z1  seven shells s p d f d p s (3 2 2 1 1 3 2 primitives) on four centres, 25 functions: every (bra class, ket class),
      both team sizes, every accumulator count, contracted d on the workgroup path, 4 / 6 / 9 primitive pairs per wave team
  Z2  single primitives s..f on X (bra) and Y (ket), six separations: x = 0, x around the 1e-13 switch of the Boys
      function, the short series, x = 20-31 (the long series; an asymptote used here would be wrong by 1e-10), x around
      the switch at 40, and x ~ 1300-2000
  Z3  the C-H fragment in def2-TZVP (37 functions, exponents up to 13 575, the primitive cut active)

Bound: eri_fixtures.BOUND = 1e-12 * max(1, max|ref| of the column block) in every family -- the level at which host and
device agree with each other.  The host engine's worst error against the reference is 2.5e-14 (the R = 3e-7 geometry;
<= 1.5e-15 elsewhere), so no family needed a bound derived from a 53-bit run of the reference; tools/eri_reference_parity.py
writes both engines' figures per family (profiles/eri_reference_parity.txt).

Layout: the device (like the host with lower_only) writes the shell blocks A >= B, diagonal blocks whole; that covers
every element i >= j, which is all the consumer reads.  Every block A < B must come back zero from a buffer that held a
sentinel, and the elements i < j inside a diagonal shell block must hold the mirrored value (eri_fixtures.shell_lower_mask)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import eri_fixtures as F  # noqa: E402
from quantum_compute_dft_amd import integrals  # noqa: E402

SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _open(sh):
    host = integrals.EriColumns(sh)
    q = integrals.schwarz_bounds(sh, host.diag())
    host.close()
    return integrals.DeviceEriColumns(sh, q), q


def _nq(sh, C, D):
    return (2 * int(sh.l[C]) + 1) * (2 * int(sh.l[D]) + 1)


def _cols(devc, sh, C, D, screen, dev):
    buf = torch.full((_nq(sh, C, D) * sh.nao * sh.nao,), SENTINEL, dtype=torch.float64, device=dev)
    return devc.cols(C, D, screen, buf).cpu().numpy()


def _check(got, ref, what, extra=0.0):
    """Element by element over the WHOLE block (zeros of the blocks A < B included); returns the error."""
    assert got.shape == ref.shape, what
    err = float(np.abs(got - ref).max())
    allowed = F.BOUND * max(1.0, float(np.abs(ref).max())) + extra
    assert err <= allowed, (what, err, allowed)
    return err


def _upper_blocks_are_zero(got, sh, n=None):
    return not np.any(got[:, ~F.shell_lower_mask(sh, n)])


def test_z1_every_ket_pair_element_by_element(dev):
    f = F.z1()
    sh = f["sh"]
    devc, _ = _open(sh)
    own = np.repeat(np.arange(sh.nshell), 2 * sh.l + 1)
    worst, calls = {}, 0
    for C in range(sh.nshell):
        for D in range(C + 1):
            ref = F.z1_columns(C, D)
            orders = [((C, D), ref)]
            if (C, D) in ((1, 0), (3, 2), (5, 3), (6, 4)):                              # the swapped order of the same pair
                orders.append(((D, C), F.swapped(ref, 2 * int(sh.l[C]) + 1, 2 * int(sh.l[D]) + 1)))
            for (c, d), r in orders:
                got = _cols(devc, sh, c, d, 0.0, dev)
                _check(got, r, ("z1", c, d))
                assert _upper_blocks_are_zero(got, sh), ("z1", c, d)
                calls += 1
                e = np.abs(got - r).max(axis=0)                                         # (nao, nao)
                for A in range(sh.nshell):
                    for B in range(A + 1):
                        key = (int(sh.l[A]), int(sh.l[B]), int(sh.l[c]), int(sh.l[d]))
                        worst[key] = max(worst.get(key, 0.0), float(e[np.ix_(own == A, own == B)].max()))
    devc.close()
    assert len(worst) == 256                                                            # 16 ordered bra classes x 16 ordered ket classes
    assert calls == 28 + 4                                                              # no pair left out; _check covers whole blocks
    print("\nworst |device - reference| on Z1 per (bra class | ket class), rows la lb, columns lc ld:")
    for la in range(4):
        for lb in range(4):
            print("spdf"[la] + "spdf"[lb], " ".join("%.1e" % worst[(la, lb, lc, ld)] for lc in range(4) for ld in range(4)))


def test_z1_all_pairs_in_one_call(dev):
    f = F.z1()
    sh = f["sh"]
    devc, _ = _open(sh)
    pairs = [(C, D) for C in range(sh.nshell) for D in range(C + 1)]
    ref = np.concatenate([F.z1_columns(C, D) for C, D in pairs])
    assert len(pairs) == 28
    buf = torch.full((ref.size,), SENTINEL, dtype=torch.float64, device=dev)
    got = devc.cols_many(pairs, 0.0, buf).cpu().numpy()
    devc.close()
    o = 0
    for C, D in pairs:
        nq = _nq(sh, C, D)
        _check(got[o:o + nq], ref[o:o + nq], ("z1 many", C, D))
        o += nq
    assert _upper_blocks_are_zero(got, sh)


@pytest.mark.parametrize("g", range(6))
def test_z2_boys_regimes(dev, g):
    z = F.z2()[g]
    sh = z["sh"]
    devc, _ = _open(sh)
    for (C, D), ref in zip(z["kets"], z["cols"]):
        got = _cols(devc, sh, C, D, 0.0, dev)
        err = _check(got[:, :16, :16], ref, ("z2", z["R"], C, D))
        assert _upper_blocks_are_zero(got, sh)
        print("z2 R = %g ket (%d, %d): worst |device - reference| %.2e, max|ref| %.2e" % (z["R"], C, D, err, np.abs(ref).max()))
    devc.close()


def test_z3_shipped_table(dev):
    z = F.z3()
    sh = z["sh"]
    devc, _ = _open(sh)
    for (C, D), ref in zip(z["kets"], z["cols"]):
        orders = [((C, D), ref)]
        if (C, D) == z["kets"][2]:                                                      # (p_H, s_H) in the swapped order too
            orders.append(((D, C), F.swapped(ref, 2 * int(sh.l[C]) + 1, 2 * int(sh.l[D]) + 1)))
        for (c, d), r in orders:
            got = _cols(devc, sh, c, d, 0.0, dev)
            err = _check(got, r, ("z3", c, d))
            assert _upper_blocks_are_zero(got, sh)
            print("z3 ket (%d, %d): worst |device - reference| %.2e, max|ref| %.2e" % (c, d, err, np.abs(r).max()))
    devc.close()


def _skipped_blocks(got, ref, sh, n):
    """Shell blocks A >= B of a column block that came back all zero although the reference is not."""
    own = np.repeat(np.arange(sh.nshell), 2 * sh.l + 1)[:n]
    count = 0
    for A in range(int(own.max()) + 1):
        for B in range(A + 1):
            ix = np.ix_(range(got.shape[0]), own == A, own == B)
            count += int(not np.any(got[ix]) and np.any(ref[ix]))
    return count


def test_screening_against_the_truth(dev):
    """Schwarz bounds from the host diagonal.  What the device skips at `screen` must really be that small: the result
    stays within screen + the parity bound of the UNSCREENED reference.

    * Z1 and the R = 40 geometry of Z2 at screen = 1e-10.  In Z1 the smallest product of two shell-pair bounds is
      2.6e-3, so nothing may be skipped there and the test catches a screen that fires too early.  At R = 40 every bra
      pair with one shell on X and one on Y has a bound of exactly zero and is skipped; its integrals underflow to zero
      as well, so its zeros do not tell a skip from a computation, and the stored X-X blocks must be untouched.
    * Z1 at screen = 1e-2, where products of bounds do fall below the screen: here at least one block must come back as
      zeros where the reference is not zero, or the test would prove nothing about skipping."""
    f = F.z1()
    sh = f["sh"]
    devc, q = _open(sh)
    assert np.outer(q, q).min() > 1e-10
    for screen in (1e-10, 1e-2):
        skipped = 0
        for C in range(sh.nshell):
            for D in range(C + 1):
                ref = F.z1_columns(C, D)
                got = _cols(devc, sh, C, D, screen, dev)
                _check(got, ref, ("z1 screened", screen, C, D), extra=screen)
                skipped += _skipped_blocks(got, ref, sh, sh.nao)
        assert (skipped == 0) if screen == 1e-10 else (skipped >= 1), (screen, skipped)
    devc.close()
    z = F.z2()[-1]
    assert z["R"] == 40.0
    sh = z["sh"]
    devc, q = _open(sh)
    assert np.outer(q, q).min() < 1e-10
    for (C, D), ref in zip(z["kets"], z["cols"]):
        got = _cols(devc, sh, C, D, 1e-10, dev)
        _check(got[:, :16, :16], ref, ("z2 screened", C, D), extra=1e-10)
        assert not np.any(got[:, 16:, :16]), "bra pairs across 40 bohr have a Schwarz bound of zero"
        assert _upper_blocks_are_zero(got, sh)
    devc.close()
