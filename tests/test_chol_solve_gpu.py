"""chol_solve_packed on the device (sgrl_amd/csrc/wave_hip.h HipWaveT, wave_half.h HalfWaveT on the DPP primitives): the register
solver lcp_block_pivot uses for its one right-hand side per pivoting round, run alone in one 64-lane workgroup through the test hook
sgrl_debug_chol_solve (include/sgrl.h).  Sizes at the instance boundaries (3 / 6 / 9 / 12 / 15 / 18 / 21 / 24), with slack inside an
instance, and past each policy's cap; the clamped pivot; two halves of one wavefront with different sizes.

Accuracy has no constant of its own: every case is solved in extended precision on the host, the explicit-inverse path the primitive
replaces (chol_inv_packed, x = T'(T rhs); the hook's flag bit 1) runs on the same input, and the new path's relative error may not
exceed TWICE the old one's.  Substitution is normally the more accurate of the two; the factor covers a different rounding order.
Measured pairs: profiles/lcp_solve_ab.txt."""
import ctypes

import numpy as np
import pytest

import chol_cases as cc

pytestmark = pytest.mark.gpu

HALF, INVERSE = 1, 2


def run(problems, flags):
    """(ok, x of each problem, the packed matrices as the call left them, the packed inputs)."""
    from sgrl_amd import _lib
    L = _lib.lib()
    n, C, x = cc.slots(problems)
    C_out, x_out = np.full(2 * cc.LD, np.nan), np.full(64, np.nan)
    ok = np.full(2, -1, dtype=np.int32)
    vp = ctypes.c_void_p
    L.sgrl_debug_chol_solve.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp]
    rc = L.sgrl_debug_chol_solve(flags, n.ctypes.data, C.ctypes.data, x.ctypes.data, C_out.ctypes.data, x_out.ctypes.data, ok.ctypes.data)
    _lib.check(rc, "sgrl_debug_chol_solve")
    return ok, [x_out[p * 32:p * 32 + n[p]] for p in range(2)], C_out, C


def _held_to_the_old_path(tag, A, rhs, flags, slot=0, rows=slice(None)):
    problems = [None, None]
    problems[slot] = (A, rhs)
    ok, xs, _, _ = run(problems, flags)
    ok_old, xs_old, _, _ = run(problems, flags | INVERSE)
    assert ok[slot] == 1 and ok_old[slot] == 1
    assert np.isfinite(xs[slot]).all()
    ext = cc.solve_ext(A[rows, rows], rhs[rows])
    e_new, e_old = cc.rel_err(xs[slot][rows], ext), cc.rel_err(xs_old[slot][rows], ext)
    print("%s: relative error new %.3e  explicit inverse %.3e" % (tag, e_new, e_old))
    assert e_new <= 2.0 * e_old
    return xs[slot]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 6, 7, 8, 9, 10, 15, 16, 23, 24])
def test_full_wave_is_no_worse_than_the_explicit_inverse_path(n):
    _held_to_the_old_path("full wave n = %2d" % n, *cc.case(n), flags=0)


@pytest.mark.parametrize("n", [1, 3, 4, 6, 7, 9, 10, 15])
def test_half_wave_is_no_worse_than_the_explicit_inverse_path(n):
    _held_to_the_old_path("half wave n = %2d" % n, *cc.case(n), flags=HALF, slot=n & 1)


@pytest.mark.parametrize("flags,n", [(0, 25), (HALF, 16)])
def test_beyond_the_cap_returns_false_and_touches_nothing(flags, n):
    A, rhs = cc.case(n)
    ok, xs, C_out, C_in = run([(A, rhs), cc.case(9) if flags else None], flags)
    assert ok[0] == 0
    assert np.array_equal(C_out[:cc.LD], C_in[:cc.LD]) and np.array_equal(xs[0], rhs)
    if flags:                                                 # the mate within the cap is solved all the same
        assert ok[1] == 1 and cc.rel_err(xs[1], cc.solve_ext(*cc.case(9))) < 1e-9


@pytest.mark.parametrize("na,nb", [(3, 14), (15, 0)])
def test_a_half_does_not_depend_on_its_wave_mate(na, nb):
    """Two free sets of different size classes in one wavefront: each half's result is the one it gets alone, bit for bit."""
    pa = cc.case(na, seed=1)
    pb = cc.case(nb, seed=2) if nb else None
    ok, xs, C, _ = run([pa, pb], HALF)
    ok_a, xs_a, C_a, _ = run([pa, None], HALF)
    assert ok[0] == 1 and ok_a[0] == 1 and ok[1] == 1
    assert np.array_equal(xs[0], xs_a[0]) and np.array_equal(C[:cc.LD], C_a[:cc.LD])
    assert cc.rel_err(xs[0], cc.solve_ext(*pa)) < 1e-9
    if pb is not None:
        ok_b, xs_b, C_b, _ = run([None, pb], HALF)
        assert ok_b[1] == 1
        assert np.array_equal(xs[1], xs_b[1]) and np.array_equal(C[cc.LD:], C_b[cc.LD:])
        assert cc.rel_err(xs[1], cc.solve_ext(*pb)) < 1e-9


@pytest.mark.parametrize("flags,n", [(0, 12), (0, 20), (HALF, 9)])
def test_clamped_pivot_gives_the_restated_finite_result(flags, n):
    """Two equal rows of Y, R = 0: pivot 1 falls under kMinVal (chol_cases.clamp_case says why the case is built as it is).  The two
    clamped entries against a host restatement of the same operation order (fused multiply-subtracts as the device build contracts
    them), to a few ulp: the restatement's 1 / sqrt and the device's rsqrt may differ by an ulp or two, the entries are two or three
    roundings further on -- eight ulp.  The regular rows are held like every other case."""
    A, rhs = cc.clamp_case(n)
    x = _held_to_the_old_path("%s wave clamp n = %2d, regular rows" % ("half" if flags else "full", n), A, rhs, flags, slot=flags & 1,
                              rows=slice(2, None))
    ref = cc.restate(A, rhs, fused=True)
    assert np.abs(x[:2]).min() > 1e14                         # the clamp decided these two: of the order of 1 / kMinVal
    print("clamped entries", x[:2], "restated", ref[:2])
    assert (np.abs(x[:2] - ref[:2]) <= 8 * cc.EPS * np.abs(ref[:2])).all()
