"""HalfWaveT::chol_solve_packed (sgrl_amd/csrc/wave_half.h) on the CPU: the register solver lcp_block_pivot uses for its one
right-hand side per pivoting round, driven alone on the lane fibers of tests/emu/emu_pair.cpp (tests/emu/emu_chol_solve.cpp): sizes
around the instance boundaries (3 / 6 / 9 / 12 / 15) and the cap, the clamped pivot, and two halves of one wavefront with different sizes.

Accuracy has no constant of its own: every case is solved in extended precision, and the new path's relative error may not exceed
TWICE that of the explicit-inverse path it replaces (chol_inv_packed, x = T'(T rhs)) on the same input -- substitution is normally the
more accurate of the two; the factor covers a different rounding order."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chol_cases as cc

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        d = os.path.join(_HERE, "emu")
        so = os.path.join(d, "libsgrl_emu_chol.so")
        csrc = os.path.join(_HERE, "..", "sgrl_amd", "csrc")
        srcs = [os.path.join(d, "emu_chol_solve.cpp"), os.path.join(d, "emu_pair.cpp"), os.path.join(csrc, "step_body.h"),
                os.path.join(csrc, "wave_half.h"), os.path.join(_HERE, "..", "include", "sgrl_model.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, srcs[0], "-lm"])
        _LIB = ctypes.CDLL(so)
    return _LIB


def run(problems, inverse=False):
    """Both halves at once: (ok, x of each problem, the packed matrices as the call left them, the inputs)."""
    n, C, x = cc.slots(problems)
    C0, x0 = C.copy(), x.copy()
    ok = np.full(2, -1, dtype=np.int32)
    rc = lib().sgrl_emu_chol_solve(int(inverse), n.ctypes.data_as(ctypes.c_void_p), C.ctypes.data_as(ctypes.c_void_p),
                                   x.ctypes.data_as(ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, {-1: "bad n", -2: "the lanes of a half diverged (deadlock)", -3: "an access left its buffer"}.get(rc, rc)
    return ok, [x[p * 32:p * 32 + n[p]] for p in range(2)], C, (C0, x0)


@pytest.mark.parametrize("n", [1, 3, 4, 6, 7, 9, 10, 15])
def test_solution_is_no_worse_than_the_explicit_inverse_path(n):
    A, rhs = cc.case(n)
    ok, xs, _, _ = run([(A, rhs), None])
    ok_old, xs_old, _, _ = run([(A, rhs), None], inverse=True)
    assert ok[0] == 1 and ok_old[0] == 1
    ext = cc.solve_ext(A, rhs)
    e_new, e_old = cc.rel_err(xs[0], ext), cc.rel_err(xs_old[0], ext)
    print("half wave n = %2d: relative error new %.3e  explicit inverse %.3e" % (n, e_new, e_old))
    assert e_new <= 2.0 * e_old
    # and it is the operation order the header states (CPU build: no contraction, 1 / sqrt)
    ref = cc.restate(A, rhs, fused=False)
    assert np.abs(xs[0] - ref).max() <= 8 * cc.EPS * np.abs(ref).max()


def test_beyond_the_cap_returns_false_and_touches_nothing():
    A, rhs = cc.case(16)
    ok, xs, C, (C0, _) = run([(A, rhs), cc.case(9)])
    assert list(ok) == [0, 1]                                 # the mate within the cap is solved all the same
    assert np.array_equal(C[:cc.LD], C0[:cc.LD]) and np.array_equal(xs[0], rhs)
    assert cc.rel_err(xs[1], cc.solve_ext(*cc.case(9))) < 1e-9


@pytest.mark.parametrize("na,nb", [(3, 14), (15, 0), (10, 9)])
def test_a_half_does_not_depend_on_its_wave_mate(na, nb):
    """Two free sets of different size classes in one wavefront: each half's result is the one it gets alone, bit for bit."""
    pa = cc.case(na, seed=1)
    pb = cc.case(nb, seed=2) if nb else None
    ok, xs, C, _ = run([pa, pb])
    ok_a, xs_a, C_a, _ = run([pa, None])
    assert ok[0] == 1 and ok_a[0] == 1 and ok[1] == 1
    assert np.array_equal(xs[0], xs_a[0]) and np.array_equal(C[:cc.LD], C_a[:cc.LD])
    if pb is not None:
        ok_b, xs_b, C_b, _ = run([None, pb])
        assert ok_b[1] == 1
        assert np.array_equal(xs[1], xs_b[1]) and np.array_equal(C[cc.LD:], C_b[cc.LD:])
        ok_s, xs_s, _, _ = run([pb, pa])                  # and the half it runs in does not matter either
        assert np.array_equal(xs_s[0], xs[1]) and np.array_equal(xs_s[1], xs[0])
    assert cc.rel_err(xs[0], cc.solve_ext(*pa)) < 1e-9


@pytest.mark.parametrize("n", [9, 12])
def test_clamped_pivot_gives_the_restated_finite_result(n):
    """Two equal rows of Y, R = 0: pivot 1 falls under kMinVal (chol_cases.clamp_case says why the case is built as it is)."""
    A, rhs = cc.clamp_case(n)
    ok, xs, _, _ = run([None, (A, rhs)])
    x = xs[1]
    assert ok[1] == 1 and np.isfinite(x).all()
    ref = cc.restate(A, rhs, fused=False)
    assert np.abs(x[:2]).min() > 1e14                         # the clamp decided these two: of the order of 1 / kMinVal
    assert (np.abs(x[:2] - ref[:2]) <= 8 * cc.EPS * np.abs(ref[:2])).all()
    # the other rows are an ordinary SPD system of their own: held like every other case
    ext = cc.solve_ext(A[2:, 2:], rhs[2:])
    ok_old, xs_old, _, _ = run([None, (A, rhs)], inverse=True)
    e_new, e_old = cc.rel_err(x[2:], ext), cc.rel_err(xs_old[1][2:], ext)
    print("half wave clamp n = %2d: relative error of the regular rows new %.3e  explicit inverse %.3e" % (n, e_new, e_old))
    assert e_new <= 2.0 * e_old
