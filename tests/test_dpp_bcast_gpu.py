"""The register linear algebra of the step kernel with the lane broadcast INSIDE the FMA instruction (v_fmac_f64_dpp row_newbcast:
sgrl_amd/csrc/wave_hip.h fnma_bcast16_run / fnma_bcast16_self, used by chol_inv_reg / chol_solve_reg of both wave policies) against the
lane-read form it replaced.  The two are the same operations in the same order -- fmac(acc, bcast(x), -l) and fma(-l, bcast(x), acc) are
one rounding of the same product and sum -- so there is no tolerance: everything either form stores must be equal BIT FOR BIT.

Both forms run through the test hooks sgrl_debug_chol_inv and sgrl_debug_chol_solve_form (include/sgrl.h), one 64-lane workgroup each;
form 0 exists in those hooks only.  Sizes on both sides of the 16-lane DPP row (beyond it the full wave mirrors the multiplier column
across rows and keeps lane reads where a row cannot serve itself), two halves of different size classes, the clamped pivot, and the
sizes past each policy's cap."""
import ctypes

import numpy as np
import pytest

import chol_cases as cc

pytestmark = pytest.mark.gpu

FULL, HALF = 0, 1
NEW, OLD = 1, 0


def _lib():
    from sgrl_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    L.sgrl_debug_chol_inv.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    L.sgrl_debug_chol_solve_form.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    return _lib, L


def inv(form, policy, problems):
    """(ok, the packed L^-1 slots as chol_inv_packed left them, the packed inputs)."""
    _l, L = _lib()
    n, C, _ = cc.slots(problems)
    C_out = np.full(2 * cc.LD, np.nan)
    ok = np.full(2, -1, dtype=np.int32)
    _l.check(L.sgrl_debug_chol_inv(form, policy, n.ctypes.data, C.ctypes.data, C_out.ctypes.data, ok.ctypes.data), "sgrl_debug_chol_inv")
    return ok, C_out, C


def solve(form, policy, problems):
    """(ok, the x slots, the packed matrices as chol_solve_packed left them, the packed inputs, the right-hand sides)."""
    _l, L = _lib()
    n, C, x = cc.slots(problems)
    C_out, x_out = np.full(2 * cc.LD, np.nan), np.full(64, np.nan)
    ok = np.full(2, -1, dtype=np.int32)
    _l.check(L.sgrl_debug_chol_solve_form(form, policy, n.ctypes.data, C.ctypes.data, x.ctypes.data, C_out.ctypes.data, x_out.ctypes.data,
                                          ok.ctypes.data), "sgrl_debug_chol_solve_form")
    return ok, x_out, C_out, C, x


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _forms_agree(policy, problems, live):
    """Both hooks, both forms, on the same problems: equal bit for bit, finite where a problem lives, and solved."""
    ok_n, Li_n, _ = inv(NEW, policy, problems)
    ok_o, Li_o, _ = inv(OLD, policy, problems)
    sk_n, x_n, C_n, _, _ = solve(NEW, policy, problems)
    sk_o, x_o, C_o, _, _ = solve(OLD, policy, problems)
    for p in live:
        assert ok_n[p] == 1 and ok_o[p] == 1 and sk_n[p] == 1 and sk_o[p] == 1
        n = problems[p][0].shape[0]
        assert np.isfinite(Li_n[p * cc.LD:(p + 1) * cc.LD]).all() and np.isfinite(x_n[p * 32:p * 32 + n]).all()
    assert _same_bits(Li_n, Li_o)
    assert _same_bits(x_n, x_o) and _same_bits(C_n, C_o)
    return x_n, Li_n, C_n


@pytest.mark.parametrize("n", [1, 3, 9, 15, 16, 17, 18, 21, 24])
def test_full_wave_new_form_equals_the_lane_read_form(n):
    A, rhs = cc.case(n)
    x, _, _ = _forms_agree(FULL, [(A, rhs), None], live=[0])
    assert cc.rel_err(x[:n], cc.solve_ext(A, rhs)) < 1e-9          # and it is the solution (not two equal wrong answers)


@pytest.mark.parametrize("n", [1, 9, 15])
def test_half_wave_new_form_equals_the_lane_read_form(n):
    A, rhs = cc.case(n)
    slot = n & 1
    problems = [None, None]
    problems[slot] = (A, rhs)
    x, _, _ = _forms_agree(HALF, problems, live=[slot])
    assert cc.rel_err(x[slot * 32:slot * 32 + n], cc.solve_ext(A, rhs)) < 1e-9


@pytest.mark.parametrize("na,nb", [(3, 14), (15, 0)])
def test_two_halves_equal_the_lane_read_form_and_their_solo_results(na, nb):
    pa = cc.case(na, seed=1)
    pb = cc.case(nb, seed=2) if nb else None
    live = [0, 1] if nb else [0]
    x, Li, C = _forms_agree(HALF, [pa, pb], live=live)
    for p, pr in ((0, pa), (1, pb)):
        if pr is None:
            continue
        solo = [None, None]
        solo[p] = pr
        _, Li_s, _ = inv(NEW, HALF, solo)
        _, x_s, C_s, _, _ = solve(NEW, HALF, solo)
        sl, xs = slice(p * cc.LD, (p + 1) * cc.LD), slice(p * 32, p * 32 + pr[0].shape[0])
        assert _same_bits(Li[sl], Li_s[sl]) and _same_bits(C[sl], C_s[sl]) and _same_bits(x[xs], x_s[xs])


@pytest.mark.parametrize("policy,n", [(FULL, 12), (FULL, 20), (HALF, 9)])
def test_clamped_pivot_equals_the_lane_read_form(policy, n):
    """Two equal rows of Y, R = 0 (chol_cases.clamp_case): pivot 1 falls under kMinVal and the clamp decides it, in both forms alike."""
    A, rhs = cc.clamp_case(n)
    problems = [None, None]
    problems[policy] = (A, rhs)
    x, _, _ = _forms_agree(policy, problems, live=[policy])
    assert np.abs(x[policy * 32:policy * 32 + 2]).min() > 1e14     # the clamp decided these two: of the order of 1 / kMinVal


@pytest.mark.parametrize("policy,n", [(FULL, 25), (HALF, 16)])
def test_beyond_the_cap_both_hooks_return_false_and_touch_nothing(policy, n):
    A, rhs = cc.case(n)
    problems = [(A, rhs), cc.case(9) if policy else None]
    for form in (NEW, OLD):
        ok, Li, C_in = inv(form, policy, problems)
        assert ok[0] == 0 and _same_bits(Li[:cc.LD], C_in[:cc.LD])
        ok, x, C_out, C_in, x_in = solve(form, policy, problems)
        assert ok[0] == 0 and _same_bits(C_out[:cc.LD], C_in[:cc.LD]) and _same_bits(x[:32], x_in[:32])
        if policy:                                                 # the mate within the cap is solved all the same
            assert ok[1] == 1 and cc.rel_err(x[32:32 + 9], cc.solve_ext(*cc.case(9))) < 1e-9
