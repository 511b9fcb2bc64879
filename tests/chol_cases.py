"""Shared inputs and host arithmetic of the chol_solve_packed tests (test_chol_solve_emu.py on the CPU fibers, test_chol_solve_gpu.py on
the device): the SPD systems, the packed layout of the debug entry points, an extended-precision solve as the truth and a restatement
of the primitive's own operation order."""
import functools
from fractions import Fraction

import numpy as np

LD = 352            # doubles per packed-triangle slot of sgrl_debug_chol_solve / sgrl_emu_chol_solve
MINVAL = 1e-15      # step_body.h kMinVal
EPS = float(np.finfo(np.float64).eps)


@functools.lru_cache(maxsize=None)
def case(n, seed=0):
    """A = Y Y' + diag(R), Y n x 24 from a fixed seed, R log-uniform in 1e-6 .. 1e-2, right-hand side of mixed sign."""
    rng = np.random.RandomState(1000 * seed + n)
    Y = rng.standard_normal((max(n, 1), 24))[:n]
    R = 10.0 ** rng.uniform(-6, -2, size=n)
    rhs = rng.uniform(0.2, 1.5, size=n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    A = Y @ Y.T + np.diag(R)
    A.setflags(write=False)
    rhs.setflags(write=False)
    return A, rhs


@functools.lru_cache(maxsize=None)
def clamp_case(n):
    """Rows 0 and 1 of Y equal, R = 0: pivot 1 is zero up to rounding and the clamp decides it.  The pair lives on four dofs of its own
    (|y|^2 = 1/4, so the pivot's rounding residue, a few ulp of 1/4, is under kMinVal whatever the rounding order), the other rows on
    the remaining twenty: the clamped 2 x 2 block is then decoupled from the rest EXACTLY (its off-block entries are products with
    zeros), and its solution -- entries of the order 1 / kMinVal -- is a short chain of products that a restatement of the operation
    order reproduces to a few ulp.  (Coupled to the other rows, the exactly-cancelling entries a_i1 - l_i0 l_10 would be pure rounding
    noise multiplied by 1 / sqrt(kMinVal): no two roundings of the same order agree on that, on any path.)"""
    assert n >= 3
    rng = np.random.RandomState(77 + n)
    Y = np.zeros((n, 24))
    Y[0, :4] = Y[1, :4] = 0.25
    Y[2:, 4:] = rng.standard_normal((n - 2, 20))
    rhs = rng.uniform(0.2, 1.5, size=n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    A = Y @ Y.T
    assert A[0, 0] == 0.25 and A[0, 1] == 0.25 and A[1, 1] == 0.25 and not A[:2, 2:].any()
    A.setflags(write=False)
    rhs.setflags(write=False)
    return A, rhs


def pack(A):
    n = A.shape[0]
    out = np.zeros(LD)
    for i in range(n):
        out[i * (i + 1) // 2:i * (i + 1) // 2 + i + 1] = A[i, :i + 1]
    return out


def slots(problems):
    """(n, C, rhs) arrays of the two-problem layout from up to two (A, rhs) pairs (None = an empty problem)."""
    n = np.zeros(2, dtype=np.int32)
    C = np.zeros(2 * LD)
    x = np.zeros(64)
    for p, pr in enumerate(problems):
        if pr is None:
            continue
        A, rhs = pr
        n[p] = A.shape[0]
        C[p * LD:(p + 1) * LD] = pack(A)
        x[p * 32:p * 32 + n[p]] = rhs
    return n, C, x


def solve_ext(A, rhs):
    """The solution in extended precision (np.longdouble Cholesky; one step of refinement in the same precision on top)."""
    n = A.shape[0]
    Al = A.astype(np.longdouble)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        L[j, j] = np.sqrt(Al[j, j] - (L[j, :j] * L[j, :j]).sum())
        for i in range(j + 1, n):
            L[i, j] = (Al[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]

    def sub(b):
        y = np.zeros(n, dtype=np.longdouble)
        for i in range(n):
            y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
        x = np.zeros(n, dtype=np.longdouble)
        for i in range(n - 1, -1, -1):
            x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
        return x
    b = rhs.astype(np.longdouble)
    x = sub(b)
    return x + sub(b - Al @ x)


def rel_err(x, x_ext):
    d = np.asarray(x, dtype=np.longdouble) - x_ext
    return float(np.sqrt((d * d).sum()) / np.sqrt((x_ext * x_ext).sum()))


def _fma(a, b, c):
    """a * b + c with one rounding (what the device's contracted multiply-adds compute)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def restate(A, rhs, fused, minval=MINVAL):
    """chol_solve_reg in its own operation order, lane by lane: `fused` = the multiply-subtracts as one rounding (the device build)
    or two (the CPU fibers, compiled without contraction).  1 / sqrt stands for the device's rsqrt (equal to an ulp or two)."""
    n = A.shape[0]
    a = [[float(A[i, k]) for k in range(n)] for i in range(n)]
    r = [float(v) for v in rhs]

    def msub(c, p, q):          # c - p * q
        return _fma(-p, q, c) if fused else c - p * q
    for j in range(n):
        pj = a[j][j]
        pj = minval if pj < minval else pj
        dj = 1.0 / float(np.sqrt(pj))
        l = [a[i][j] * dj for i in range(n)]
        zj = r[j] * dj
        for i in range(n):
            lb = l[i] if i > j else 0.0
            r[i] = zj * dj if i == j else msub(r[i], lb, zj)
            a[i][j] = lb * dj
            if i > j:
                for k in range(j + 1, i + 1):
                    a[i][k] = msub(a[i][k], l[i], l[k])
    for j in range(n - 1, 0, -1):
        for k in range(j):
            r[k] = msub(r[k], a[j][k], r[j])
    return np.array(r)
