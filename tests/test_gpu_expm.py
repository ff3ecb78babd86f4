"""Expm and ExpmGrad on the device (csrc/expm.hip and exec_expm.py through PlanExecutor): hand-built one-node
plans against ``scipy.linalg.expm`` and, for the gradient, ``scipy.linalg.expm_frechet(A.T, G)``, in float64.

The sizes are the edges of the kernels: the padding of the matrix instructions (15, 16, 17), both limits of
the one-launch path and the first size past each (48 | 49 in float64, 64 | 65 in float32; the gradient works
on twice its operand: 24 | 25, 32 | 33), and a blocked LU across a 64-wide panel (130, the gradient's 70).
Gaussian operands with entries scaled by ``c / sqrt(n)`` span ``||A||_1`` from 0.01 to about 400: every Pade
degree and several squarings.

The measure is the relative Frobenius error.  The yardstick is SciPy's own error on the same operand in
float32 (``expm`` of the float32 operand against float64; for the gradient the top-right block of ``expm`` of
the float32 block matrix ``[[A^T, G], [0, A^T]]``, as ``expm_frechet`` computes in float64 only), times
``eps64 / eps32`` for float64 — the error of scaling and squaring is linear in the unit roundoff — and never
below ``n eps`` of the dtype, for operands where SciPy happens to be exact.  The bar is the yardstick times
``MARGIN``: SciPy's 2009 algorithm sometimes squares less than the 2005 thresholds used here, and a squaring
can double the rounding error.

MARGIN = 32: the smallest power of two that is at least twice the worst ratio of error to yardstick seen on the
device.  On an MI355X the worst ratio over every case of this file and of tests/test_gpu_expm_function.py is
11.96 (``expm``, n = 2, c = 40, float64: ``||A||_1`` = 43, four squarings, error 7.9e-14); the next are 3.13
(gradient, n = 1, c = 40, float64) and 3.12 (the nilpotent block, n = 66, float64), and no float32 case is
above 1.66.

Up to the limit a call records and replays, above it the executor ends up eager; the second call must
repeat the bits of the first."""
import functools

import numpy as np
import pytest
import scipy.linalg

from aesara_amd.plan import Node, Plan
from test_gpu_eigvalsh import DTYPES, dev

MARGIN = 32                   # twice the worst measured ratio (11.96), as a power of two: see above
SCALES = (0.01, 0.2, 0.9, 2, 5, 40)
FORWARD = [(n, c) for n in (1, 2, 15, 16, 17, 48, 49, 64, 65, 130) for c in (SCALES if n in (17, 65) else (0.9, 40))]
GRADIENT = [(n, c) for n in (1, 5, 24, 25, 32, 33, 70) for c in (0.9, 40)]
TILE_ROWS = {"float32": 64, "float64": 48}


def plan_of(dtype, grad=False):
    plan = Plan(f"expm_{dtype}_{int(grad)}", {}, [], [], [])
    ins = [plan.new_var(dtype, [None, None], name) for name in (("a", "g") if grad else ("a",))]
    out = plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = list(ins), [out]
    plan.nodes.append(Node("ExpmGrad" if grad else "Expm", list(ins), [out], {}))
    return plan


def gaussian(n, c, seed=0):
    """Entries ``c / sqrt(n)`` times a standard normal, exact in float32, as float64."""
    M = np.random.default_rng(1000 * n + seed).standard_normal((n, n)) * (c / np.sqrt(n))
    return M.astype("float32").astype("float64")


def rel(got, want):
    return np.linalg.norm(got.astype("float64") - want) / np.linalg.norm(want)


def block(A, G):
    n = A.shape[0]
    return np.block([[A.T, G], [np.zeros((n, n)), A.T]])


def yardstick(err32, n, dtype):
    eps = float(np.finfo(dtype).eps)
    return max(err32 * (eps / float(np.finfo("float32").eps)), n * eps)


def reference(A, G=None):
    """(the float64 result, SciPy's relative error on the same operand in float32): computed once a case."""
    n = A.shape[0]
    if G is None:
        want = scipy.linalg.expm(A)
        return want, rel(scipy.linalg.expm(A.astype("float32")), want)
    want = scipy.linalg.expm_frechet(A.T, G, compute_expm=False)
    return want, rel(scipy.linalg.expm(block(A, G).astype("float32"))[:n, n:], want)


@functools.lru_cache(maxsize=None)
def gaussian_case(n, c, grad):
    A = gaussian(n, c)
    G = gaussian(n, 1.0, seed=1) if grad else None
    return (A, G) + reference(A, G)


def run2(dtype, A, G=None, a=None):
    """The result of the first call; the second must repeat its bits — replayed on the one-launch path,
    eager above it.  ``a``: the device operand, where it is not the contiguous copy of ``A``."""
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan_of(dtype, G is not None), use_graph=True)
    ins = [dev(A.astype(dtype)) if a is None else a] + ([] if G is None else [dev(G.astype(dtype))])
    outs = [ex(*ins)[0].cpu().numpy() for _ in range(2)]
    rows = A.shape[0] * (1 if G is None else 2)
    assert (len(ex._graphs) == 1 and not ex._no_replay) if rows <= TILE_ROWS[dtype] else ex._no_replay
    assert np.array_equal(outs[0], outs[1], equal_nan=True)
    assert outs[0].dtype == np.dtype(dtype) and outs[0].shape == A.shape
    return outs[0]


def check(got, want, err32, dtype, what):
    err, cap = rel(got, want), yardstick(err32, want.shape[0], dtype)
    print(f"{what} {dtype}: error {err:.3e}, {err / cap:.2f} of the yardstick {cap:.3e}")
    assert err <= MARGIN * cap, (what, err, cap)
    return MARGIN * cap


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,c", FORWARD)
def test_expm(n, c, dtype):
    A, _, want, err32 = gaussian_case(n, c, False)
    check(run2(dtype, A), want, err32, dtype, f"expm n={n} c={c}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,c", GRADIENT)
def test_expm_grad(n, c, dtype):
    A, G, want, err32 = gaussian_case(n, c, True)
    check(run2(dtype, A, G), want, err32, dtype, f"grad n={n} c={c}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [20, 70])
def test_a_rate_matrix_gives_rows_that_sum_to_one(n, dtype):
    """Non-negative off-diagonal entries, rows summing to zero: a stochastic matrix, within the same bar."""
    Q = np.random.default_rng(n).uniform(0.0, 1.0, (n, n)).astype("float32").astype("float64")
    np.fill_diagonal(Q, 0.0)
    np.fill_diagonal(Q, -Q.sum(1))
    got = run2(dtype, Q)
    cap = check(got, *reference(Q), dtype, f"rate n={n}")
    assert np.linalg.norm(got.astype("float64").sum(1) - 1.0) / np.sqrt(n) <= cap


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [8, 66])
def test_a_nilpotent_jordan_block(n, dtype):
    """3 (the upper shift): defective — the eig / inv(V) route of the reference's gradient divides by a
    singular V, the block form does not care."""
    A = 3.0 * np.eye(n, k=1)
    check(run2(dtype, A), *reference(A), dtype, f"nilpotent n={n}")
    if n == 8:
        G = gaussian(n, 1.0, seed=2)
        check(run2(dtype, A, G), *reference(A, G), dtype, f"nilpotent grad n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 65])
def test_the_zero_matrix_gives_exactly_the_identity(n, dtype):
    assert np.array_equal(run2(dtype, np.zeros((n, n))), np.eye(n, dtype=dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 65])
def test_a_transposed_view(n):
    A, _, want, err32 = gaussian_case(n, 2, False)
    a = dev(A.T.astype("float32").copy()).t()
    assert not a.is_contiguous()
    check(run2("float32", A, a=a), want, err32, "float32", f"transposed view n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [5, 65])
def test_a_nan_gives_nans_and_does_not_raise(n, dtype):
    A = gaussian(n, 0.9)
    A[0, 0] = np.nan
    assert np.isnan(scipy.linalg.expm(A)).all()
    assert np.isnan(run2(dtype, A)).all()
