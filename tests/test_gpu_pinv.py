"""MatrixPinv on the device (csrc/svd.hip and the loops of exec_svd.py through PlanExecutor): hand-built
one-node plans against ``np.linalg.pinv`` of the same values in float64.

The bar is derived, not tuned.  The computed factors are exact for ``A + E`` with ``||E||_F <= ((9 r + 1)
+ max(m, n)) eps ||A||_F``: ``r = 30 (k_pad - 1)`` stages of disjoint rotations at the sweep cap (the cap,
not the call's own count: no bar depends on the code under test; ``k_pad`` is ``min(m, n)`` rounded up to
even, to a multiple of 64 above 64), 9 >= sqrt(2) * 6 from Higham's bound for one computed rotation
(Lemma 19.8), 1 for the stopping threshold, and ``max(m, n) eps ||A||_F`` for the QR stage and the closing
product.  ``hermitian=True`` rotates from both sides: ``r = 2 * 30 (n_pad - 1)``, as in
tests/test_gpu_eigvalsh.py.  Wedin's theorem for equal rank carries it to the result: ``||P^ - P||_F <=
sqrt(2) ||A+||_2^2 ||E||_F``, with ``||A+||_2`` from the float64 reference's singular values.  NumPy's own
float32 ``pinv`` stays below 1.1e-3 of this bar on these shapes (the last test, on the CPU).

The graded case (kappa = 1e8, float64) is the one that tells the scaled rotation threshold from a
norm-wise one: its bar is about 1.6e-3 ||P||, and a solver that loses ``eps kappa^2`` misses it by orders
of magnitude.  Up to 64 columns a call records and replays; above it the executor ends up eager; three
calls repeat their bits."""
import numpy as np
import pytest
import torch

from aesara_amd.plan import Node, Plan
from test_gpu_eigvalsh import DTYPES, GARBAGE, dev

SHAPES = [(1, 1), (2, 3), (3, 2), (33, 31), (64, 64), (65, 64), (200, 40), (40, 200), (65, 65), (130, 130),
          (70, 257)]
DEFICIENT = [(6, 4), (64, 64), (130, 70)]


def plan_of(dtype, hermitian=False):
    plan = Plan(f"pinv_{dtype}_{int(hermitian)}", {}, [], [], [])
    a, out = plan.new_var(dtype, [None, None], "a"), plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = [a], [out]
    plan.nodes.append(Node("MatrixPinv", [a], [out], {"hermitian": hermitian}))
    return plan


def k_pad(k):
    return k + k % 2 if k <= 64 else -(-k // 64) * 64


def bar(A, dtype, hermitian=False):
    m, n = A.shape
    r = (2 if hermitian else 1) * 30 * (k_pad(min(m, n)) - 1)
    s = np.linalg.svd(A, compute_uv=False)
    s = s[s > 1e-15 * s.max(initial=0.0)]
    if not s.size:
        return 0.0
    return np.sqrt(2) / s.min() ** 2 * (9 * r + 1 + max(m, n)) * float(np.finfo(dtype).eps) * np.linalg.norm(A)


def graded(m, n, dtype, kappa=10.0, signs=False):
    """``U diag(geomspace(1, 1 / kappa)) V^T`` with entries exact in ``dtype``, as float64; with ``signs``
    the symmetric indefinite ``Q diag(+-s) Q^T``."""
    rng, k = np.random.default_rng(1000 * m + n), min(m, n)
    U = np.linalg.qr(rng.standard_normal((m, k)))[0]
    s = np.geomspace(1.0, 1.0 / kappa, k)
    if signs:
        M = (U * (s * np.where(np.arange(k) % 2, -1.0, 1.0))) @ U.T
        M = ((M + M.T) / 2).astype(dtype).astype("float64")
        return np.tril(M) + np.tril(M, -1).T
    V = np.linalg.qr(rng.standard_normal((n, k)))[0]
    return ((U * s) @ V.T).astype(dtype).astype("float64")


def run3(plan, a, k):
    """The result of the first call; the next two must repeat its bits — replayed up to 64 columns, eager above."""
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan, use_graph=True)
    outs = [ex(a)[0].cpu().numpy() for _ in range(3)]
    assert (len(ex._graphs) == 1 and not ex._no_replay) if k <= 64 else (ex._no_replay and not ex._graphs)
    assert all(np.array_equal(o, outs[0], equal_nan=True) for o in outs[1:])
    return outs[0]


def check(got, A, dtype, what, hermitian=False):
    want = np.linalg.pinv(A, hermitian=hermitian)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    err, cap = np.linalg.norm(got.astype("float64") - want), bar(A, dtype, hermitian)
    print(f"{what}: error {err:.3e}, {err / cap if cap else 0.0:.2e} of the bar {cap:.3e}")
    assert err <= cap, (what, err, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_full_rank(shape, dtype):
    A = graded(*shape, dtype)
    check(run3(plan_of(dtype), dev(A.astype(dtype)), min(shape)), A, dtype, f"{shape} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 130])
def test_graded_singular_values(n):
    A = graded(n, n, "float64", kappa=1e8)
    check(run3(plan_of("float64"), dev(A), n), A, "float64", f"graded n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", DEFICIENT)
@pytest.mark.parametrize("kind", ["zero_lines", "zero"])
def test_exact_rank_deficiency(kind, shape, dtype):
    """Two all-zero columns and one all-zero row, and the all-zero matrix: what must be zero is exactly zero."""
    A = graded(*shape, dtype)
    A[:, [1, shape[1] - 1]] = 0.0
    A[2, :] = 0.0
    if kind == "zero":
        A[:] = 0.0
    got = run3(plan_of(dtype), dev(A.astype(dtype)), min(shape))
    check(got, A, dtype, f"{kind} {shape} {dtype}")
    assert not np.any(got[[1, shape[1] - 1], :]) and not np.any(got[:, 2])
    assert kind != "zero" or not np.any(got)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [6, 64, 130])
def test_hermitian(n, dtype):
    """Eigenvalues of both signs; the strict upper triangle holds garbage and must not be read."""
    M = graded(n, n, dtype, signs=True)
    a = np.where(np.triu(np.ones((n, n), bool), 1), GARBAGE[dtype], M).astype(dtype)
    check(run3(plan_of(dtype, True), dev(a), n), M, dtype, f"hermitian n={n} {dtype}", True)


@pytest.mark.gpu
def test_strided_operand():
    A = graded(33, 31, "float32")
    big = torch.full((100, 70), 1e30, dtype=torch.float32, device="cuda")
    a = big.t()[1:67:2, 2:95:3]
    a.copy_(dev(A.astype("float32")))
    assert tuple(a.shape) == (33, 31) and not a.is_contiguous()
    check(run3(plan_of("float32"), a, 31), A, "float32", "strided (33, 31) float32")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_is_raised_in_the_call_that_met_it(dtype):
    from aesara_amd.executor import PlanExecutor
    good = graded(3, 2, dtype).astype(dtype)
    nan = good.copy()
    nan[2, 0] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match="SVD did not converge"):
        np.linalg.pinv(nan)
    with pytest.raises(np.linalg.LinAlgError, match="SVD did not converge") as ei:       # in the recording call
        PlanExecutor(plan_of(dtype), use_graph=True)(dev(nan))
    assert "[HIP step" in str(ei.value)
    ex = PlanExecutor(plan_of(dtype), use_graph=True)
    a = dev(good)
    first = ex(a)[0].cpu().numpy()
    a.copy_(dev(nan))
    with pytest.raises(np.linalg.LinAlgError, match="SVD did not converge"):             # in a replay
        ex(a)
    a.copy_(dev(good))
    assert np.array_equal(ex(a)[0].cpu().numpy(), first) and len(ex._graphs) == 1
    big = graded(70, 130, dtype).astype(dtype)                                           # eager, above 64 columns
    big[50, 100] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match="SVD did not converge"):
        PlanExecutor(plan_of(dtype), use_graph=True)(dev(big))


@pytest.mark.parametrize("kappa", [10.0, 100.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_numpy_float32_stays_far_inside_the_same_bar(shape, kappa):
    """On the CPU: the float32 reference alone is at most 1.1e-3 of the bar the device is held to."""
    A = graded(*shape, "float32", kappa)
    err = np.linalg.norm(np.linalg.pinv(A.astype("float32")).astype("float64") - np.linalg.pinv(A))
    assert err <= 1.1e-3 * bar(A, "float32")
