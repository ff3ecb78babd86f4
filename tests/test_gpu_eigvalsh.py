"""Eigvalsh on the device (csrc/eig.hip and the loops of exec_eig.py through PlanExecutor): hand-built
one-node plans against NumPy float64.

The bar is derived, not tuned.  By Weyl, ``|w_i - w_i^| <= (9 r + 1) eps ||A||_F``: ``r = 2 * 30 *
(n_pad - 1)`` stages of disjoint rotations at the sweep cap (the cap, not the call's own count: no
bar depends on the code under test), 9 >= sqrt(2) * 6 from Higham's bound for one computed rotation
(Lemma 19.8), and 1 for the stopping threshold; times kappa(B) for the generalised problem.  Up to 64
rows a call records and replays; above it the executor ends up eager; three calls repeat their bits."""
import numpy as np
import pytest
import torch

from aesara_amd.plan import Node, Plan

DTYPES = ("float32", "float64")
SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 130, 257)
GARBAGE = {"float32": 1e30, "float64": 1e300}      # finite, in the triangle that must not be read
KAPPA_B = 10.0


def plan_of(dtype, lower, with_b=False):
    plan = Plan(f"eigvalsh_{dtype}_{int(lower)}_{int(with_b)}", {}, [], [], [])
    ins = [plan.new_var(dtype, [None, None], name) for name in (("a", "b") if with_b else ("a",))]
    out = plan.new_var(dtype, [None])
    plan.inputs, plan.outputs = list(ins), [out]
    plan.nodes.append(Node("Eigvalsh", list(ins), [out], {"lower": lower}))
    return plan


def n_pad(n):
    return n + n % 2 if n <= 64 else -(-n // 64) * 64


def bar(M, dtype, kappa=1.0):
    r = 2 * 30 * (n_pad(M.shape[0]) - 1)
    return kappa * (9 * r + 1) * float(np.finfo(dtype).eps) * np.linalg.norm(M)


def symmetric(kind, n, dtype, seed=0):
    """A symmetric matrix whose entries are exact in ``dtype``, as float64."""
    rng = np.random.default_rng(1000 * n + seed)
    if kind == "rot45":            # [[0, 1], [1, 0]] inside a larger matrix: exact 45 degrees, pairs of +-s
        M = np.zeros((n, n))
        for i in range(0, n - 1, 2):
            M[i, i + 1] = M[i + 1, i] = 1.0 + i
    elif kind == "diag_desc":      # no rotations, and still to be sorted
        M = np.diag(np.arange(n, 0, -1.0))
    elif kind == "two_i":
        M = 2.0 * np.eye(n)
    else:
        G = rng.standard_normal((n, n))
        M = (G + G.T) / 2
        M *= {"tiny": {"float32": 1e-15, "float64": 1e-30}, "huge": {"float32": 1e15, "float64": 1e30}}.get(
            kind, {}).get(dtype, 1.0)
    M = M.astype(dtype).astype("float64")
    return np.tril(M) + np.tril(M, -1).T


def spd(n, dtype):
    """B = Q diag(1 ... 10) Q^T: kappa(B) = 10, smallest eigenvalue 1."""
    Q = np.linalg.qr(np.random.default_rng(7 * n + 1).standard_normal((n, n)))[0]
    B = (Q * np.linspace(1.0, 10.0, n)) @ Q.T
    B = ((B + B.T) / 2).astype(dtype).astype("float64")
    return np.tril(B) + np.tril(B, -1).T


def one_triangle(M, lower, dtype):
    """``M`` in ``dtype`` with garbage in the triangle ``lower`` does not name."""
    other = np.triu(np.ones(M.shape, bool), 1) if lower else np.tril(np.ones(M.shape, bool), -1)
    return np.where(other, GARBAGE[dtype], M).astype(dtype)


def reference(M, B=None):
    if B is None:
        return np.linalg.eigvalsh(M)
    L = np.linalg.cholesky(B)
    C = np.linalg.solve(L, np.linalg.solve(L, M).T).T
    return np.linalg.eigh((C + C.T) / 2)[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run3(plan, ins, n):
    """The result of the first call; the next two must repeat its bits — replayed up to 64 rows, eager above."""
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan, use_graph=True)
    outs = [ex(*ins)[0].cpu().numpy() for _ in range(3)]
    assert (len(ex._graphs) == 1 and not ex._no_replay) if n <= 64 else (ex._no_replay and not ex._graphs)
    assert all(np.array_equal(o, outs[0], equal_nan=True) for o in outs[1:])
    return outs[0]


def check(got, M, dtype, what, B=None):
    want = reference(M, B)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    err, cap = np.max(np.abs(got.astype("float64") - want), initial=0.0), bar(M, dtype, KAPPA_B if B is not None else 1.0)
    print(f"{what}: error {err:.3e}, {err / cap if cap else 0.0:.2e} of the bar {cap:.3e}")
    assert np.all(np.diff(got) >= 0) and err <= cap, (what, err, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_random_symmetric(n, lower, dtype):
    M = symmetric("gauss", n, dtype)
    got = run3(plan_of(dtype, lower), [dev(one_triangle(M, lower, dtype))], n)
    check(got, M, dtype, f"gauss n={n} lower={lower} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [6, 64, 130])
@pytest.mark.parametrize("kind", ["rot45", "diag_desc", "two_i", "tiny", "huge"])
def test_special_matrices(kind, n, dtype):
    M = symmetric(kind, n, dtype)
    got = run3(plan_of(dtype, True), [dev(one_triangle(M, True, dtype))], n)
    check(got, M, dtype, f"{kind} n={n} {dtype}")
    if kind in ("diag_desc", "two_i"):
        assert np.array_equal(got, np.sort(np.diag(M)).astype(dtype))       # no rotation: exact


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [33, 65])
@pytest.mark.parametrize("layout", ["transposed", "row_strided"])
def test_operand_layouts(layout, n, dtype):
    M = symmetric("gauss", n, dtype, seed=3)
    if layout == "transposed":          # the lower triangle of the view is the upper one of the buffer
        a = dev(one_triangle(M, False, dtype)).t()
    else:
        big = torch.full((n + 2, 2 * n + 3), GARBAGE[dtype], dtype=getattr(torch, dtype), device="cuda")
        a = big[1:n + 1, 3:3 + n]
        a.copy_(dev(one_triangle(M, True, dtype)))
    assert not a.is_contiguous()
    check(run3(plan_of(dtype, True), [a], n), M, dtype, f"{layout} n={n} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("n", [3, 64, 65, 130])
def test_generalised(n, lower, dtype):
    M, B = symmetric("gauss", n, dtype, seed=5), spd(n, dtype)
    ins = [dev(one_triangle(M, lower, dtype)), dev(one_triangle(B, lower, dtype))]
    check(run3(plan_of(dtype, lower, True), ins, n), M, dtype, f"generalised n={n} lower={lower} {dtype}", B)


@pytest.mark.parametrize("n", SIZES)
def test_numpy_float32_stays_inside_the_same_bar(n):
    """On the CPU: the float32 reference alone is inside the bar the device is held to."""
    M = symmetric("gauss", n, "float32")
    err = np.max(np.abs(np.linalg.eigvalsh(M.astype("float32")).astype("float64") - reference(M)))
    assert err <= bar(M, "float32")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_are_raised_in_the_call_that_met_them(dtype):
    from aesara_amd.executor import PlanExecutor
    good, eye = symmetric("gauss", 3, dtype), np.eye(3)
    nan = good.copy()
    nan[2, 0] = np.nan
    neg = eye.copy()
    neg[0, 0] = -1.0
    minor = r"The leading minor of order {} of B is not positive definite"
    for bad_a, bad_b, exc, msg in ((nan, eye, ValueError, "array must not contain infs or NaNs"),
                                   (good, neg, np.linalg.LinAlgError, minor.format(1))):
        plan = plan_of(dtype, True, True)
        with pytest.raises(exc, match=msg) as ei:                           # in the recording call
            PlanExecutor(plan, use_graph=True)(dev(bad_a.astype(dtype)), dev(bad_b.astype(dtype)))
        assert "[HIP step" in str(ei.value)
        ex = PlanExecutor(plan, use_graph=True)
        a, b = dev(good.astype(dtype)), dev(eye.astype(dtype))
        first = ex(a, b)[0].cpu().numpy()
        a.copy_(dev(bad_a.astype(dtype)))
        b.copy_(dev(bad_b.astype(dtype)))
        with pytest.raises(exc, match=msg):                                 # in a replay
            ex(a, b)
        a.copy_(dev(good.astype(dtype)))
        b.copy_(dev(eye.astype(dtype)))
        assert np.array_equal(ex(a, b)[0].cpu().numpy(), first) and len(ex._graphs) == 1
    # above 64 rows: a NaN in a, and a negative pivot in the second diagonal block of b
    M, B = symmetric("gauss", 130, dtype), np.eye(130)
    nan = M.copy()
    nan[100, 7] = np.nan
    with pytest.raises(ValueError, match="array must not contain infs or NaNs"):
        PlanExecutor(plan_of(dtype, True), use_graph=True)(dev(nan.astype(dtype)))
    B[69, 69] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match=minor.format(70)):
        PlanExecutor(plan_of(dtype, True, True), use_graph=True)(dev(M.astype(dtype)), dev(B.astype(dtype)))
