"""SolveTriangular / CholeskySolve / Solve / MatrixInverse / Det on the device (csrc/linalg.hip and the
block loops of exec_linalg.py through PlanExecutor): the one-node plans the Ops lower to
(linalg_util.op_plan; tests/test_linalg_lowering.py holds the linker to them) on the committed cases,
held to the bars derived in tests/linalg_util.py.  No front end is imported here; whole graphs run in
tests/test_gpu_linalg_function.py.

Every case runs three times from one executor in replay mode — the first call records, the next
two replay — and the three results must have the same bits.  Errors are exceptions, never device
faults, and are tried in the recording call and in a replay.
"""
import numpy as np
import pytest
import torch

import linalg_util
from linalg_util import CASES, DTYPES, NB

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def golden(name, dt):
    if (name, dt) not in _GOLDEN:
        _GOLDEN[name, dt] = dict(np.load(linalg_util.case_file(name, dt)))
    return _GOLDEN[name, dt]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def executor(plan):
    from aesara_amd.executor import PlanExecutor
    return PlanExecutor(plan, use_graph=True)


def run3(plan, ins):
    """The result of the recording call; both replays must repeat its bits."""
    ex = executor(plan)
    outs = [ex(*ins)[0].cpu().numpy() for _ in range(3)]
    assert len(ex._graphs) == 1 and not ex._no_replay          # recorded once, replayed twice
    assert all(np.array_equal(o, outs[0], equal_nan=True) for o in outs[1:])
    return outs[0]


def check(name, dt, got, what=""):
    z = golden(name, dt)
    assert got.dtype == np.dtype(dt) and got.shape == linalg_util.out_shape(name), (got.dtype, got.shape)
    r = linalg_util.ratios(name, dt, got, z)
    print(f"{name} {dt} {what}: " + ", ".join(f"{k} at {v:.3f} of its bar" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (name, dt, what, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(name, dtype):
    ins = [dev(a) for a in linalg_util.operands(name, dtype)]
    check(name, dtype, run3(linalg_util.op_plan(name, dtype), ins))


def _strided_matrix(a):
    """``a`` as a row-strided slice of a larger buffer (the rest holds NaN)."""
    n, m = a.shape
    big = torch.full((n + 2, 2 * m + 3), float("nan"), dtype=dev(a).dtype, device="cuda")
    view = big[1:n + 1, 3:3 + m]
    view.copy_(dev(a))
    return view


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["transposed", "row_slice", "b_strided"])
@pytest.mark.parametrize("name", [f"tri_n{n}_l{lo}t{t}_{rhs}" for n in (NB + 1, 2 * NB + 2) for lo in (0, 1)
                                  for t in (0, 1) for rhs in ("vec", NB + 6)])
def test_solve_triangular_operand_layouts(name, layout, dtype):
    A, b = linalg_util.operands(name, dtype)
    if layout == "transposed":
        ins = [dev(A.T).t(), dev(b)]
    elif layout == "row_slice":
        ins = [_strided_matrix(A), dev(b)]
    else:
        wide = torch.zeros((b.shape[0],) + (2,) * 1 + tuple(b.shape[1:]), dtype=dev(b).dtype, device="cuda")
        bv = wide[:, 1]                      # every other row of the buffer
        bv.copy_(dev(b))
        ins = [dev(A), bv]
    assert layout == "b_strided" or not ins[0].is_contiguous()
    assert layout != "b_strided" or not ins[1].is_contiguous()
    check(name, dtype, run3(linalg_util.op_plan(name, dtype), ins), layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["solve_far_pivot", "solve_n130_sym_l0", "inv_far_pivot", "det_far_pivot"])
def test_lu_ops_read_their_matrix_through_its_strides(name, dtype):
    ops = linalg_util.operands(name, dtype)
    sym = "_sym_" in name
    # (a symmetric case handed over transposed names the OTHER triangle: not the same system)
    ins = [_strided_matrix(ops[0]) if sym else dev(ops[0].T).t()] + [dev(b) for b in ops[1:]]
    check(name, dtype, run3(linalg_util.op_plan(name, dtype), ins), "strided")


# ------------------------------------------------------------------ errors ------------
def small_plan(op, dtype, rhs="vec", **params):
    name = f"_err_{op}"
    CASES[name] = dict(op=op, n=2, rhs=rhs, kind="gauss", params=params)
    try:
        return linalg_util.op_plan(name, dtype)
    finally:
        del CASES[name]


SINGULAR = np.array([[1.0, 2.0], [2.0, 4.0]])
REGULAR = np.array([[1.0, 2.0], [4.0, 4.0]])       # (its LU is exact: pivot 4, multiplier 1/4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_singular_matrix_raises_from_solve_and_inverse_and_gives_zero_from_det(dtype):
    b = dev(np.array([1.0, 1.0], dtype))
    for op, ins, msg in (("solve", lambda A: [A, b], "Matrix is singular"), ("inv", lambda A: [A], "Singular matrix")):
        params = dict(assume_a="gen", lower=False, check_finite=True) if op == "solve" else {}
        plan = small_plan(op, dtype, "vec" if op == "solve" else None, **params)
        with pytest.raises(np.linalg.LinAlgError, match=msg) as ei:        # in the first (eager) call
            executor(plan)(*ins(dev(SINGULAR.astype(dtype))))
        assert "[HIP step" in str(ei.value)
        ex = executor(plan)
        A = dev(REGULAR.astype(dtype))
        first = ex(*ins(A))[0].cpu().numpy()
        A.copy_(dev(SINGULAR.astype(dtype)))
        with pytest.raises(np.linalg.LinAlgError, match=msg):               # in a replay
            ex(*ins(A))
        A.copy_(dev(REGULAR.astype(dtype)))
        assert np.array_equal(ex(*ins(A))[0].cpu().numpy(), first)         # the info word was cleared
        assert len(ex._graphs) == 1
    ex = executor(small_plan("det", dtype, None))
    A = dev(REGULAR.astype(dtype))
    assert ex(A)[0].cpu().numpy() == np.asarray(-4.0, dtype)
    A.copy_(dev(SINGULAR.astype(dtype)))
    d = ex(A)[0].cpu().numpy()
    assert d.shape == () and d == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("rhs", ["vec", 3])
def test_a_zero_on_a_triangular_diagonal_raises_with_its_index(lower, rhs, dtype):
    n = NB + 6
    name = f"tri_n{NB + 1}_l{int(lower)}t0_vec"
    T = linalg_util.triangular(n, lower, 7, dtype).astype(dtype)
    b = np.ones((n,) if rhs == "vec" else (n, rhs), dtype)
    CASES["_err_tri"] = dict(CASES[name], n=n, rhs=rhs)
    try:
        plan = linalg_util.op_plan("_err_tri", dtype)
    finally:
        del CASES["_err_tri"]
    ex = executor(plan)
    Td, bd = dev(T), dev(b)
    ex(Td, bd)
    bad = T.copy()
    bad[NB + 2, NB + 2] = 0.0          # two zeros: the first one (LAPACK's info) is reported
    bad[3, 3] = 0.0
    Td.copy_(dev(bad))
    with pytest.raises(np.linalg.LinAlgError, match=r"resolution failed at diagonal 3\b"):
        ex(Td, bd)
    bad[3, 3] = 1.0
    Td.copy_(dev(bad))
    with pytest.raises(np.linalg.LinAlgError, match=rf"resolution failed at diagonal {NB + 2}\b"):
        ex(Td, bd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["tri", "chol", "solve"])
@pytest.mark.parametrize("where", ["A", "b"])
def test_non_finite_operands_under_check_finite(op, where, dtype):
    params = {"tri": dict(lower=True, trans=0, unit_diagonal=False), "chol": dict(lower=True),
              "solve": dict(assume_a="gen", lower=False)}[op]
    A = np.array([[2.0, 0.0], [1.0, 3.0]], dtype)
    b = np.array([1.0, 2.0], dtype)
    poison = np.nan if where == "A" else np.inf     # (an inf in A can cancel into a zero pivot: NaN there)
    for check_finite in (True, False):
        ex = executor(small_plan(op, dtype, "vec", check_finite=check_finite, **params))
        Ad, bd = dev(A), dev(b)
        good = ex(Ad, bd)[0].cpu().numpy()
        assert np.all(np.isfinite(good))
        (Ad if where == "A" else bd)[1 if where == "b" else (1, 0)] = poison
        if check_finite:
            with pytest.raises(ValueError, match="array must not contain infs or NaNs"):    # in a replay
                ex(Ad, bd)
            with pytest.raises(ValueError, match="array must not contain infs or NaNs"):    # in a first call
                executor(small_plan(op, dtype, "vec", check_finite=True, **params))(Ad, bd)
        else:
            got = ex(Ad, bd)[0].cpu().numpy()
            assert not np.all(np.isfinite(got))
