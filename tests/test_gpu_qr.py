"""``QR`` on the device (csrc/qr.hip and the panel loop of exec_linalg.py through PlanExecutor): the
one-node plans ``nlinalg.qr`` lowers to (qr_util.op_plan; tests/test_qr_lowering.py holds the linker to
them) on the committed cases, held to the bars derived in tests/qr_util.py.  No front end is imported
here; whole graphs run in tests/test_gpu_qr_function.py.

Every case runs three times from one executor in replay mode — the first call records, the next
two replay — and all outputs of the three calls must have the same bits.
"""
import numpy as np
import pytest
import torch

import qr_util
from qr_util import CASES, DTYPES, NB

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def golden(name, dt):
    if (name, dt) not in _GOLDEN:
        _GOLDEN[name, dt] = dict(np.load(qr_util.case_file(name, dt)))
    return _GOLDEN[name, dt]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def executor(plan):
    from aesara_amd.executor import PlanExecutor
    return PlanExecutor(plan, use_graph=True)


def run3(plan, ins):
    """The outputs of the recording call; both replays must repeat their bits."""
    ex = executor(plan)
    calls = [[o.cpu().numpy() for o in ex(*ins)] for _ in range(3)]
    assert len(ex._graphs) == 1 and not ex._no_replay          # recorded once, replayed twice
    for later in calls[1:]:
        assert len(later) == len(calls[0])
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(later, calls[0]))
    return calls[0]


def check(name, dt, outs, what=""):
    c = CASES[name]
    z = golden(name, dt)
    assert [o.shape for o in outs] == qr_util.out_shapes(c["m"], c["n"], c["mode"]), [o.shape for o in outs]
    assert all(o.dtype == np.dtype(dt) for o in outs)
    assert all(np.all(np.isfinite(o)) for o in outs), (name, dt, what)
    r = qr_util.ratios(name, dt, outs, z)
    print(f"{name} {dt} {what}: " + ", ".join(f"{k} at {v:.3f} of its bar" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (name, dt, what, r)
    if c["mode"] in ("reduced", "complete", "r"):
        R = outs[-1]
        assert not np.any(np.tril(R, -1)), "the zeros below the diagonal of R are exact"


@pytest.mark.parametrize("name,dtype", qr_util.all_cases())
def test_cases(name, dtype):
    outs = run3(qr_util.op_plan(name, dtype), [dev(qr_util.operand(name, dtype))])
    check(name, dtype, outs)
    c = CASES[name]
    if c["kind"] == "triu":
        A = qr_util.operand(name, dtype)
        if c["mode"] == "raw":
            h, tau = outs
            assert not np.any(tau) and np.array_equal(h.T, A)
        else:
            Q, R = outs
            assert np.array_equal(Q, np.eye(c["m"], dtype=dtype)) and np.array_equal(R, A)
    if c["kind"] == "zero_col":
        assert not np.any(outs[1][:, list(qr_util.ZERO_COLS)])
    if name == "empty_cols_complete":
        assert np.array_equal(outs[0], np.eye(3, dtype=dtype))


def _strided_matrix(a):
    """``a`` as a row-strided slice of a larger buffer (the rest holds NaN)."""
    n, m = a.shape
    big = torch.full((n + 2, 2 * m + 3), float("nan"), dtype=dev(a).dtype, device="cuda")
    view = big[1:n + 1, 3:3 + m]
    view.copy_(dev(a))
    return view


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["transposed", "row_slice"])
@pytest.mark.parametrize("name", ["tall_reduced", "wide_raw", "sq_complete"])
def test_operand_layouts(name, layout, dtype):
    A = qr_util.operand(name, dtype)
    x = dev(A.T).t() if layout == "transposed" else _strided_matrix(A)
    assert not x.is_contiguous()
    check(name, dtype, run3(qr_util.op_plan(name, dtype), [x]), layout)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", qr_util.MODES)
def test_a_nan_entry_gives_nan_outputs_and_the_call_returns(mode, dtype):
    outs = run3(qr_util.plan_of(mode, dtype), [dev(qr_util.nan_matrix(dtype))])
    assert [o.shape for o in outs] == qr_util.out_shapes(NB + 6, NB + 2, mode)
    assert all(np.isnan(o).any() for o in outs), [int(np.isnan(o).sum()) for o in outs]


def _range(t):
    return t.data_ptr(), t.data_ptr() + max(t.numel(), 1) * t.element_size()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["reduced", "complete", "raw"])
def test_outputs_alias_nothing_and_survive_the_next_call(mode, dtype):
    name = {"reduced": "tall_reduced", "complete": "tall_complete", "raw": "tall_raw"}[mode]
    ex = executor(qr_util.op_plan(name, dtype))
    A = dev(qr_util.operand(name, dtype))
    kept = []
    for call in range(3):                         # eager / recording, then two replays
        a, b = ex(A)
        (a0, a1), (b0, b1) = _range(a), _range(b)
        assert a1 <= b0 or b1 <= a0, "the two outputs overlap"
        assert all(_range(o)[1] <= _range(A)[0] or _range(A)[1] <= _range(o)[0] for o in (a, b))
        kept.append((a, b, a.clone(), b.clone()))
        # another matrix through the same executor must leave the earlier results alone
        ex(dev(qr_util.operand(name, dtype)[::-1].copy()))
        for x, y, x0, y0 in kept:
            assert torch.equal(x, x0) and torch.equal(y, y0)
    check(name, dtype, [kept[-1][0].cpu().numpy(), kept[-1][1].cpu().numpy()], "kept")
