"""RFFT / IRFFT on the device (csrc/fft.hip through PlanExecutor), against NumPy evaluated at higher
precision on the same inputs (op-level plans, any shape) and against the reference's stored outputs
(graph-level cases of tests/golden/fft).  No front end is imported here.

Accuracy bar (tests/fft_util.py): relative L2 error of a whole output <= 8.5 * eps(dtype) * L, L the
sum over the transformed axes of log2 of the power-of-two length actually transformed (Bluestein:
3 * log2 m) — float32 against a float64 evaluation, float64 against a longdouble one; float64
graph-level cases against the reference's own float64 output at twice the cap (the reference
carries the same bound).
"""
import numpy as np
import pytest

import fft_util
from fft_util import cap, rel_l2

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in fft_util.load_fft_cases()}
GRAPH_CASES = sorted(n for n, c in CASES.items() if c["kind"] == "graph")
OPS = ("rfft", "irfft")
DTYPES = ("float32", "float64")
POW2 = [1, 2, 4, 8, 16, 32, 64, 128, 1024, 4096]
BLUESTEIN = [3, 5, 6, 7, 10, 12, 17, 100, 1000, 2047, 2048]

_EXECUTORS = {}


def executor(op, dtype, ndim, use_graph=False):
    """One executor per op-level plan (``ndim``: of the real array)."""
    from aesara_amd.executor import PlanExecutor
    key = (op, dtype, ndim, use_graph)
    if key not in _EXECUTORS:
        _EXECUTORS[key] = PlanExecutor(fft_util.case_plan(CASES[f"op_{op}_{dtype}_{ndim}d"]),
                                       use_graph=use_graph)
    return _EXECUTORS[key]


def spectrum_shape(shape):
    return tuple(shape[:-1]) + (shape[-1] // 2 + 1, 2)


def make_operand(op, dtype, shape, seed=0):
    """Random operand whose transform has the real shape ``shape``: the real array itself, or a
    spectrum (re, im) with NON-ZERO imaginary parts in the DC and Nyquist bins."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape if op == "rfft" else spectrum_shape(shape)).astype(dtype)


def exact(op, a, s):
    """NumPy at the next higher precision on the same values."""
    a = np.asarray(a)
    hi = np.float64 if a.dtype == np.float32 else np.longdouble
    axes = tuple(range(1, 1 + len(s)))
    if op == "rfft":
        A = np.fft.rfftn(a.astype(hi), s=tuple(s), axes=axes)
        assert A.real.dtype == hi
        return np.stack([A.real, A.imag], axis=-1)
    z = a[..., 0].astype(hi) + 1j * a[..., 1].astype(hi)
    out = np.fft.irfftn(z, s=tuple(s), axes=axes) * hi(np.prod(s))
    assert out.dtype == hi
    return out


def check(op, dtype, a, s, host=None, use_graph=False, what=""):
    """Run the op-level plan on ``a`` (ndarray or device tensor; ``host``: its values) and hold the
    result against the cap."""
    host = np.asarray(a) if host is None else host
    ndim = host.ndim - (1 if op == "irfft" else 0)
    ex = executor(op, dtype, ndim, use_graph)
    (got,) = ex(a, np.asarray(s, dtype="int64"))
    L = sum(fft_util.axis_cost(int(n)) for n in s)          # one pass per transformed axis
    got = got.cpu().numpy()
    want = exact(op, host, s)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    err, bound = rel_l2(got, want), cap(dtype, L)
    print(f"{op} {dtype} {what} shape={host.shape} s={list(s)} L={L}: rel L2 {err:.3e} (cap {bound:.3e})")
    assert err <= bound, (op, dtype, host.shape, list(s), err, bound)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_last_axis_lengths(op, dtype):
    """Every schedule of the row kernel: single radix-4, radix-4 + radix-2, several rows per
    workgroup, one row per workgroup, 1 / 2 / 4 butterflies per thread, both limits; Bluestein
    from m = 8 to the limit; odd and even inverse lengths.  Batches 1 and 3."""
    for n in POW2 + BLUESTEIN:
        for batch in (1, 3):
            check(op, dtype, make_operand(op, dtype, (batch, n), seed=n + batch), [n])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_more_rows_than_a_grid_dimension(op, dtype):
    check(op, dtype, make_operand(op, dtype, (70000, 2), seed=5), [2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", [(2, 4, 8), (3, 5, 6), (2, 7, 10), (2, 3, 4, 6)],
                         ids=lambda s: "x".join(map(str, s)))
def test_nd_shapes(op, dtype, shape):
    check(op, dtype, make_operand(op, dtype, shape, seed=11), list(shape[1:]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_s_smaller_and_larger_than_the_array(op, dtype):
    a = make_operand(op, dtype, (2, 5, 6), seed=13)          # rfft: (2, 5, 6); irfft: (2, 5, 4, 2)
    for s in ([3, 4], [8, 9], [3, 9], [8, 4], [5, 6], [1, 1], [7, 2]):
        check(op, dtype, a, s)
    b = make_operand(op, dtype, (3, 40), seed=14)
    for s in ([16], [17], [64], [100]):
        check(op, dtype, b, s)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_non_contiguous_inputs(op, dtype):
    """A transposed view and a ``[:, ::2]`` view are read through their strides."""
    import torch
    rng = np.random.default_rng(17)
    for n in (6, 16, 1024):
        cols = n if op == "rfft" else n // 2 + 1
        tail = () if op == "rfft" else (2,)
        base = rng.standard_normal((cols, 5) + tail).astype(dtype)           # transposed
        t = torch.from_numpy(base).cuda()
        view = t.transpose(0, 1)
        assert not view.is_contiguous()
        check(op, dtype, view, [n], host=np.swapaxes(base, 0, 1), what="transposed")
        base = rng.standard_normal((5, 2 * cols) + tail).astype(dtype)       # every other column
        view = torch.from_numpy(base).cuda()[:, ::2]
        assert not view.is_contiguous()
        check(op, dtype, view, [n], host=base[:, ::2], what="[:, ::2]")


@pytest.mark.parametrize("dtype", DTYPES)
def test_irfft_ignores_imaginary_parts_of_dc_and_nyquist(dtype):
    for n in (8, 9, 12, 1024, 1000):
        a = make_operand("irfft", dtype, (3, n), seed=n)
        assert np.all(a[:, 0, 1] != 0) and np.all(a[:, -1, 1] != 0)
        got = check("irfft", dtype, a, [n])
        b = a.copy()
        b[:, 0, 1] = 0
        if n % 2 == 0:
            b[:, -1, 1] = 0
        np.testing.assert_array_equal(got, check("irfft", dtype, b, [n]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_op_level_plans_under_use_graph(op, dtype):
    """The op-level plans with ``use_graph=True``, three calls each.  Their ``s`` is a graph INPUT,
    i.e. a device value the executor has to read back: the recording pass gives up on that read
    and these calls run eagerly (checked: right results, no replay entry).  Recorded and replayed
    transforms: the next test."""
    for shape in ((3, 5, 6), (4, 1024)):
        for k in range(3):
            check(op, dtype, make_operand(op, dtype, shape, seed=20 + k), list(shape[1:]),
                  use_graph=True, what=f"use_graph call {k}")
        ex = executor(op, dtype, len(shape), use_graph=True)
        assert ex._no_replay and not ex._graphs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", [(3, 5, 6), (4, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_recorded_and_replayed_calls(op, dtype, shape):
    """``s`` derived from the operand's shape stays on the host, so the whole call (table kernel,
    chirp spectrum, one transform per axis) is recorded once and replayed: the capture and two
    replays on fresh inputs, at a Bluestein shape and at the one-row-per-workgroup 16-byte form."""
    import torch
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(fft_util.shape_plan(op, dtype, len(shape)), use_graph=True)
    s = list(shape[1:])
    bound = cap(dtype, sum(fft_util.axis_cost(n) for n in s))
    for call in range(3):
        host = make_operand(op, dtype, shape, seed=30 + call)
        (got,) = ex(torch.from_numpy(host).cuda())
        err = rel_l2(got.cpu().numpy(), exact(op, host, s))
        print(f"{op} {dtype} {shape} recorded call {call}: rel L2 {err:.3e} (cap {bound:.3e})")
        assert tuple(got.shape) == (spectrum_shape(shape) if op == "rfft" else shape)
        assert err <= bound, (op, dtype, shape, call, err, bound)
        assert ex._graphs and not ex._no_replay, call
    assert len(ex._graphs) + len(ex._reloc) >= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_empty_batch_and_fresh_output(op, dtype):
    import torch
    (got,) = executor(op, dtype, 3)(make_operand(op, dtype, (0, 4, 6)), np.array([4, 6], dtype="int64"))
    assert tuple(got.shape) == ((0, 4, 4, 2) if op == "rfft" else (0, 4, 6))
    assert got.dtype == getattr(torch, dtype)
    a = torch.from_numpy(make_operand(op, dtype, (2, 1), seed=3)).cuda()    # a length-1 transform
    keep = a.clone()
    (got,) = executor(op, dtype, 2)(a, np.array([1], dtype="int64"))
    assert got.data_ptr() != a.data_ptr()
    got.zero_()
    torch.cuda.synchronize()
    assert torch.equal(a, keep)


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_graph_cases_match_the_reference(name):
    """``fft.rfft`` / ``fft.irfft`` with every norm, ``is_odd``, the round trip and the gradients
    through both Ops: the committed plans against the reference's stored outputs."""
    from aesara_amd.executor import PlanExecutor
    c = CASES[name]
    dtype = c["dtype"]
    ex = PlanExecutor(fft_util.case_plan(c))
    got = [g.cpu().numpy() for g in ex(*fft_util.case_inputs(c))]
    L = c["L"]       # from the reference's own graph: the ``s`` of each of its FFT nodes (the generator)
    ref = fft_util.case_arrays(c, "out")
    want = fft_util.case_arrays(c, "exact") if dtype == "float32" else ref
    bound = cap(dtype, L) * (1 if dtype == "float32" else 2)
    for k, (g, w, r) in enumerate(zip(got, want, ref)):
        assert g.shape == r.shape and g.dtype == r.dtype, (k, g.shape, g.dtype, r.shape, r.dtype)
        err = rel_l2(g, w)
        print(f"{name} output {k}: rel L2 {err:.3e} (cap {bound:.3e}, L={L})")
        assert err <= bound, (name, k, err, bound)


@pytest.mark.parametrize("name", ["fft_grad_float32_3x5x6", "fft_round_float64_2x4x8"])
def test_graph_cases_replay_from_a_recorded_launch_list(name):
    """``s`` derived from the input's shape stays on the host, so the whole plan (table kernels,
    chirp spectrum, transforms) is recorded once and replayed."""
    from aesara_amd.executor import PlanExecutor
    c = CASES[name]
    ex = PlanExecutor(fft_util.case_plan(c), use_graph=True)
    ins = fft_util.case_inputs(c)
    want = fft_util.case_arrays(c, "exact" if c["dtype"] == "float32" else "out")
    bound = cap(c["dtype"], c["L"]) * (1 if c["dtype"] == "float32" else 2)
    for call in range(3):
        got = [g.cpu().numpy() for g in ex(*ins)]
        for k, (g, w) in enumerate(zip(got, want)):
            assert rel_l2(g, w) <= bound, (name, call, k, rel_l2(g, w), bound)
    assert ex._graphs and not ex._no_replay
