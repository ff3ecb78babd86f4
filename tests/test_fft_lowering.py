"""RFFTOp / IRFFTOp through the lowering and the executor's host logic (no GPU): the committed
plans of tests/golden/fft are what the linker lowers, a dry run produces the reference's output
shapes and dtypes and calls only C-ABI entry points, and the refusals are the documented ones."""
import os
import sys

import numpy as np
import pytest

import fft_util
import ref_overlay

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")

CASES = {c["name"]: c for c in fft_util.load_fft_cases()}
LENGTHS = [1, 2, 4, 8, 16, 32, 64, 128, 1024, 4096, 3, 5, 6, 7, 10, 12, 17, 100, 1000, 2047, 2048]
ND_SHAPES = [(2, 4, 8), (3, 5, 6), (2, 7, 10), (2, 3, 4, 6)]


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


@pytest.fixture(scope="module")
def gen(ae):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_fft_golden
    return gen_fft_golden


def dry(name, *ins):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(fft_util.case_plan(CASES[name]), dry_run=True)
    return ex, ex(*ins)


@needs_reference
def test_committed_plans_are_what_the_linker_lowers(gen):
    built = {}
    for name, mk in gen.op_cases():
        built[name] = gen.lower(*mk(), name)
    for name, dt, mk, _specs in gen.graph_cases():
        built[name] = gen.lower(*mk(dt), name)
    assert set(built) == set(CASES)
    bad = [n for n, p in built.items() if p.to_json() != CASES[n]["plan"]]
    assert not bad, bad


@needs_reference
def test_rfft_lowers_to_an_rfft_node(ae):
    import aesara.tensor as at
    from aesara.compile.mode import Mode
    from aesara.tensor import fft
    from aesara_amd.linker import HIP_QUERY, HipLinker
    x = at.tensor3("x")
    y = fft.irfft(fft.rfft(x, norm="ortho"), norm="ortho")
    f = ae.function([x], [y, ae.grad(y.sum(), x)],
                    mode=Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY))
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert "RFFT" in ops and "IRFFT" in ops


@needs_reference
def test_float16_is_refused_by_name(ae):
    from aesara.compile.mode import Mode
    from aesara.tensor import fft
    from aesara.tensor.type import TensorType
    from aesara_amd.linker import HIP_QUERY, HipLinker
    from aesara_amd.lower import UnsupportedOp
    x = TensorType("float16", shape=(None, None))("x")
    with pytest.raises(UnsupportedOp, match="float16"):
        ae.function([x], fft.rfft(x),
                    mode=Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY))


@needs_reference
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_dry_run_gives_the_reference_shapes_and_dtypes(ae, dtype):
    """The reference's own Ops (perform: NumPy) on zeros of every tested shape against a dry run
    of the committed plan; the dry run's trace holds C-ABI names only."""
    import aesara.tensor as at
    from aesara.tensor import fft
    from aesara.tensor.type import TensorType
    shapes = [(b, n) for n in LENGTHS for b in (1, 3)] + ND_SHAPES
    extra_s = {(3, 5, 6): [[2, 4], [8, 9], [3, 9]], (3, 40): [[16], [17], [64]]}
    fns = {}
    for nd in (2, 3, 4):
        a, A = (TensorType(dtype, shape=(None,) * k)() for k in (nd, nd + 1))
        s = at.lvector()
        fns["rfft", nd] = ae.function([a, s], fft.rfft_op(a, s))
        fns["irfft", nd] = ae.function([A, s], fft.irfft_op(A, s))
    for shape in shapes + list(extra_s):
        for s in [list(shape[1:])] + extra_s.get(shape, []):
            s = np.asarray(s, dtype="int64")
            for op in ("rfft", "irfft"):
                full = shape if op == "rfft" else tuple(shape[:-1]) + (shape[-1] // 2 + 1, 2)
                x = np.zeros(full, dtype=dtype)
                want = fns[op, len(shape)](x, s)
                ex, (got,) = dry(f"op_{op}_{dtype}_{len(shape)}d", x, s)
                assert tuple(got.shape) == want.shape and got.dtype == want.dtype.name, (op, shape, s)
                assert ex.trace and all(t.startswith("ahip_") for t in ex.trace), ex.trace
                assert {t for t in ex.trace if "fft" in t} <= {"ahip_fft_r2c", "ahip_fft_c2c", "ahip_fft_c2r"}


def test_dry_run_of_the_graph_level_cases():
    """Committed graph-level plans: a dry run gives the stored outputs' shapes and dtypes."""
    for name, c in CASES.items():
        if c["kind"] != "graph":
            continue
        ex, got = dry(name, *fft_util.case_inputs(c))
        for g, w in zip(got, fft_util.case_arrays(c, "out")):
            assert tuple(g.shape) == w.shape and g.dtype == w.dtype.name, name
        n_fft = sum(n.op in ("RFFT", "IRFFT") for n in fft_util.case_plan(c).nodes)
        assert c["L"] >= n_fft * (len(c["inputs"][0]["shape"]) - 1)      # at least 1 per axis per node
        assert all(t.startswith("ahip_") for t in ex.trace)


def test_empty_batch_launches_nothing():
    ex, (got,) = dry("op_rfft_float32_3d", np.zeros((0, 4, 6), "float32"), np.array([4, 6]))
    assert tuple(got.shape) == (0, 4, 4, 2) and not ex.trace
    ex, (got,) = dry("op_irfft_float64_3d", np.zeros((0, 4, 4, 2), "float64"), np.array([4, 6]))
    assert tuple(got.shape) == (0, 4, 6) and not ex.trace


@pytest.mark.parametrize("op", ["rfft", "irfft"])
def test_zero_points_raise_numpys_error(op):
    x = np.zeros((2, 4, 6) if op == "rfft" else (2, 4, 4, 2), "float32")
    for s in ([4, 0], [0, 6]):
        with pytest.raises(ValueError, match=r"Invalid number of FFT data points \(0\) specified\."):
            dry(f"op_{op}_float32_3d", x, np.array(s))
        ref = np.fft.rfftn if op == "rfft" else np.fft.irfftn
        with pytest.raises(ValueError, match=r"Invalid number of FFT data points \(0\) specified\."):
            ref(np.zeros((2, 4, 6)), s=s, axes=(1, 2))


@pytest.mark.parametrize("op", ["rfft", "irfft"])
@pytest.mark.parametrize("n", [8192, 4097, 2049, 6000])
def test_lengths_past_the_limit_are_refused_at_call_time(op, n):
    x = np.zeros((1, 8) if op == "rfft" else (1, 5, 2), "float64")
    with pytest.raises(NotImplementedError, match=rf"length {n}\b.*4096.*2048"):
        dry(f"op_{op}_float64_2d", x, np.array([n]))


def test_workspace_sizes_and_limits_of_the_library():
    from aesara_amd._lib import DTYPE_CODES, lib
    f32, f64 = DTYPE_CODES["float32"], DTYPE_CODES["float64"]
    assert lib.ahip_fft_ws_bytes(f32, 1024) == 1024 * 8
    assert lib.ahip_fft_ws_bytes(f64, 4096) == 4096 * 16
    # Bluestein: twiddles [m] + chirp [n] + chirp spectrum [m], m = next_pow2(2n - 1)
    assert lib.ahip_fft_ws_bytes(f32, 1000) == 2 * 2048 * 8 + 8192
    assert lib.ahip_fft_ws_bytes(f64, 2048) == 2048 * 16       # a power of two: no chirp
    assert lib.ahip_fft_ws_bytes(f64, 2047) == 2 * 4096 * 16 + 32768
    for n in (0, -3, 4097, 8192, 2049):
        assert lib.ahip_fft_ws_bytes(f32, n) == 0
    assert lib.ahip_fft_ws_bytes(DTYPE_CODES["int32"], 8) == 0
    # argument checks of the shim (nothing is launched)
    assert lib.ahip_fft_r2c(f32, None, 1, 0, 1, 0, 0, 1, 0, None, 0, 2, 2, None, 0, None) == -1
    assert b"Invalid number of FFT data points (0) specified." in lib.ahip_last_error()
    assert lib.ahip_fft_c2r(f32, None, 1, 8192, 1, 0, 0, 2, 0, None, 0, 1, 1, None, 0, None) == -5
    assert b"8192" in lib.ahip_last_error() and b"4096" in lib.ahip_last_error()


@pytest.mark.parametrize("op", ["rfft", "irfft"])
@pytest.mark.parametrize("shape", [(3, 5, 6), (4, 1024), (2, 3, 4, 6)])
def test_shape_derived_s_stays_on_the_host(op, shape):
    """The hand-built plans the GPU test replays: a dry run gives NumPy's shapes and never needs the
    value of a device array (``s`` is host integer arithmetic)."""
    from aesara_amd.executor import PlanExecutor
    full = shape if op == "rfft" else tuple(shape[:-1]) + (shape[-1] // 2 + 1, 2)
    ex = PlanExecutor(fft_util.shape_plan(op, "float32", len(shape)), dry_run=True)
    (got,) = ex(np.zeros(full, "float32"))
    assert tuple(got.shape) == (tuple(shape[:-1]) + (shape[-1] // 2 + 1, 2) if op == "rfft" else shape)
    assert set(ex.trace) <= {"ahip_fft_r2c", "ahip_fft_c2c", "ahip_fft_c2r"} and ex.trace


def _inc_plan(idx_list, n_idx, set_instead_of_inc, y_ndim):
    from aesara_amd.plan import Node, Plan, Var
    vs = {0: Var(0, "int64", []), 1: Var(1, "int64", []), 2: Var(2, "int64", []),
          3: Var(3, "int64", [3]), 4: Var(4, "int64", [None] * y_ndim)}
    for k in range(n_idx):
        vs[5 + k] = Var(5 + k, "int64", [])
    out = 5 + n_idx
    vs[out] = Var(out, "int64", [3])
    nodes = [Node("MakeVector", [0, 1, 2], [3], {"dtype": "int64"})]
    if y_ndim == 1:             # the value is a host vector too: MakeVector of the first two scalars
        vs[4] = Var(4, "int64", [2])
        nodes.append(Node("MakeVector", [0, 1], [4], {"dtype": "int64"}))
    nodes += [Node("IncSubtensor", [3, 4] + [5 + k for k in range(n_idx)], [out],
                  {"idx_list": idx_list, "set_instead_of_inc": set_instead_of_inc, "inplace": False})]
    return Plan("inc_host", vs, [0, 1, 2] + ([4] if y_ndim == 0 else []) + [5 + k for k in range(n_idx)],
                [out], nodes)


@pytest.mark.parametrize("set_", [True, False])
def test_incsubtensor_on_a_host_integer_vector_stays_on_the_host(set_):
    """``set_subtensor(s[-1], ...)`` on a MakeVector of host integers (tensor/fft.py:89, :202) is shape
    arithmetic: NumPy's result as a host array, no device call; positive and negative runtime
    indices and a slice; the operand vector is not written."""
    from aesara_amd.executor import PlanExecutor
    i64 = lambda v: np.asarray(v, dtype="int64")                          # noqa: E731
    base = [4, 5, 6]
    for index in (2, -1, -3, 0):
        ex = PlanExecutor(_inc_plan([{"index": "in"}], 1, set_, 0), dry_run=True)
        (got,) = ex(i64(4), i64(5), i64(6), i64(10), i64(index))
        want = np.array(base)
        want[index] = 10 if set_ else want[index] + 10
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == want.tolist()
        assert not ex.trace
    ex = PlanExecutor(_inc_plan([{"slice": [1, None, None]}], 0, set_, 1), dry_run=True)
    y = np.array([4, 5], dtype="int64")
    (got,) = ex(i64(4), i64(5), i64(6))
    want = np.array(base)
    want[1:] = y if set_ else want[1:] + y
    assert isinstance(got, np.ndarray) and got.tolist() == want.tolist() and not ex.trace
    ex = PlanExecutor(_inc_plan([{"slice": ["in", "in", None]}], 2, set_, 0), dry_run=True)
    (got,) = ex(i64(4), i64(5), i64(6), i64(3), i64(-2), i64(3))
    want = np.array(base)
    want[-2:3] = 3 if set_ else want[-2:3] + 3
    assert got.tolist() == want.tolist() and not ex.trace
