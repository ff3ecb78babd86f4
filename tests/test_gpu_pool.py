"""Pool / MaxPoolGrad / AvgPoolGrad / MaxPoolGradGrad on the device (csrc/pool.hip through
PlanExecutor): the plans the four Ops lower to (pool_util.op_plan; tests/test_pool_lowering.py holds
the linker to them) on the committed inputs against the reference's stored outputs.  No front end is
imported here; whole graphs run in tests/test_gpu_pool_function.py.

Accuracy (tests/pool_util.py, derived there): ``max`` forward, ``MaxPoolGrad`` and grad-of-grad are
compared bit for bit with the reference's C result (NaNs in the same places); sums, averages and
``AvgPoolGrad`` element by element at |got - exact| <= K * eps * L + tiny (float64: against the
reference's float64 output at twice that).
"""
import numpy as np
import pytest

import pool_util
from pool_util import DTYPES, OP_CASES, OPS

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in pool_util.load_pool_cases()}
_EXECUTORS, _VALUES, _GOLDEN = {}, {}, {}


def case(name, dtype):
    return CASES[f"op_{name}_{dtype}"]


def executor(c, op, use_graph=False, sym=False):
    from aesara_amd.executor import PlanExecutor
    key = (c["name"], op, use_graph, sym)
    if key not in _EXECUTORS:
        plan = pool_util.op_plan(c["case"], op, c["dtype"], symbolic=sym)
        _EXECUTORS[key] = PlanExecutor(plan, use_graph=use_graph)
    return _EXECUTORS[key]


def golden(c):
    if c["name"] not in _GOLDEN:
        _GOLDEN[c["name"]] = dict(np.load(pool_util.case_file(c)))
    return _GOLDEN[c["name"]]


def values(c):
    """x, gz, ggx and maxout (the stored forward result) of a case (made once, never written)."""
    if c["name"] not in _VALUES:
        v = pool_util.case_values(c["case"], c["dtype"])
        v["maxout"] = golden(c)["fwd_max_out"]
        _VALUES[c["name"]] = v
    return _VALUES[c["name"]]


def inputs(c, op, **replace):
    v = values(c)
    return [replace.get(k, v[k]) for k in OPS[op][1]]


def run(c, op, ins=None, **kw):
    (got,) = executor(c, op, **kw)(*(inputs(c, op) if ins is None else ins))
    return got.cpu().numpy()


def check(c, op, got, what="", scale=1.0):
    """Exact ops: the reference's bits.  Bar ops: print and assert the worst ratio."""
    z = golden(c)
    ref = z[f"{op}_out"]
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    if op in pool_util.EXACT_OPS:
        assert op not in c["inexact"]
        assert pool_util.same_bits(got, ref * np.asarray(scale, ref.dtype)), (c["name"], op, what)
        return 0.0
    f32 = c["dtype"] == "float32"
    want = z[f"{op}_exact"] if f32 else ref
    K = pool_util.reduction_length(c["case"], op)
    ratio = pool_util.op_ratio(got, want * scale, c["dtype"], K, z[f"{op}_L"] * abs(scale), not f32)
    print(f"{c['name']} {op} {what}: K = {K}, worst element at {ratio:.3f} of the bar")
    assert ratio <= 1.0, (c["name"], op, what, ratio)
    return ratio


def uncovered(name):
    """Mask over the image of the cells that lie under no window."""
    g = pool_util.geometry(name)
    axes = []
    for k in range(g.ndim):
        cover = np.zeros(g.img[k], bool)
        for b, e in g.windows(k):
            cover[b:e] = True
        axes.append(cover)
    covered = axes[0]
    for a in axes[1:]:
        covered = covered[..., None] & a
    return np.broadcast_to(~covered, g.x_shape)


def _pairs(names, computed_only=False):
    return [(n, op) for n in names for op in pool_util.case_ops(n)
            if not (computed_only and pool_util.raises(n, op))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,op", _pairs(sorted(OP_CASES)))
def test_op_cases(name, op, dtype):
    c = case(name, dtype)
    if pool_util.raises(name, op):
        with pytest.raises(ValueError, match="padding must be zero for average_exc_pad"):
            run(c, op)
        return
    ex = executor(c, op)
    t0 = len(ex.trace)
    got = run(c, op)
    check(c, op, got)
    if got.size == 0:
        assert not ex.trace[t0:], ex.trace[t0:]              # an empty result launches nothing
    if op == "maxgrad" or op.startswith("avggrad"):
        # cells under no window (stride > window, the border that ignore_border cuts off) are 0
        free = uncovered(name)
        assert np.all(got[free] == 0)
        if name in ("e", "e_border", "g_empty"):
            assert free.any()
        if op.startswith("avggrad"):
            assert np.all(golden(c)[f"{op}_L"][free] == 0)
    if name == "n" and op == "maxgrad":
        # a NaN never compares equal: its two windows pass no gradient at all
        assert np.all(got[0, 0, 0:2, 0:2] == 0) and np.all(got[1, 2, 2:4, 2:4] == 0)
        assert np.count_nonzero(got) == got.size // 4 - 2
    if name == "n" and op == "fwd_max":
        assert np.isnan(got[0, 0, 0, 0]) and np.isnan(got[1, 2, 1, 1]) and np.isnan(got).sum() == 2


def _image_views(x):
    """The image as device views holding the same values: a [:, :, ::2, ::-1] slice of a taller,
    mirrored array; a dimshuffle(0, 3, 1, 2) view of an NHWC array; swapped leading dimensions."""
    import torch
    N, Cc, H, W = x.shape
    tall = np.full((N, Cc, 2 * H, W), 7.0, x.dtype)
    tall[:, :, ::2, :] = x[:, :, :, ::-1]
    # torch has no negative strides: the reversed view is built as a DevArray over the tall buffer
    from aesara_amd.device import DevArray
    base = DevArray.from_torch(torch.from_numpy(tall).cuda())
    s = base.strides
    sliced = base.view((N, Cc, H, W), (s[0], s[1], 2 * s[2], -s[3]), base.offset + (W - 1) * s[3])
    nhwc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    swapped = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2, 3))).cuda().permute(1, 0, 2, 3)
    return {"sliced": sliced, "nhwc": nhwc, "swapped": swapped}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["fwd_max", "fwd_sum", "fwd_average_exc_pad", "maxgrad", "gradgrad"])
@pytest.mark.parametrize("name", ["c", "t2"])
def test_strided_images_are_read_in_place(name, op, dtype):
    """Cases c and t2 (the latter: the gradient kernel of non-overlapping windows reading x cell by
    cell) on strided and transposed views of the image: the bits of the contiguous operand, and no
    copy kernel in the executor's trace."""
    c = case(name, dtype)
    want = run(c, op)
    ex = executor(c, op)
    for what, view in _image_views(values(c)["x"]).items():
        t0 = len(ex.trace)
        got = run(c, op, inputs(c, op, x=view))
        assert "ahip_copy_strided" not in ex.trace[t0:] and len(ex.trace[t0:]) == 1, (what, ex.trace[t0:])
        np.testing.assert_array_equal(got, want, err_msg=what)
        check(c, op, got, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["fwd_max", "fwd_average_inc_pad"])
@pytest.mark.parametrize("name", ["t2", "t4", "t14", "t34", "i"])
def test_streaming_loads_give_the_same_bits(name, op, dtype):
    """The forward kernels with non-temporal loads (the policy for images of 96 MiB or more, here
    switched on for a small one through the executor's threshold)."""
    from aesara_amd.executor import PlanExecutor
    c = case(name, dtype)
    ex = PlanExecutor(pool_util.op_plan(name, op, dtype))
    ex.BIG_STREAM = 1
    (got,) = ex(*inputs(c, op))
    np.testing.assert_array_equal(got.cpu().numpy(), run(c, op))
    check(c, op, got.cpu().numpy(), "streaming")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", ["fwd_max", "fwd_sum"])
def test_wide_loads_and_their_unaligned_fallback(op, dtype):
    """Case i (windows (1, 2), rows of 1030): from an aligned buffer a window row is one load; from
    a buffer that starts one element late, or whose rows are an odd number of elements apart, the
    same values come through single loads.  All three give the same bits."""
    import torch
    c = case("i", dtype)
    x = values(c)["x"]
    want = run(c, op)
    check(c, op, want, "aligned")
    late = torch.zeros(x.size + 1, dtype=torch.from_numpy(x).dtype, device="cuda")
    late[1:] = torch.from_numpy(x).reshape(-1).cuda()
    odd = torch.zeros((1, 1, 3, 1031), dtype=late.dtype, device="cuda")
    odd[..., :1030] = torch.from_numpy(x).cuda()
    for what, view in (("late", late[1:].reshape(x.shape)), ("odd rows", odd[..., :1030])):
        assert tuple(view.shape) == x.shape
        np.testing.assert_array_equal(run(c, op, [view]), want, err_msg=what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,op", _pairs(["c", "d"], computed_only=True))
def test_recorded_and_replayed_calls(name, op, dtype):
    """``use_graph=True``: the recording call, three replays on new values in the same device
    buffers (the stored ones times powers of two, so the stored columns scale exactly), then a call
    with another shape, which records again and agrees with the eager executor bit for bit."""
    import torch
    c = case(name, dtype)
    v = values(c)
    keys = OPS[op][1]
    dev = {k: torch.from_numpy(v[k].copy()).cuda() for k in keys}
    ex = executor(c, op, use_graph=True)
    data = {"maxgrad": "gz", "gradgrad": "ggx"}.get(op, "gz" if op.startswith("avggrad") else "x")
    for call, (sx, sd) in enumerate([(1.0, 1.0), (2.0, 0.5), (0.25, 4.0), (8.0, 2.0)]):
        for k in keys:
            s = sd if k == data else sx
            dev[k].copy_(torch.from_numpy(v[k] * np.asarray(s, v[k].dtype)))
        (got,) = ex(*[dev[k] for k in keys])
        check(c, op, got.cpu().numpy(), f"recorded call {call}", scale=sd)
        assert ex._graphs and not ex._no_replay, call
    shape = (1, 2, 9, 8)
    from aesara_amd.exec_pool import pool_geometry
    _, ws, stride, pad, ib, _ = OP_CASES[name]
    g = pool_geometry(shape, np.asarray(ws), np.asarray(stride), np.asarray(pad), 2, ib)
    rng = np.random.default_rng(5)
    x = np.round(rng.standard_normal(shape) * 2).astype(dtype)
    other = {"x": x, "gz": rng.standard_normal(g.out_shape).astype(dtype),
             "ggx": rng.standard_normal(shape).astype(dtype)}
    (mo,) = executor(c, "fwd_max")(x)
    other["maxout"] = mo.cpu().numpy()
    (got,) = ex(*[other[k] for k in keys])
    (eager,) = executor(c, op)(*[other[k] for k in keys])
    assert tuple(got.shape) == (g.x_shape if op == "maxgrad" or op.startswith("avggrad") else g.out_shape)
    np.testing.assert_array_equal(got.cpu().numpy(), eager.cpu().numpy())
    assert not ex._no_replay


@pytest.mark.parametrize("dtype", DTYPES)
def test_symbolic_ws_stride_pad_are_host_vectors(dtype):
    """Case c's plans with ``lvector`` ws / stride / pad: given case c's values they give case c's
    results, given case d's (padding (1, 2)) case d's — the same executor, nothing baked in."""
    iv = lambda t: np.asarray(t, "int64")        # noqa: E731
    c = case("c", dtype)
    for op in ("fwd_max", "fwd_average_exc_pad", "maxgrad", "avggrad_average_inc_pad", "gradgrad"):
        for target in ("c", "d"):
            t = case(target, dtype)
            geo = [iv(v) for v in OP_CASES[target][1:4]]
            got = run(c, op, inputs(t, op) + geo, sym=True)
            check(t, op, got, f"symbolic, geometry of case {target}")
    # the vectors steer host control flow: under use_graph such a plan runs eagerly, correctly
    for call in range(2):
        got = run(c, "maxgrad", inputs(c, "maxgrad") + [iv(v) for v in OP_CASES["c"][1:4]], sym=True,
                  use_graph=True)
        check(c, "maxgrad", got, f"symbolic under use_graph, call {call}")
    with pytest.raises(ValueError, match="stride must be a vector of size 2"):
        run(c, "fwd_max", [values(c)["x"], iv((3, 3)), iv((2,)), iv((0, 0))], sym=True)
    check(c, "fwd_max", run(c, "fwd_max"), "after an error")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("use_graph", [False, True])
def test_outputs_are_fresh(use_graph, dtype):
    """Writing into a returned gradient does not alter a later call."""
    c = case("f", dtype)
    for op in ("maxgrad", "avggrad_average_inc_pad", "fwd_max"):
        ex = executor(c, op, use_graph=use_graph)
        first = None
        for call in range(3):
            (got,) = ex(*inputs(c, op))
            if first is None:
                first = got.cpu().numpy()
            np.testing.assert_array_equal(got.cpu().numpy(), first)
            got.fill_(123.0)


def test_flat_indices_beyond_2_to_31():
    """float32, (65537, 8, 64, 64): 2^31 + 32768 elements.  The forward kernel and the average
    gradient take their 64-bit index form; the last image is checked against the first."""
    import torch
    c = case("a", "float32")
    N = 65537 * 8
    x = torch.zeros((N, 64, 64), dtype=torch.float32, device="cuda")
    img = torch.from_numpy(np.random.default_rng(3).standard_normal((64, 64)).astype("float32")).cuda()
    x[0] = img
    x[-1] = img
    (z,) = executor(c, "fwd_max")(x)
    assert tuple(z.shape) == (N, 32, 32)
    assert torch.equal(z[-1], z[0]) and torch.equal(z[0], img.reshape(32, 2, 32, 2).amax(dim=(1, 3)))
    assert not z[1:-1].any()
    del x
    gz = z
    gz[-2] = 3.0
    shape_only = torch.zeros(1, dtype=torch.float32, device="cuda").expand(N, 64, 64)
    (gx,) = executor(c, "avggrad_average_exc_pad")(shape_only, gz)
    assert tuple(gx.shape) == (N, 64, 64)
    want = z[0].repeat_interleave(2, 0).repeat_interleave(2, 1) / 4
    assert torch.equal(gx[-1], want) and torch.equal(gx[0], want)
    assert torch.equal(gx[-2], torch.full((64, 64), 0.75, device="cuda")) and not gx[1:-2].any()
