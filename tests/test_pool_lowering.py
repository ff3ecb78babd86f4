"""Pool, MaxPoolGrad, AveragePoolGrad and DownsampleFactorMaxGradGrad through the rewrite query, the
lowering and the executor's host logic (no GPU): the plans of pool_util.op_plan are what the linker
lowers, ``pool_geometry`` gives the reference's shapes, windows and divisors, the rest of
the family is refused by name, a dry run raises the host errors and calls C-ABI entry points only,
and every stored reference output is inside its bar."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import pool_util
import ref_overlay
from pool_util import OP_CASES, OPS

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")

CASES = {c["name"]: c for c in pool_util.load_pool_cases()}
POOL_CALLS = {"ahip_pool_fwd", "ahip_maxpool_grad", "ahip_avgpool_grad", "ahip_maxpool_gradgrad"}


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


@pytest.fixture(scope="module")
def gen(ae):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_pool_golden
    return gen_pool_golden


def dummy_mode():
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    return Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY)


def case(name, dtype="float32"):
    return CASES[f"op_{name}_{dtype}"]


def dry(c, op, *ins, sym=False):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(pool_util.op_plan(c["case"], op, c["dtype"], symbolic=sym), dry_run=True)
    return ex, ex(*ins)


def operands(name, op, dtype="float32", **replace):
    """Zero operands of the right shapes for a dry run."""
    g = pool_util.geometry(name)
    shapes = {"x": g.x_shape, "maxout": g.out_shape, "gz": g.out_shape, "ggx": g.x_shape}
    return [replace.get(k, np.zeros(shapes[k], dtype)) for k in OPS[op][1]]


# ------------------------------------------------------------------ lowering ----------
@needs_reference
def test_the_tested_plans_are_what_the_linker_lowers(gen):
    bad = []
    for name, c in CASES.items():
        if c["kind"] == "op":
            for op in pool_util.case_ops(c["case"]):
                for sym in (False, True) if c["case"] == "c" else (False,):
                    plan = gen.lower(*gen.op_graph(c["case"], op, c["dtype"], symbolic=sym), f"{name}_{op}")
                    if not pool_util.same_lowering(plan, pool_util.op_plan(c["case"], op, c["dtype"], sym)):
                        bad.append((name, op, sym))
        elif c["kind"] == "graph":
            ins, outs, specs = gen.GRAPHS[c["graph"]](c["dtype"])
            ops = [n.op for n in gen.lower(ins, outs, name).nodes]
            if specs != c["inputs"] or any(ops.count(k) < n for k, n in gen.GRAPH_OPS[c["graph"]].items()):
                bad.append(name)
    assert not bad, bad
    assert {c["case"] for c in CASES.values() if c["kind"] == "op"} == set(OP_CASES)


@needs_reference
def test_each_op_lowers_to_its_plan_op(ae):
    """The test that shows the feature: without the lowering the first compile raises
    ``UnsupportedOp: Pool has no HIP lowering``."""
    import aesara.tensor as at
    from aesara.tensor.signal import pool as rp
    x, z, g = at.tensor4("x"), at.tensor4("z"), at.tensor4("g")
    geo = ((3, 3), (2, 2), (1, 1))
    built = {
        "Pool": ([x], rp.Pool(ignore_border=True, mode="average_inc_pad", ndim=2)(x, *geo),
                 {"mode": "average_inc_pad", "ignore_border": True, "ndim": 2}),
        "MaxPoolGrad": ([x, z, g], rp.MaxPoolGrad(ignore_border=True, ndim=2)(x, z, g, *geo),
                        {"mode": "max", "ignore_border": True, "ndim": 2}),
        "AvgPoolGrad": ([x, g], rp.AveragePoolGrad(ignore_border=False, mode="sum", ndim=2)(x, g, (3, 3), (2, 2)),
                        {"mode": "sum", "ignore_border": False, "ndim": 2}),
        "MaxPoolGradGrad": ([x, z, g], rp.DownsampleFactorMaxGradGrad(ignore_border=True, ndim=2)(x, z, g, *geo),
                            {"mode": "max", "ignore_border": True, "ndim": 2}),
    }
    for opname, (ins, out, params) in built.items():
        f = ae.function(ins, out, mode=dummy_mode())
        nodes = f.maker.linker.plan.nodes
        assert [n.op for n in nodes] == [opname], [n.op for n in nodes]
        assert nodes[0].params == params
        # ws, stride, pad stay operands: three constant integer vectors behind the data
        assert len(nodes[0].inputs) == len(ins) + 3
    t3 = at.tensor3("t")
    f = ae.function([t3], rp.Pool(ignore_border=True, mode="max", ndim=1)(t3, (3,), (2,), (1,)), mode=dummy_mode())
    assert f.maker.linker.plan.nodes[0].params == {"mode": "max", "ignore_border": True, "ndim": 1}
    t5 = at.tensor5("t5")
    f = ae.function([t5], rp.pool_3d(t5, (2, 2, 2), ignore_border=True), mode=dummy_mode())
    pools = [n for n in f.maker.linker.plan.nodes if n.op == "Pool"]
    assert len(pools) == 1 and pools[0].params["ndim"] == 3


@needs_reference
@pytest.mark.parametrize("mode", pool_util.MODES)
def test_grad_of_pool_2d_lowers_completely(ae, mode):
    """``aesara.grad`` through ``pool_2d`` (and, for ``max``, the gradient of that): every node of
    the rewritten graph has a lowering, and the pooling Ops stay what they are under ``fast_run``."""
    import aesara.tensor as at
    from aesara.tensor.signal.pool import pool_2d
    from aesara_amd.executor import PlanExecutor
    x, v = at.tensor4("x"), at.tensor4("v")
    y = pool_2d(x, (3, 3), ignore_border=True, stride=(2, 2), pad=(1, 1) if mode != "average_exc_pad" else (0, 0),
                mode=mode)
    gx = ae.grad((y ** 2).sum(), x)
    outs = [y, gx] + ([ae.grad((gx * v).sum(), x)] if mode == "max" else [])
    f = ae.function([x, v], outs, mode=dummy_mode(), on_unused_input="ignore")
    plan = f.maker.linker.plan
    ops = [n.op for n in plan.nodes]
    assert ops.count("Pool") == 1
    if mode == "max":
        assert ops.count("MaxPoolGrad") >= 1 and ops.count("MaxPoolGradGrad") == 1, ops
    else:
        assert ops.count("AvgPoolGrad") == 1, ops
    ex = PlanExecutor(plan, dry_run=True)
    res = ex(np.zeros((2, 3, 7, 9), "float64"), np.zeros((2, 3, 7, 9), "float64"))
    assert tuple(res[0].shape) == ((2, 3, 4, 5) if mode != "average_exc_pad" else (2, 3, 3, 4))
    assert all(tuple(r.shape) == (2, 3, 7, 9) for r in res[1:])
    assert POOL_CALLS & set(ex.trace)


@needs_reference
def test_the_rest_of_the_family_is_refused_at_compile_time(ae):
    import aesara.tensor as at
    from aesara.tensor.signal import pool as rp
    from aesara.tensor.type import TensorType
    from aesara_amd.lower import UnsupportedOp
    x = at.tensor4("x")
    with pytest.raises(UnsupportedOp, match="MaxPoolRop"):
        ae.function([x], rp.MaxPoolRop(ignore_border=True, ndim=2)(x, x, (2, 2)), mode=dummy_mode())
    i = TensorType("int32", shape=(None,) * 4)("i")
    with pytest.raises(UnsupportedOp, match="int32.*float32 / float64 only"):
        ae.function([i], rp.Pool(ignore_border=True, mode="max", ndim=2)(i, (2, 2)), mode=dummy_mode())
    h = TensorType("float16", shape=(None,) * 4)("h")
    with pytest.raises(UnsupportedOp, match="float16"):
        ae.function([h], rp.Pool(ignore_border=True, mode="sum", ndim=2)(h, (2, 2)), mode=dummy_mode())
    x6 = TensorType("float32", shape=(None,) * 6)("x6")
    with pytest.raises(UnsupportedOp, match="ndim = 4"):
        ae.function([x6], rp.Pool(ignore_border=True, mode="max", ndim=4)(x6, (2, 2, 2, 2)), mode=dummy_mode())
    g6 = TensorType("float32", shape=(None,) * 6)("g6")
    with pytest.raises(UnsupportedOp, match="ndim = 4"):
        ae.function([x6, g6], rp.AveragePoolGrad(ignore_border=True, mode="sum", ndim=4)(x6, g6, (2, 2, 2, 2)),
                    mode=dummy_mode())


# ------------------------------------------------------------------ geometry ----------
def brute_force(shape, ws, stride, pad, ignore_border, mode):
    """The contract restated: output extents, per-dimension windows (image coordinates) and
    divisor factors."""
    nd = len(ws)
    outs, windows, sizes = [], [], []
    for X, w, s, p in zip(shape[len(shape) - nd:], ws, stride, pad):
        P = X + 2 * p
        if ignore_border:
            o = P // s if w == s else max((P - w) // s + 1, 0)
        else:
            o = (P - 1) // s + 1 if s >= w else max(0, (P - 1 - w + s) // s) + 1
        wins, szs = [], []
        for j in range(o):
            lo, hi = j * s, min(j * s + w, P)
            clo, chi = max(lo, p), min(hi, P - p)
            wins.append((clo - p, chi - p))
            szs.append({"max": 1, "sum": 1, "average_inc_pad": hi - lo, "average_exc_pad": chi - clo}[mode])
        outs.append(o)
        windows.append(wins)
        sizes.append(szs)
    return tuple(outs), windows, sizes


@pytest.mark.parametrize("name", sorted(OP_CASES))
def test_pool_geometry_restates_the_contract(name):
    shape, ws, stride, pad, ib, _ = OP_CASES[name]
    for mode in pool_util.MODES:
        g = pool_util.geometry(name, mode)
        outs, windows, sizes = brute_force(shape, ws, stride, pad, ib, mode)
        assert g.out == outs and g.out_shape == tuple(shape[:len(shape) - len(ws)]) + outs
        for k in range(len(ws)):
            assert g.windows(k) == windows[k], (name, mode, k)
            assert g.sizes(k) == sizes[k], (name, mode, k)
            assert all(0 <= b < e <= g.img[k] for b, e in g.windows(k))
    assert name != "g_empty" or g.out == (0, 0)


@needs_reference
def test_pool_geometry_gives_the_reference_out_shape(ae):
    from aesara.tensor.signal.pool import Pool
    from aesara_amd.exec_pool import pool_geometry
    for X, w, s, p, ib in itertools.product(range(1, 12), (1, 2, 3, 4), (1, 2, 3, 5), (0, 1, 2), (True, False)):
        if p >= w or (p and not ib):
            continue
        want = [int(v) for v in Pool.out_shape((3, X, X + 1), (w, w), ib, (s, s), (p, p), 2)]
        try:
            got = pool_geometry((3, X, X + 1), np.array([w, w]), np.array([s, s]), np.array([p, p]), 2, ib)
        except ValueError:
            assert not ib and min(want) <= 0
            continue
        assert list(got.out_shape) == want, (X, w, s, p, ib)


def test_pool_geometry_raises_the_host_errors():
    from aesara_amd.exec_pool import pool_geometry
    v = lambda *a: np.asarray(a, "int64")        # noqa: E731
    ok = dict(ndim=2, ignore_border=True)
    with pytest.raises(ValueError, match="ws must be a vector of size 2"):
        pool_geometry((2, 6, 6), v(2), v(2, 2), v(0, 0), **ok)
    with pytest.raises(ValueError, match="stride must be a vector of size 2"):
        pool_geometry((2, 6, 6), v(2, 2), v(2, 2, 2), v(0, 0), **ok)
    with pytest.raises(ValueError, match="pad must be a vector of size 2"):
        pool_geometry((2, 6, 6), v(2, 2), v(2, 2), v(0), **ok)
    with pytest.raises(ValueError, match="window .* must be positive"):
        pool_geometry((2, 6, 6), v(2, 0), v(2, 2), v(0, 0), **ok)
    with pytest.raises(ValueError, match="stride .* must be positive"):
        pool_geometry((2, 6, 6), v(2, 2), v(-1, 2), v(0, 0), **ok)
    with pytest.raises(ValueError, match="must not be negative"):
        pool_geometry((2, 6, 6), v(2, 2), v(2, 2), v(0, -1), **ok)
    with pytest.raises(ValueError, match="padding must be smaller than strides"):
        pool_geometry((2, 6, 6), v(2, 2), v(2, 2), v(2, 0), **ok)
    with pytest.raises(ValueError, match="padding must be zero when ignore border is False"):
        pool_geometry((2, 6, 6), v(2, 2), v(2, 2), v(1, 1), 2, False)
    with pytest.raises(ValueError, match="without ignore_border needs a non-empty"):
        pool_geometry((2, 0, 6), v(2, 2), v(1, 1), v(0, 0), 2, False)
    with pytest.raises(ValueError, match="a window holds padding only"):
        pool_geometry((2, 0, 6), v(2, 2), v(2, 2), v(1, 1), **ok)
    with pytest.raises(TypeError, match="integers"):
        pool_geometry((2, 6, 6), np.asarray([2.0, 2.0]), v(2, 2), v(0, 0), **ok)
    assert pool_geometry((2, 3), v(3, 4), v(3, 4), v(0, 0), **ok).out_shape == (0, 0)


# ------------------------------------------------------------------ dry runs ----------
@pytest.mark.parametrize("name", sorted(OP_CASES))
def test_dry_runs_give_the_shapes_and_call_only_pool_entry_points(name):
    c = case(name)
    g = pool_util.geometry(name)
    for op in pool_util.case_ops(name):
        if pool_util.raises(name, op):
            continue
        ex, (out,) = dry(c, op, *operands(name, op))
        want = g.x_shape if op in ("maxgrad",) or op.startswith("avggrad") else g.out_shape
        assert tuple(out.shape) == want and out.dtype == "float32", (name, op, out.shape)
        launched = [t for t in ex.trace if t.startswith("ahip_")]
        if name == "g_empty" and want == g.out_shape:
            assert not launched, (op, launched)           # an empty result: nothing is launched
        else:
            assert len(launched) == 1 and launched[0] in POOL_CALLS, (name, op, launched)


def test_host_errors_are_raised_in_the_offending_call():
    c, cd = case("c"), case("d")
    for op, bad in (("maxgrad", "gz"), ("maxgrad", "maxout"), ("avggrad_sum", "gz"), ("gradgrad", "maxout")):
        with pytest.raises(ValueError, match=rf"\(2, 3, 3, 4\), but the given {bad} has shape \(2, 3, 3, 5\)"):
            dry(c, op, *operands("c", op, **{bad: np.zeros((2, 3, 3, 5), "float32")}))
    with pytest.raises(ValueError, match=r"ggx of shape \(2, 3, 7, 9\), but the given ggx has shape \(2, 3, 7, 8\)"):
        dry(c, "gradgrad", *operands("c", "gradgrad", ggx=np.zeros((2, 3, 7, 8), "float32")))
    with pytest.raises(ValueError, match="padding must be zero for average_exc_pad") as ei:
        dry(cd, "avggrad_average_exc_pad", *operands("d", "avggrad_average_exc_pad"))
    assert "[HIP step" in str(ei.value)                 # annotated with the node like the other ops
    with pytest.raises(TypeError, match="does not match float32"):
        dry(c, "fwd_max", np.zeros((2, 3, 7, 9), "float64"))
    # symbolic ws / stride / pad: host vectors at run time
    iv = lambda *a: np.asarray(a, "int64")       # noqa: E731
    x = np.zeros((2, 3, 7, 9), "float32")
    ex, (out,) = dry(c, "fwd_max", x, iv(3, 3), iv(2, 2), iv(0, 0), sym=True)
    assert tuple(out.shape) == (2, 3, 3, 4)
    ex, (out,) = dry(c, "fwd_max", x, iv(2, 4), iv(1, 3), iv(1, 2), sym=True)
    assert tuple(out.shape) == (2, 3, 8, 4)
    with pytest.raises(ValueError, match="ws must be a vector of size 2"):
        dry(c, "fwd_max", x, iv(3, 3, 3), iv(2, 2), iv(0, 0), sym=True)
    with pytest.raises(ValueError, match="stride .* must be positive"):
        dry(c, "maxgrad", x, np.zeros((2, 3, 3, 4), "float32"), np.zeros((2, 3, 3, 4), "float32"),
            iv(3, 3), iv(2, 0), iv(0, 0), sym=True)
    with pytest.raises(ValueError, match="must not be negative"):
        dry(c, "avggrad_average_inc_pad", x, np.zeros((2, 3, 3, 4), "float32"), iv(3, 3), iv(2, 2), iv(0, -1),
            sym=True)


def test_entry_points_refuse_geometry_that_would_leave_the_buffers():
    """No launch is made: only the argument checks of csrc/pool.hip (no GPU in this tier)."""
    from aesara_amd import _lib
    lib = _lib.lib
    i64 = lambda *a: (C.c_int64 * len(a))(*a)          # noqa: E731
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    strides = i64(0, 0, 36, 0, 6, 1)

    def geo(O=(1, 3, 3), ws=(1, 2, 2), stride=(1, 2, 2), pad=(0, 0, 0), X=(1, 6, 6)):
        return i64(1, 1, 2, *X, *O, *ws, *stride, *pad)
    EINVAL = _lib.AHIP_EINVAL
    f32 = _lib.DTYPE_CODES["float32"]
    assert lib.ahip_pool_fwd(_lib.DTYPE_CODES["int32"], 0, 0, geo(), p, strides, p, None) == EINVAL
    assert b"float32 / float64 only" in lib.ahip_last_error()
    assert lib.ahip_pool_fwd(f32, 7, 0, geo(), p, strides, p, None) == EINVAL
    assert b"unknown mode" in lib.ahip_last_error()
    assert lib.ahip_pool_fwd(f32, 0, 0, geo(O=(1, 4, 3)), p, strides, p, None) == EINVAL
    assert b"window outside the image" in lib.ahip_last_error()
    assert lib.ahip_maxpool_grad(f32, geo(pad=(0, 2, 0)), p, strides, p, p, p, None) == EINVAL
    assert b"smaller than the window" in lib.ahip_last_error()
    assert lib.ahip_avgpool_grad(f32, 0, geo(), p, p, None) == EINVAL              # max has no average gradient
    assert lib.ahip_maxpool_gradgrad(f32, geo(stride=(1, 0, 2)), p, strides, p, p, p, None) == EINVAL
    assert lib.ahip_pool_fwd(f32, 0, 0, geo(), None, strides, p, None) == EINVAL
    assert b"null pointer" in lib.ahip_last_error()
    # an empty result is not an error and needs no pointers
    assert lib.ahip_pool_fwd(f32, 0, 0, geo(O=(1, 0, 0), ws=(1, 7, 7), stride=(1, 7, 7)), None, strides, None, None) == 0


# ------------------------------------------------------------------ fixtures ----------
def test_fixtures_load_and_every_stored_output_is_inside_its_bar():
    worst, n_exact = 0.0, 0
    for name, c in CASES.items():
        z = np.load(pool_util.case_file(c))
        if c["kind"] != "op":
            assert all(f"out{k}" in z for k in range(c["n_out"]))
            if c["dtype"] == "float32":
                for k in range(c["n_out"]):
                    assert pool_util.rel_l2(z[f"out{k}"], z[f"exact{k}"]) <= pool_util.graph_cap(c, k)
            continue
        g = pool_util.geometry(c["case"])
        assert not c["inexact"], (name, c["inexact"])
        for op in pool_util.case_ops(c["case"]):
            if pool_util.raises(c["case"], op):
                assert op in c["raises"] and f"{op}_out" not in z
                continue
            out = z[f"{op}_out"]
            want = g.x_shape if op == "maxgrad" or op.startswith("avggrad") else g.out_shape
            assert out.shape == want and out.dtype == np.dtype(c["dtype"]), (name, op, out.shape)
            K = pool_util.reduction_length(c["case"], op)
            if op in pool_util.EXACT_OPS:
                n_exact += 1
                assert c["perform_agrees"][op] or (op == "maxgrad" and c["case"] in pool_util.TIE_WITH_PADDING) \
                    or (op == "fwd_max" and c["case"] == "n"), (name, op)
                continue
            L = z[f"{op}_L"]
            assert L.shape == out.shape and np.all(np.abs(out) <= L * (1 + K * pool_util.eps(c["dtype"])))
            if c["dtype"] == "float64":
                continue        # no more exact result is stored to judge a float64 output against
            ratio = pool_util.op_ratio(out, z[f"{op}_exact"], c["dtype"], K, L)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, op, ratio)
    assert n_exact >= 3 * 2 * (len(OP_CASES) - 1) and 0.0 < worst <= 1.0
    # the zero cells of the gradients: stride 3 under a 2 x 2 window leaves rows / columns 2 untouched
    z = np.load(pool_util.case_file(case("e")))
    for op in ("maxgrad", "avggrad_sum", "avggrad_average_inc_pad", "avggrad_average_exc_pad"):
        assert np.all(z[f"{op}_out"][:, :, 2, :] == 0) and np.all(z[f"{op}_out"][:, :, :, 2] == 0)
        assert np.any(z[f"{op}_out"][:, :, :2, :2] != 0)
