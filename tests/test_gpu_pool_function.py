"""``pool_2d`` / ``pool_3d``, ``aesara.grad`` through them, ``max_pool_2d_same_size``, a Hessian-vector
product and whole CNN training steps under ``aesara.function(..., mode="HIP")``: the reference's front
end (from the packed overlay, like tests/test_gpu_conv_function.py) over the real PlanExecutor,
compared with the stored reference outputs of tests/golden/pool at the bars of tests/pool_util.py.
Skipped where the overlay is not packed."""
import os
import sys

import numpy as np
import pytest

import pool_util
import ref_overlay
from pool_util import OP_CASES

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_overlay.available(),
                                 reason="no reference front end (oracle/_ref overlay not packed)")]

CASES = {c["name"]: c for c in pool_util.load_pool_cases()}


@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    import aesara_amd
    aesara_amd.get_mode()            # registers linker "hip" / mode "HIP" with the reference
    return ae


@pytest.fixture(scope="module")
def gen(ae):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_pool_golden
    return gen_pool_golden


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _judge(c, op, got, what):
    z = np.load(pool_util.case_file(c))
    ref = z[f"{op}_out"]
    assert got.dtype == ref.dtype and got.shape == ref.shape, (op, got.dtype, got.shape)
    if op in pool_util.EXACT_OPS:
        assert pool_util.same_bits(got, ref), (c["name"], op, what)
        return
    f32 = c["dtype"] == "float32"
    ratio = pool_util.op_ratio(got, z[f"{op}_exact"] if f32 else ref, c["dtype"],
                               pool_util.reduction_length(c["case"], op), z[f"{op}_L"], not f32)
    print(f"{c['name']} {op} through aesara.function, {what}: {ratio:.3f} of the bar")
    assert ratio <= 1.0, (c["name"], op, what, ratio)


@pytest.mark.parametrize("dtype", pool_util.DTYPES)
@pytest.mark.parametrize("mode", pool_util.MODES)
@pytest.mark.parametrize("name", ["c", "d", "k"])
def test_pool_and_its_gradient_under_mode_hip(ae, name, mode, dtype):
    """y = pool_2d / pool_3d(x) and the gradient of sum(y * gz) with respect to x are the forward Op
    and its gradient Op on the case's operands.  Three calls: the second and third are replays of the
    recorded launch list.  ``average_exc_pad`` with padding: the forward runs, the gradient raises."""
    from aesara.tensor.signal.pool import pool_2d, pool_3d
    from aesara.tensor.type import TensorType
    c = CASES[f"op_{name}_{dtype}"]
    shape, ws, stride, pad, ib, _ = OP_CASES[name]
    x, gz = (TensorType(dtype, shape=(None,) * len(shape))(n) for n in ("x", "gz"))
    y = (pool_3d if len(ws) == 3 else pool_2d)(x, ws, ignore_border=ib, stride=stride, pad=pad, mode=mode)
    gop = "maxgrad" if mode == "max" else f"avggrad_{mode}"
    v = pool_util.case_values(name, dtype)
    if pool_util.raises(name, gop):
        f = ae.function([x], y, mode="HIP")
        _judge(c, f"fwd_{mode}", _np(f(v["x"])), "forward only")
        g = ae.function([x, gz], ae.grad((y * gz).sum(), x), mode="HIP")
        with pytest.raises(ValueError, match="padding must be zero for average_exc_pad"):
            g(v["x"], v["gz"])
        return
    f = ae.function([x, gz], [y, ae.grad((y * gz).sum(), x)], mode="HIP")
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert ops.count("Pool") == 1 and ops.count("MaxPoolGrad" if mode == "max" else "AvgPoolGrad") == 1, ops
    for call in range(3):
        got_y, got_gx = (_np(g) for g in f(v["x"], v["gz"]))
        _judge(c, f"fwd_{mode}", got_y, f"call {call}")
        _judge(c, gop, got_gx, f"call {call}")


def _graph(ae, gen, gname, dtype):
    c = CASES[f"{gname}_{dtype}"]
    ins, outs, _ = gen.GRAPHS[gname](dtype)
    f = ae.function(ins, outs, mode="HIP")
    z = np.load(pool_util.case_file(c))
    xs = pool_util.case_inputs(c)
    f32 = dtype == "float32"
    for call in range(2):
        got = [_np(g) for g in f(*xs)]
        assert len(got) == c["n_out"]
        for k, g in enumerate(got):
            ref = z[f"out{k}"]
            assert g.shape == ref.shape and g.dtype == ref.dtype, (k, g.shape, g.dtype)
            err, cap = pool_util.rel_l2(g, z[f"exact{k}"] if f32 else ref), pool_util.graph_cap(c, k)
            print(f"{c['name']} output {k}, call {call}: rel L2 {err:.3e}, {err / cap:.4f} of the cap {cap:.3e}")
            assert err <= cap, (c["name"], k, call, err, cap)
    return f


@pytest.mark.parametrize("dtype", pool_util.DTYPES)
@pytest.mark.parametrize("gname", ["cnn_plain", "cnn_padded"])
def test_cnn_training_steps_with_pooling_layers(ae, gen, gname, dtype):
    f = _graph(ae, gen, gname, dtype)
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert ops.count("Pool") == 2 and ops.count("MaxPoolGrad") == 1 and ops.count("AvgPoolGrad") == 1, ops


@pytest.mark.parametrize("dtype", pool_util.DTYPES)
def test_max_pool_2d_same_size(ae, gen, dtype):
    _graph(ae, gen, "same_size", dtype)


@pytest.mark.parametrize("dtype", pool_util.DTYPES)
def test_hessian_vector_product_reaches_the_gradient_of_the_gradient(ae, gen, dtype):
    f = _graph(ae, gen, "hvp", dtype)
    assert [n.op for n in f.maker.linker.plan.nodes].count("MaxPoolGradGrad") == 1


@pytest.mark.parametrize("dtype", pool_util.DTYPES)
def test_ten_sgd_steps_of_the_cnn_follow_the_reference(ae, gen, dtype):
    """conv -> relu -> max pool -> conv -> relu -> average pool -> dense -> cross-entropy on shared
    variables, ten updates: the loss sequence against the stored one within the graph cap."""
    c = CASES[f"sgd_{dtype}"]
    z = np.load(pool_util.case_file(c))
    f, _, specs = gen.sgd_function(dtype, "HIP")
    x, y = (pool_util.make_input(s) for s in specs)
    losses = np.array([_np(f(x, y)) for _ in range(c["steps"])]).astype(dtype)
    f32 = dtype == "float32"
    err, cap = pool_util.rel_l2(losses, z["exact0"] if f32 else z["out0"]), pool_util.graph_cap(c, 0)
    print(f"sgd_{dtype}: losses {losses[0]:.4f} -> {losses[-1]:.4f}, rel L2 {err:.3e}, {err / cap:.4f} of the cap "
          f"{cap:.3e}")
    assert losses[-1] < losses[0] and err <= cap, (err, cap)
