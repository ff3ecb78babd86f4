"""AbstractConv2d and its two gradients through the rewrite query, the lowering and the executor's
host logic (no GPU): the committed plans of tests/golden/conv are what the linker lowers, the
family's other members are refused by name, ``border_mode`` resolves as the reference resolves it,
and a dry run gives the reference's shapes, errors and chunking while calling C-ABI entry points
only."""
import os
import sys

import numpy as np
import pytest

import conv_util
import ref_overlay
from conv_util import OPS

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")

CASES = {c["name"]: c for c in conv_util.load_conv_cases()}
CONV_CALLS = {"ahip_im2col2d", "ahip_col2im2d", "ahip_gemm", "ahip_gemm_batched", "ahip_copy_strided",
              "ahip_fill"}


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


@pytest.fixture(scope="module")
def gen(ae):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_conv_golden
    return gen_conv_golden


def dummy_mode():
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    return Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY)


def dry(c, op, *ins):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(conv_util.case_plan(c, op), dry_run=True)
    return ex, ex(*ins)


def ones(*shape):
    return np.ones(shape, "float32")


@needs_reference
def test_committed_plans_are_what_the_linker_lowers(gen):
    bad = []
    for name, c in CASES.items():
        if c["kind"] == "op":
            for op in OPS:
                plan = gen.lower(*gen.op_graph(op, c["dtype"], conv_util.settings(c["case"])), f"{name}_{op}")
                if plan.to_json() != c["plans"][op]:
                    bad.append((name, op))
                (node,) = [n for n in plan.nodes if n.op.startswith("Conv2d")]
                assert node.params == conv_util.plan_params(c["case"]), (name, op, node.params)
        else:
            ins, outs, specs = gen.cnn(c["dtype"], name.split("_")[1])
            if gen.lower(ins, outs, name).to_json() != c["plan"] or specs != c["inputs"]:
                bad.append(name)
    assert not bad, bad
    assert {c["case"] for c in CASES.values() if c["kind"] == "op"} == set(conv_util.OP_CASES)


@needs_reference
def test_conv2d_lowers_to_one_conv2d_node(ae):
    import aesara.tensor as at
    from aesara.tensor.nnet import conv2d
    x, w = at.tensor4("x"), at.tensor4("w")
    f = ae.function([x, w], conv2d(x, w, border_mode="half"), mode=dummy_mode())
    nodes = f.maker.linker.plan.nodes
    assert [n.op for n in nodes] == ["Conv2d"], [n.op for n in nodes]
    assert nodes[0].params == {"border_mode": "half", "subsample": [1, 1], "filter_dilation": [1, 1],
                               "filter_flip": True, "num_groups": 1}


@needs_reference
def test_grad_lowers_to_both_gradient_ops_with_host_shapes(ae):
    """``aesara.grad`` through conv2d: one Conv2dGradW and one Conv2dGradI whose ``shape`` operands
    reach the executor as host integer vectors (a dry run never needs a device value)."""
    import aesara.tensor as at
    from aesara.tensor.nnet import conv2d
    from aesara_amd.executor import PlanExecutor
    x, w = at.tensor4("x"), at.tensor4("w")
    y = conv2d(x, w, border_mode="half", subsample=(2, 1))
    f = ae.function([x, w], ae.grad((y ** 2).sum(), [w, x]), mode=dummy_mode())
    plan = f.maker.linker.plan
    ops = [n.op for n in plan.nodes]
    assert ops.count("Conv2dGradW") == 1 and ops.count("Conv2dGradI") == 1 and ops.count("Conv2d") == 1
    ex = PlanExecutor(plan, dry_run=True)
    seen = {}
    for name in ("_op_Conv2dGradW", "_op_Conv2dGradI"):
        def spy(node, args, orig=getattr(ex, name), name=name):
            seen[name] = args[2]
            return orig(node, args)
        setattr(ex, name, spy)
    dw, dx = ex(np.zeros((2, 3, 7, 6), "float64"), np.zeros((4, 3, 3, 2), "float64"))
    assert tuple(dw.shape) == (4, 3, 3, 2) and tuple(dx.shape) == (2, 3, 7, 6)
    assert isinstance(seen["_op_Conv2dGradW"], np.ndarray) and seen["_op_Conv2dGradW"].tolist() == [3, 2]
    assert isinstance(seen["_op_Conv2dGradI"], np.ndarray) and seen["_op_Conv2dGradI"].tolist() == [7, 6]
    assert seen["_op_Conv2dGradW"].dtype.kind == "i"


@needs_reference
def test_the_rest_of_the_family_is_refused_at_compile_time(ae):
    import aesara.tensor as at
    from aesara.tensor.nnet import abstract_conv as ac
    from aesara.tensor.type import TensorType
    from aesara_amd.lower import UnsupportedOp
    x, w = at.tensor4("x"), at.tensor4("w")
    w6 = TensorType("float64", shape=(None,) * 6)("w6")
    with pytest.raises(UnsupportedOp, match="unshared"):
        ae.function([x, w6], ac.AbstractConv2d(unshared=True)(x, w6), mode=dummy_mode())
    with pytest.raises(UnsupportedOp, match="unshared"):
        ae.function([x, w], ac.AbstractConv2d_gradWeights(unshared=True)(x, w, (3, 3, 2, 2)),
                    mode=dummy_mode())
    x5, w5 = (TensorType("float64", shape=(None,) * 5)(n) for n in ("x5", "w5"))
    with pytest.raises(UnsupportedOp, match="convdim = 3"):
        ae.function([x5, w5], ac.AbstractConv3d()(x5, w5), mode=dummy_mode())
    h = TensorType("float16", shape=(None,) * 4)("h")
    k = TensorType("float16", shape=(None,) * 4)("k")
    with pytest.raises(UnsupportedOp, match="float16"):
        ae.function([h, k], ac.AbstractConv2d()(h, k), mode=dummy_mode())


@needs_reference
@pytest.mark.parametrize("mode", ["valid", "half", "full", 2, (1, 2), ((1, 0), (2, 1)), (3, (0, 2))],
                         ids=str)
def test_border_mode_resolves_as_border_mode_to_pad(ae, mode):
    from aesara.tensor.nnet import abstract_conv as ac
    from aesara_amd.lower_conv import normalise_border_mode, resolve_pad
    for kshp in ((1, 1), (2, 3), (4, 4)):
        for dil in ((1, 1), (2, 3)):
            op = ac.AbstractConv2d(border_mode=mode, filter_dilation=dil)
            dil_kshp = tuple((k - 1) * d + 1 for k, d in zip(kshp, dil))
            param = normalise_border_mode(op.border_mode)
            assert param in ("half", "full") or (isinstance(param, list) and all(len(p) == 2 for p in param))
            assert resolve_pad(param, dil_kshp) == ac.border_mode_to_pad(op.border_mode, 2, dil_kshp), \
                (mode, kshp, dil)


def test_dry_run_of_every_committed_case():
    """Stored shapes and dtypes, C-ABI names only; one im2col / col2im per op-level call."""
    from aesara_amd.executor import PlanExecutor
    from golden_inputs import make_input
    for name, c in CASES.items():
        if c["kind"] == "op":
            v = {k: make_input(s) for k, s in c["specs"].items()}
            assert c["K"] == conv_util.reduction_lengths(c["case"])
            for op in OPS:
                ex, (got,) = dry(c, op, *conv_util.op_inputs(op, v["x"], v["w"], v["dy"]))
                want = np.load(conv_util.case_file(c, op))
                assert tuple(got.shape) == want["out"].shape == want["L"].shape and got.dtype == c["dtype"]
                assert set(ex.trace) <= CONV_CALLS, ex.trace
                # one launch for the batch, unless an image of col is no multiple of 16 bytes (case d:
                # 37 x 25 elements): then every image gets its own aligned slot and launch
                (N, C, _, _), (_, _, kh, kw), _ = conv_util.OP_CASES[c["case"]]
                tight = (C * kh * kw * int(np.prod(conv_util.out_hw(c["case"])))) % 4 == 0
                assert sum(t in ("ahip_im2col2d", "ahip_col2im2d") for t in ex.trace) == (1 if tight else N)
        else:
            ex = PlanExecutor(conv_util.case_plan(c), dry_run=True)
            got = ex(*conv_util.case_inputs(c))
            z = np.load(conv_util.case_file(c))
            for k, g in enumerate(got):
                assert tuple(g.shape) == z[f"out{k}"].shape and g.dtype == z[f"out{k}"].dtype.name
            assert all(t.startswith("ahip_") for t in ex.trace)
            assert c["K_max"] == 576                     # the first layer's weight gradient: 4 * 12 * 12


def test_the_stored_reference_outputs_are_inside_the_bar():
    """What the generator refuses to write otherwise; the bar is not vacuous for the reference's
    own float32 results either (some element above a hundredth of it)."""
    worst = 0.0
    for c in CASES.values():
        if c["kind"] != "op":
            continue
        for op in OPS:
            z = np.load(conv_util.case_file(c, op))
            if c["dtype"] == "float32":
                r = conv_util.op_ratio(z["out"], z["exact"], "float32", c["K"][op], z["L"])
                assert r <= 1.0, (c["name"], op, r)
                worst = max(worst, r)
            else:
                assert "exact" not in z.files
            # an output that is off by one average product (L / K) misses the bar by 1 / (2 K^2 eps):
            # by orders of magnitude for every reduction shorter than about a thousand terms
            K = c["K"][op]
            if z["L"].size and z["L"].max() > 0 and K <= 1000:
                off = z["out"].astype("float64") + z["L"] / K
                miss = conv_util.op_ratio(off, z["out"], c["dtype"], K, z["L"], True)
                assert miss > 0.4 / (K * K * conv_util.eps(c["dtype"])) > 3, (c["name"], op, miss)
    assert 0.01 < worst <= 1.0


def test_zero_sizes_launch_no_product():
    c = CASES["op_a_float32"]
    z = lambda *s: np.zeros(s, "float32")          # noqa: E731
    for op, ins, shape, filled in (
            ("fwd", [z(0, 4, 7, 6), ones(6, 4, 3, 2)], (0, 6, 7, 7), False),
            ("fwd", [ones(2, 4, 7, 6), z(0, 4, 3, 2)], (2, 0, 7, 7), False),
            ("gw", [z(0, 4, 7, 6), z(0, 6, 7, 7), ones(6, 4, 3, 2)], (6, 4, 3, 2), True),
            ("gw", [ones(2, 4, 7, 6), z(2, 0, 7, 7), z(0, 4, 3, 2)], (0, 4, 3, 2), False),
            ("gi", [ones(6, 4, 3, 2), z(0, 6, 7, 7), z(0, 4, 7, 6)], (0, 4, 7, 6), False),
            ("gi", [z(0, 4, 3, 2), z(2, 0, 7, 7), ones(2, 4, 7, 6)], (2, 4, 7, 6), True)):
        ex, (got,) = dry(c, op, *ins)
        assert tuple(got.shape) == shape and ex.trace == (["ahip_fill"] if filled else []), (op, ex.trace)
    # an image smaller than the kernel: empty spatial output, nothing launched
    ex, (got,) = dry(CASES["op_e_float32"], "fwd", ones(1, 1, 2, 40), ones(1, 1, 3, 3))
    assert tuple(got.shape) == (1, 1, 0, 38) and not ex.trace


def test_the_references_errors():
    ca, cb = CASES["op_a_float32"], CASES["op_b_float32"]          # b: two groups
    with pytest.raises(ValueError, match="number of input channels must be divible by num_groups"):
        dry(cb, "fwd", ones(3, 3, 9, 8), ones(6, 2, 3, 3))
    with pytest.raises(ValueError, match="number of filters must be divisible by num_groups"):
        dry(cb, "fwd", ones(3, 4, 9, 8), ones(5, 2, 3, 3))
    with pytest.raises(ValueError, match="should specify the number of channels of 1 group"):
        dry(cb, "fwd", ones(3, 4, 9, 8), ones(6, 4, 3, 3))
    with pytest.raises(ValueError, match="should specify the number of channels of 1 group"):
        dry(ca, "fwd", ones(2, 4, 7, 6), ones(6, 3, 3, 2))
    with pytest.raises(ValueError, match=r"invalid input_shape for gradInputs: the given input_shape would "
                                         r"produce an output of shape \(2, 6, 8, 7\), but the given topgrad "
                                         r"has shape \(2, 6, 7, 7\)"):
        dry(ca, "gi", ones(6, 4, 3, 2), ones(2, 6, 7, 7), ones(2, 4, 8, 6))
    # subsample (2, 1): image heights 8 and 9 give topgrad's 3 rows, 7 and 10 do not
    for H, ok in ((7, False), (8, True), (9, True), (10, False)):
        if ok:
            _, (got,) = dry(cb, "gi", ones(6, 2, 3, 3), ones(3, 6, 3, 9), ones(3, 4, H, 8))
            assert tuple(got.shape) == (3, 4, H, 8)
        else:
            with pytest.raises(ValueError, match="invalid input_shape for gradInputs"):
                dry(cb, "gi", ones(6, 2, 3, 3), ones(3, 6, 3, 9), ones(3, 4, H, 8))
    with pytest.raises(ValueError, match="produce an output of shape"):
        dry(ca, "gw", ones(2, 4, 7, 6), ones(2, 6, 7, 6), ones(6, 4, 3, 2))
    with pytest.raises(TypeError, match="float64 does not match float32"):
        dry(ca, "fwd", np.ones((2, 4, 7, 6), "float64"), ones(6, 4, 3, 2))


def test_negative_padding_is_refused():
    from aesara_amd.executor import PlanExecutor
    from aesara_amd.plan import Plan
    js = CASES["op_b_float32"]["plans"]["fwd"]
    plan = Plan.from_json(js)
    (node,) = [n for n in plan.nodes if n.op == "Conv2d"]
    node.params = dict(node.params, border_mode=[[-1, 0], [2, 1]])
    with pytest.raises(ValueError, match="border_mode must be >= 0"):
        PlanExecutor(plan, dry_run=True)(ones(3, 4, 9, 8), ones(6, 2, 3, 3))


def test_chunks_depend_on_shapes_and_the_switch_only(monkeypatch):
    """col of case a5 is 24 rows x 49 pixels per image: 4704 bytes in float32."""
    c = CASES["op_a5_float32"]
    ins = [ones(5, 4, 7, 6), ones(6, 4, 3, 2)]
    mib = lambda images: str((images * 4704 + 0.5) / 2 ** 20)          # noqa: E731
    for mb, launches in ((None, 1), ("0", 5), (mib(1), 5), (mib(2), 3), (mib(4), 2), (mib(5), 1)):
        if mb is None:
            monkeypatch.delenv("AESARA_HIP_CONV_WS_MB", raising=False)
        else:
            monkeypatch.setenv("AESARA_HIP_CONV_WS_MB", mb)
        ex, _ = dry(c, "fwd", *ins)
        assert ex.trace.count("ahip_im2col2d") == launches == ex.trace.count("ahip_gemm_batched"), (mb, ex.trace)


def test_argument_checks_of_the_library():
    """Nothing is launched: bad arguments come back as AHIP_EINVAL with a message."""
    import ctypes as C
    from aesara_amd._lib import DTYPE_CODES, lib
    f32, i32 = DTYPE_CODES["float32"], DTYPE_CODES["int32"]
    st = (C.c_int64 * 4)(1, 1, 1, 1)
    geo = (1, 1, 4, 4, 3, 3, 0, 0, 1, 1, 1, 1, 2, 2)
    assert lib.ahip_im2col2d(i32, None, st, *geo, None, None) == -1
    assert b"float32 / float64" in lib.ahip_last_error()
    assert lib.ahip_im2col2d(f32, None, st, 1, 1, 4, 4, 3, 3, -1, 0, 1, 1, 1, 1, 2, 2, None, None) == -1
    assert b"border_mode must be >= 0" in lib.ahip_last_error()
    assert lib.ahip_col2im2d(f32, None, 1, 1, 4, 4, 3, 3, 0, 0, 0, 1, 1, 1, 2, 2, None, None) == -1
    assert lib.ahip_col2im2d(f32, None, 1, 1, 1 << 16, 1 << 16, 3, 3, 0, 0, 1, 1, 1, 1, 2, 2, None, None) == -1
    assert b"too large" in lib.ahip_last_error()
    # empty problems return before any pointer is looked at
    assert lib.ahip_im2col2d(f32, None, st, 0, 1, 4, 4, 3, 3, 0, 0, 1, 1, 1, 1, 2, 2, None, None) == 0
    assert lib.ahip_col2im2d(f32, None, 0, 1, 4, 4, 3, 3, 0, 0, 1, 1, 1, 1, 2, 2, None, None) == 0
