"""Conv2d / Conv2dGradW / Conv2dGradI on the device (csrc/conv.hip + the MFMA GEMM through
PlanExecutor): the committed plans of tests/golden/conv on the committed inputs against the
reference's stored outputs.  No front end is imported here.

Accuracy bars (tests/conv_util.py, derived there): op level, element by element,
|got - exact| <= K * eps * L + tiny (float64: against the reference's float64 output at twice that);
graph level, relative L2 error per output <= max(4 x the reference's own float32 error, K_max * eps)
(float64: 2 * K_max * eps against the reference's output).
"""
import numpy as np
import pytest

import conv_util
from conv_util import OPS, DTYPES
from golden_inputs import make_input

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in conv_util.load_conv_cases()}
GRAPH_CASES = sorted(n for n, c in CASES.items() if c["kind"] == "graph")
_EXECUTORS, _VALUES, _GOLDEN = {}, {}, {}


def case(name, dtype):
    return CASES[f"op_{name}_{dtype}"]


def executor(c, op, use_graph=False):
    from aesara_amd.executor import PlanExecutor
    key = (c["name"], op, use_graph)
    if key not in _EXECUTORS:
        _EXECUTORS[key] = PlanExecutor(conv_util.case_plan(c, op), use_graph=use_graph)
    return _EXECUTORS[key]


def values(c):
    """x, w, dy of a case (made once, never written)."""
    if c["name"] not in _VALUES:
        _VALUES[c["name"]] = {k: make_input(s) for k, s in c["specs"].items()}
    return _VALUES[c["name"]]


def golden(c, op):
    """(what to compare with, L, whether that is the reference's own output of the same precision)."""
    key = (c["name"], op)
    if key not in _GOLDEN:
        z = np.load(conv_util.case_file(c, op))
        f32 = c["dtype"] == "float32"
        _GOLDEN[key] = (z["exact"] if f32 else z["out"], z["L"], not f32, z["out"])
    return _GOLDEN[key]


def run(c, op, operands=None, use_graph=False):
    v = values(c)
    ins = conv_util.op_inputs(op, v["x"], v["w"], v["dy"]) if operands is None else operands
    (got,) = executor(c, op, use_graph)(*ins)
    return got.cpu().numpy()


def check(c, op, got, what="", scale=1.0):
    want, L, vs_ref, ref = golden(c, op)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    ratio = conv_util.op_ratio(got, want * scale, c["dtype"], c["K"][op], L * abs(scale), vs_ref)
    print(f"{c['name']} {op} {what}: K = {c['K'][op]}, worst element at {ratio:.3f} of the bar")
    assert ratio <= 1.0, (c["name"], op, what, ratio)
    return ratio


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f", "g", "h", "a5"])
def test_op_cases(name, op, dtype):
    c = case(name, dtype)
    got = run(c, op)
    check(c, op, got)
    if name == "g" and op == "gi":
        # subsample (3, 3) under a 3 x 3 kernel on 5 x 5: rows / columns 3 and 4 lie under no tap
        untouched = golden(c, op)[1] == 0
        assert untouched.any() and np.all(got[untouched] == 0)
        assert untouched[:, :, 3:, :].all() and untouched[:, :, :, 3:].all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_two_runs_give_the_same_bits(name, op, dtype):
    c = case(name, dtype)
    first = run(c, op)
    np.testing.assert_array_equal(first, run(c, op))


def _views(v):
    """The operands as non-contiguous device views holding the same values: the image as a
    dimshuffle(0, 3, 1, 2) view of an NHWC array, the kernel as a transposed view, topgrad as a
    [:, :, ::2, :] slice."""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(v["x"].transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
    w = torch.from_numpy(np.ascontiguousarray(v["w"].transpose(3, 2, 1, 0))).cuda().permute(3, 2, 1, 0)
    N, O, OH, OW = v["dy"].shape
    wide = np.zeros((N, O, 2 * OH, OW), v["dy"].dtype)
    wide[:, :, ::2, :] = v["dy"]
    wide[:, :, 1::2, :] = 7.0
    dy = torch.from_numpy(wide).cuda()[:, :, ::2, :]
    for t, a in ((x, v["x"]), (w, v["w"]), (dy, v["dy"])):
        assert tuple(t.shape) == a.shape and (not t.is_contiguous() or t.numel() <= 1)
    return {"x": x, "w": w, "dy": dy}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_non_contiguous_operands_give_the_bits_of_contiguous_copies(name, op, dtype):
    c = case(name, dtype)
    v = values(c)
    nc = _views(v)
    want = run(c, op)
    third = {"gw": v["w"], "gi": v["x"]}.get(op)          # gives its shape only
    got = run(c, op, {"fwd": [nc["x"], nc["w"]], "gw": [nc["x"], nc["dy"], third],
                      "gi": [nc["w"], nc["dy"], third]}[op])
    np.testing.assert_array_equal(got, want)
    check(c, op, got, "non-contiguous")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["b", "a5"])
def test_one_image_per_chunk_gives_the_bits_of_one_chunk(name, op, dtype, monkeypatch):
    c = case(name, dtype)
    ex = executor(c, op)
    cols = lambda t: sum(n in ("ahip_im2col2d", "ahip_col2im2d") for n in t)      # noqa: E731
    t0 = len(ex.trace)
    want = run(c, op)
    whole = cols(ex.trace[t0:])
    monkeypatch.setenv("AESARA_HIP_CONV_WS_MB", "0")
    t0 = len(ex.trace)
    got = run(c, op)
    assert whole == 1 and cols(ex.trace[t0:]) == conv_util.OP_CASES[name][0][0]
    np.testing.assert_array_equal(got, want)
    check(c, op, got, "one image per chunk")


@pytest.mark.parametrize("dtype", DTYPES)
def test_weight_gradient_summed_in_groups(dtype, monkeypatch):
    """Case a5 (N = 5) with room for the per-image products of two images only: sums of 2, 2 and 1
    images, the later ones added to the first.  Inside the bar, and the same bits whether im2col
    runs over the whole batch or image by image (the groups follow from the shapes alone)."""
    from aesara_amd.executor import PlanExecutor
    c = case("a5", dtype)
    ex = PlanExecutor(conv_util.case_plan(c, "gw"))
    ex.CONV_PARTS_BYTES = 2 * 6 * 4 * 3 * 2 * np.dtype(dtype).itemsize
    v = values(c)
    t0 = len(ex.trace)
    (got,) = ex(v["x"], v["dy"], v["w"])
    got = got.cpu().numpy()
    assert ex.trace[t0:].count("ahip_gemm") == 3 and ex.trace[t0:].count("ahip_gemm_batched") == 3
    check(c, "gw", got, "groups of two images")
    monkeypatch.setenv("AESARA_HIP_CONV_WS_MB", "0")
    (again,) = ex(v["x"], v["dy"], v["w"])
    np.testing.assert_array_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_recorded_and_replayed_calls(op, dtype):
    """Case a through ``use_graph=True``: the recording call and two replays with new values in the
    same device buffers.  The new values are the stored ones times powers of two, so the stored
    ``exact`` and ``L`` scale exactly."""
    import torch
    c = case("a", dtype)
    v = values(c)
    dev = {k: torch.from_numpy(a.copy()).cuda() for k, a in v.items()}
    ex = executor(c, op, use_graph=True)
    for call, (sx, sw, sd) in enumerate([(1.0, 1.0, 1.0), (2.0, 4.0, 0.5), (-0.5, 1.0, 8.0)]):
        for k, s in (("x", sx), ("w", sw), ("dy", sd)):
            dev[k].copy_(torch.from_numpy(v[k] * np.asarray(s, v[k].dtype)))
        (got,) = ex(*conv_util.op_inputs(op, dev["x"], dev["w"], dev["dy"]))
        scale = {"fwd": sx * sw, "gw": sx * sd, "gi": sw * sd}[op]
        check(c, op, got.cpu().numpy(), f"recorded call {call}", scale=scale)
        assert ex._graphs and not ex._no_replay, call


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPS)
def test_zero_sizes(op, dtype):
    """N = 0 and O = 0 with case a's settings: correctly shaped results; the weight gradient of an
    empty batch and the image gradient of no filters are zeros."""
    c = case("a", dtype)
    ex = executor(c, op)
    z = lambda *s: np.zeros(s, dtype)          # noqa: E731
    x, w, dy = np.ones((2, 4, 7, 6), dtype), np.ones((6, 4, 3, 2), dtype), np.ones((2, 6, 7, 7), dtype)
    n0 = {"fwd": ([z(0, 4, 7, 6), w], (0, 6, 7, 7)), "gw": ([z(0, 4, 7, 6), z(0, 6, 7, 7), w], (6, 4, 3, 2)),
          "gi": ([w, z(0, 6, 7, 7), z(0, 4, 7, 6)], (0, 4, 7, 6))}[op]
    o0 = {"fwd": ([x, z(0, 4, 3, 2)], (2, 0, 7, 7)), "gw": ([x, z(2, 0, 7, 7), z(0, 4, 3, 2)], (0, 4, 3, 2)),
          "gi": ([z(0, 4, 3, 2), z(2, 0, 7, 7), x], (2, 4, 7, 6))}[op]
    for ins, shape in (n0, o0):
        t0 = len(ex.trace)
        (got,) = ex(*ins)
        got = got.cpu().numpy()
        assert got.shape == shape and got.dtype == np.dtype(dtype)
        assert not np.any(got)
        launched = [t for t in ex.trace[t0:] if "col2d" in t or "im2d" in t or "gemm" in t]
        assert not launched, launched


def _after_an_error(dtype):
    for op in OPS:
        c = case("h", dtype)
        check(c, op, run(c, op), "after an error")


@pytest.mark.parametrize("dtype", DTYPES)
def test_errors_are_raised_before_any_launch(dtype):
    """Host-side checks with the reference's messages; the executors stay usable."""
    cb, ca = case("b", dtype), case("a", dtype)                # b: two groups
    o = lambda *s: np.ones(s, dtype)           # noqa: E731
    with pytest.raises(ValueError, match="number of input channels must be divible by num_groups"):
        executor(cb, "fwd")(o(3, 3, 9, 8), o(6, 2, 3, 3))
    _after_an_error(dtype)
    with pytest.raises(ValueError, match="number of input channels must be divible by num_groups"):
        executor(cb, "gw")(o(3, 3, 9, 8), o(3, 6, 3, 9), o(6, 2, 3, 3))
    _after_an_error(dtype)
    with pytest.raises(ValueError, match="should specify the number of channels of 1 group"):
        executor(cb, "fwd")(o(3, 4, 9, 8), o(6, 4, 3, 3))
    with pytest.raises(ValueError, match="should specify the number of channels of 1 group"):
        executor(ca, "fwd")(o(2, 4, 7, 6), o(6, 3, 3, 2))
    _after_an_error(dtype)
    # half mode, 3 x 2 kernel: an image of (7, 6) gives (7, 7); (8, 6) would give (8, 7)
    with pytest.raises(ValueError, match=r"invalid input_shape for gradInputs: .*\(2, 6, 8, 7\).*\(2, 6, 7, 7\)"):
        executor(ca, "gi")(o(6, 4, 3, 2), o(2, 6, 7, 7), o(2, 4, 8, 6))
    _after_an_error(dtype)
    # subsample (2, 1): image heights 8 and 9 both give 3 rows, 10 gives 4
    ex = executor(cb, "gi")
    (ok,) = ex(o(6, 2, 3, 3), o(3, 6, 3, 9), o(3, 4, 8, 8))
    assert tuple(ok.shape) == (3, 4, 8, 8)
    with pytest.raises(ValueError, match="invalid input_shape for gradInputs"):
        ex(o(6, 2, 3, 3), o(3, 6, 3, 9), o(3, 4, 10, 8))
    _after_an_error(dtype)


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_training_steps_match_the_reference(name):
    """A CNN training step (loss and the gradients of both kernels, the bias, the dense weight and
    the image): plain, and with filter_flip=False, two groups and dilation (2, 2)."""
    from aesara_amd.executor import PlanExecutor
    c = CASES[name]
    z = np.load(conv_util.case_file(c))
    got = [g.cpu().numpy() for g in PlanExecutor(conv_util.case_plan(c))(*conv_util.case_inputs(c))]
    assert len(got) == c["n_out"] == 6
    f32 = c["dtype"] == "float32"
    worst = 0.0
    for k, g in enumerate(got):
        ref = z[f"out{k}"]
        assert g.shape == ref.shape and g.dtype == ref.dtype, (k, g.shape, g.dtype)
        err, cap = conv_util.rel_l2(g, z[f"exact{k}"] if f32 else ref), conv_util.graph_cap(c, k)
        own = f", the reference's own {c['ref_err'][k]:.3e}" if f32 else ""
        print(f"{name} output {k}: rel L2 {err:.3e}, {err / cap:.4f} of the cap {cap:.3e}{own}")
        worst = max(worst, err / cap)
        assert err <= cap, (name, k, err, cap)
    print(f"{name}: worst ratio {worst:.4f}")
