"""``aesara.function([x, w], conv2d(x, w), mode="HIP")`` and ``aesara.grad`` through it on the device:
the reference's front end (from the packed overlay, like tests/test_gpu_function_e2e.py) over the real
PlanExecutor, compared with the stored reference outputs of tests/golden/conv at the op-level bar of
tests/conv_util.py.  Skipped where the overlay is not packed."""
import numpy as np
import pytest

import conv_util
import ref_overlay
from golden_inputs import make_input

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_overlay.available(),
                                 reason="no reference front end (oracle/_ref overlay not packed)")]

CASES = {c["name"]: c for c in conv_util.load_conv_cases()}


@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    import aesara_amd
    aesara_amd.get_mode()            # registers linker "hip" / mode "HIP" with the reference
    return ae


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


@pytest.mark.parametrize("dtype", conv_util.DTYPES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_conv2d_and_its_gradients_under_mode_hip(ae, name, dtype):
    """y = conv2d(x, w) and the gradients of sum(y * dy) with respect to w and x are the three Ops on
    the case's operands: judged against the stored ``exact`` / ``L`` columns.  Three calls: the
    second and third are replays of the recorded launch list."""
    from aesara.tensor.nnet import conv2d
    from aesara.tensor.type import TensorType
    c = CASES[f"op_{name}_{dtype}"]
    s = conv_util.settings(name)
    x, w, dy = (TensorType(dtype, shape=(None,) * 4)(n) for n in ("x", "w", "dy"))
    y = conv2d(x, w, border_mode=s["border_mode"], subsample=s["subsample"], filter_flip=s["filter_flip"],
               filter_dilation=s["filter_dilation"], num_groups=s["num_groups"])
    f = ae.function([x, w, dy], [y] + ae.grad((y * dy).sum(), [w, x]), mode="HIP")
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert ops.count("Conv2d") == ops.count("Conv2dGradW") == ops.count("Conv2dGradI") == 1, ops
    v = {k: make_input(sp) for k, sp in c["specs"].items()}
    for call in range(3):
        got = [_np(g) for g in f(v["x"], v["w"], v["dy"])]
        for op, g in zip(conv_util.OPS, got):
            z = np.load(conv_util.case_file(c, op))
            f32 = dtype == "float32"
            ratio = conv_util.op_ratio(g, z["exact"] if f32 else z["out"], dtype, c["K"][op], z["L"], not f32)
            print(f"{c['name']} {op} through aesara.function, call {call}: {ratio:.3f} of the bar")
            assert g.dtype == z["out"].dtype and ratio <= 1.0, (name, op, call, ratio)
