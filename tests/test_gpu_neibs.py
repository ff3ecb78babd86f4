"""Images2Neibs on the device (csrc/neibs.hip): one-node plans against ``restate``, a NumPy restatement of the loops of
``Images2Neibs.perform`` (neighbours.py:311-349); exact.  The second call is a replay.  Pairs the reference calls "not
consistent" are skipped by asking ``neibs_geometry`` (7 of the 20 on the 2 x 3 x 7 x 9 image)."""
import numpy as np
import pytest
import torch

from aesara_amd.exec_neibs import MODES, band_split, neibs_geometry
from aesara_amd.plan import Node, Plan
from test_gpu_eigvalsh import dev

BAND = band_split(4, 3, 3, 1, 1, 10 ** 6, 3)[0]             # patch rows a workgroup: float32, 3 x 3, step 1, 5 columns
TILE = band_split(8, 3, 3, 1, 1, 1, 10 ** 6)[1]             # patch columns a workgroup: int64, 3 x 3, step 1

# (image shape, patch, step, mode, dtype)
CASES = [((1, 1, 1, 1), (1, 1), (1, 1), m, "float32") for m in MODES]
CASES += [((2, 3, 7, 9), (3, 3), s, m, "float32") for s in ((1, 1), (2, 3), (3, 3), (4, 6)) for m in MODES]
CASES += [((1, 2, 3, 5), (3, 5), (1, 1), m, "float32") for m in ("wrap_centered", "full", "half")]   # patch = image
CASES += [((1, 1, 7, 9), (3, 3), (2, 4), "wrap_centered", "float32"),        # a step that does not divide the image
          ((1, 2, BAND + 3, 5), (3, 3), (1, 1), "valid", "float32"),         # one patch row more than a band
          ((1, 1, 3, TILE + 3), (3, 3), (1, 1), "valid", "int64"),           # one patch column more than a tile
          ((1, 1, 3, 2101), (2, 2100), (1, 1), "valid", "int64"),            # a patch that LDS cannot hold
          ((1, 2, 6, 10), (2, 5), (2, 5), "valid", "float32"), ((1, 2, 6, 10), (2, 5), (1, 1), "full", "float32"),
          ((0, 3, 7, 9), (3, 3), (1, 1), "valid", "float32"), ((2, 3, 2, 9), (3, 3), (1, 1), "ignore_borders", "float32")]
CASES += [((2, 3, 7, 9), (3, 3), (2, 3), "valid", dt) for dt in ("bool", "int16", "float64")]
CASES += [((2, 3, 8, 16), (3, 3), (1, 1), m, dt) for m in ("half", "wrap_centered") for dt in ("int8", "float32")]     # 16-byte rows
CASES += [((2, 3, 8, 16), (2, 2), (2, 2), "valid", dt) for dt in ("float32", "float64")]                  # disjoint


def restate(x, patch, step, mode):
    (N, C, H, W), (r, c), (sr, sc) = x.shape, patch, step
    wrap = mode == "wrap_centered"
    pr, pc = {"valid": (0, 0), "ignore_borders": (0, 0), "full": (r - 1, c - 1)}.get(mode, (r // 2, c // 2))
    gr, gc = (-(-H // sr), -(-W // sc)) if wrap else (max(1 + (H + 2 * pr - r) // sr, 0), max(1 + (W + 2 * pc - c) // sc, 0))
    z = np.zeros((N, C, gr, gc, r, c), x.dtype)
    for a, b, i, j in np.ndindex(gr, gc, r, c):
        row, col = a * sr + i - pr, b * sc + j - pc
        if wrap:
            row, col = row % H, col % W
        if 0 <= row < H and 0 <= col < W:
            z[:, :, a, b, i, j] = x[:, :, row, col]
    return z.reshape(N * C * gr * gc, r * c)


def plan_of(dtype, mode, patch=None, step=None):
    plan = Plan(f"neibs_{dtype}_{mode}", {}, [], [], [])
    x = plan.new_var(dtype, [None] * 4, "x")
    if patch is None:
        vecs = [plan.new_var("int64", [None], k) for k in ("neib_shape", "neib_step")]
    else:
        vecs = [plan.add_const(np.asarray(v, "int64")) for v in (patch, step)]
    out = plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = [x] + (vecs if patch is None else []), [out]
    plan.nodes.append(Node("Images2Neibs", [x] + vecs, [out], {"mode": mode}))
    return plan


def image(shape, dtype):
    x = np.random.default_rng(sum(shape)).integers(1, 100, shape)
    return (x % 2 if dtype == "bool" else x).astype(dtype)


def run2(dtype, mode, patch, step, x):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan_of(dtype, mode, patch, step), use_graph=True)
    outs = [ex(x)[0].cpu().numpy() for _ in range(2)]
    assert len(ex._graphs) == 1 and not ex._no_replay and ex.trace.count("ahip_images2neibs") <= 2
    np.testing.assert_array_equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,patch,step,mode,dtype", CASES)
def test_images2neibs(shape, patch, step, mode, dtype):
    try:
        neibs_geometry(shape, patch, step, mode)
    except TypeError as e:
        pytest.skip(str(e))
    x = image(shape, dtype)
    np.testing.assert_array_equal(run2(dtype, mode, patch, step, dev(x)), restate(x, patch, step, mode), strict=True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["valid", "full", "wrap_centered"])
@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_views_are_read_through_their_strides(dtype, mode):
    big = image((3, 4, 9, 12), dtype)
    for view in (lambda t: t.transpose(2, 3), lambda t: t[1:, ::2, 2:, 1:10]):
        got = run2(dtype, mode, (3, 3), (1, 1), view(dev(big)))
        np.testing.assert_array_equal(got, restate(view(torch.from_numpy(big)).numpy(), (3, 3), (1, 1), mode))


@pytest.mark.gpu
def test_an_error_surfaces_in_the_first_call_and_in_the_next():
    from aesara_amd.executor import PlanExecutor
    x = image((2, 3, 7, 9), "float32")
    ex = PlanExecutor(plan_of("float32", "valid", (3, 3), (3, 3)), use_graph=True)
    for call in range(2):
        with pytest.raises(TypeError, match=r"neib_shape\[0\]=3, neib_step\[0\]=3 and ten4.shape\[2\]=7 not consistent"):
            ex(dev(x))
