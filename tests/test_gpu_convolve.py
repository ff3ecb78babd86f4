"""Convolve on the device (csrc/convolve.hip through PlanExecutor): hand-built one-node plans against
``np.convolve`` in the three modes, at the kernel's edges: one element, swapped operands, ``n`` around one tap
chunk, ``m`` around one and two output tiles, and a ``valid`` call with 17 chunks of taps, which takes the tap split.
Float operands are Gaussian, exact in float32; the reference is float64, ``np.longdouble`` for float64 results.  The
bar is derived: ``|got - want| <= min(m, n) eps np.convolve(|a|, |v|)``, twice the classical bound of a sum of
``min(m, n)`` products in any order (worst ratio seen: DESIGN 3.3n).  Integers equal ``np.convolve`` on int64 copies
cast to the dtype, NumPy's wrap-around.  The second, replayed call repeats the bits of the first."""
import functools

import numpy as np
import pytest
import torch

from aesara_amd.exec_convolve import TAP_CHUNK, TILE_OUT
from aesara_amd.plan import Node, Plan
from test_gpu_eigvalsh import DTYPES, dev

MODES = ("full", "valid", "same")
SPLIT = (16 * TAP_CHUNK + 7, 16 * TAP_CHUNK + 5)            # m = n + 2: `valid` is three long dot products
SHAPES = [(1, 1), (5, 1), (3, 7), (7, 4)] + [(m, n) for n in (TAP_CHUNK - 1, TAP_CHUNK, TAP_CHUNK + 1)
                                             for m in (TILE_OUT - 1, TILE_OUT, TILE_OUT + 1, 2 * TILE_OUT + 3)]
CASES = [(m, n, mode) for m, n in SHAPES for mode in MODES] + [SPLIT + ("valid",)]
INT_CASES = [(m, n, mode) for m, n in ((3, 7), (TILE_OUT + 1, TAP_CHUNK + 1)) for mode in MODES] + [SPLIT + ("valid",)]


def plan_of(dtype, mode):
    plan = Plan(f"convolve_{dtype}_{mode}", {}, [], [], [])
    ins = [plan.new_var(dtype, [None], name) for name in ("a", "v")]
    out = plan.new_var(dtype, [None])
    plan.inputs, plan.outputs = list(ins), [out]
    plan.nodes.append(Node("Convolve", list(ins), [out], {"mode": mode}))
    return plan


@functools.lru_cache(maxsize=None)
def case(m, n, mode):
    """(a, v, float64 reference, longdouble reference, ``np.convolve(|a|, |v|)``), computed once."""
    rng = np.random.default_rng(1000 * m + n)
    a, v = (rng.standard_normal(k).astype("float32").astype("float64") for k in (m, n))
    return (a, v, np.convolve(a, v, mode), np.convolve(a.astype(np.longdouble), v.astype(np.longdouble), mode),
            np.convolve(np.abs(a), np.abs(v), mode))


def run2(dtype, mode, a, v):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan_of(dtype, mode), use_graph=True)
    outs = [ex(a, v)[0].cpu().numpy() for _ in range(2)]
    assert len(ex._graphs) == 1 and not ex._no_replay and outs[0].dtype == np.dtype(dtype)
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def check(got, m, n, mode, dtype, what):
    want64, wantld, scale = case(m, n, mode)[2:]
    err = np.abs(got.astype(np.longdouble).reshape(scale.shape) - (wantld if dtype == "float64" else want64))
    ratio = float(np.max(err / (min(m, n) * float(np.finfo(dtype).eps) * scale)))
    print(f"{what} m={m} n={n} {mode} {dtype}: worst error {ratio:.3f} of the bar")
    assert got.dtype == np.dtype(dtype) and ratio <= 1.0, (what, got.dtype, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,mode", CASES)
def test_convolve(m, n, mode, dtype):
    a, v = case(m, n, mode)[:2]
    check(run2(dtype, mode, dev(a.astype(dtype)), dev(v.astype(dtype))), m, n, mode, dtype, "convolve")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_reversed_and_strided_views_are_read_in_place(mode, dtype):
    from aesara_amd.device import DevArray
    m, n = TILE_OUT + 1, TAP_CHUNK + 1
    a, v = case(m, n, mode)[:2]
    abuf, vbuf = dev(a[::-1].astype(dtype)), dev(np.repeat(v, 2).astype(dtype))
    got = run2(dtype, mode, DevArray(abuf, m - 1, (m,), (-1,), dtype), DevArray(vbuf, 0, (n,), (2,), dtype))
    check(got, m, n, mode, dtype, "views")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int8", "uint8", "int32", "int64", "uint64"])
@pytest.mark.parametrize("m,n,mode", INT_CASES)
def test_integers_wrap_around_like_numpy(m, n, mode, dtype):
    rng = np.random.default_rng(m + n)
    a, v = (rng.integers(0 if dtype[0] == "u" else -8, 8, k) for k in (m, n))
    want = np.convolve(a, v, mode).astype(dtype)
    a, v = (torch.from_numpy(x.astype(dtype.lstrip("u") if dtype == "uint64" else dtype)).cuda() for x in (a, v))
    if dtype == "uint64":
        a, v = a.view(torch.uint64), v.view(torch.uint64)
    assert np.array_equal(run2(dtype, mode, a, v).view(want.dtype), want)
