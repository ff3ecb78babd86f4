"""Shared by the pooling tests and tools/gen_pool_golden.py: the fixtures under tests/golden/pool,
the case table and the accuracy bars of the pooling Ops.

Exact results.  ``Pool`` in mode ``max`` selects: no arithmetic.  ``MaxPoolGrad`` and
``DownsampleFactorMaxGradGrad`` add, per result element, the same terms in the same order as the
reference's C loop (ascending window order / row-major window walk).  All three are compared with
``np.array_equal`` against the reference's output, NaNs in the same places.

Op-level bar (derived, not tuned; conv_util's bound with the pooling reduction lengths).  A
floating-point sum of K terms, in any order, has error at most gamma_K * sum|t_i| with
gamma_K ~ K * eps / 2 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section
3.1); one more rounding for the division.  The bar is twice that, element by element:

    |got - exact| <= K * eps(dtype) * L + tiny(dtype)

``L`` is the same Op evaluated by the reference in float64 on the absolute values of its data
operand.  Forward (``sum`` and the averages): K = the window's element count.  ``AveragePoolGrad``:
K = the largest number of windows that cover one cell, plus 1 for the division.  float32 results
are judged against ``exact`` (the reference's graph in float64 on the same values), float64 results
against the reference's own float64 output at 2 * K * eps * L, because both carry the bound.  Where
``L == 0`` the bar is ``tiny``: a gradient cell under no window must be 0.

Graph-level bar: exactly ``conv_util.graph_cap`` — relative L2 error per output <= max(4 x the
reference's own float32 error, K_max * eps), float64: 2 * K_max * eps against the reference's
output, with K_max the longest reduction of the graph (the convolutions').
"""
import json
import os

import numpy as np

from aesara_amd.plan import Node, Plan
from conv_util import eps, graph_cap, op_bar, op_ratio, rel_l2  # noqa: F401
from golden_inputs import make_input

POOL_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool")
DTYPES = ("float32", "float64")
MODES = ("max", "sum", "average_inc_pad", "average_exc_pad")
AVG_MODES = MODES[1:]
# op key -> (plan op, data operands)
OPS = {"fwd_max": ("Pool", ("x",)), "fwd_sum": ("Pool", ("x",)),
       "fwd_average_inc_pad": ("Pool", ("x",)), "fwd_average_exc_pad": ("Pool", ("x",)),
       "maxgrad": ("MaxPoolGrad", ("x", "maxout", "gz")),
       "avggrad_sum": ("AvgPoolGrad", ("x", "gz")),
       "avggrad_average_inc_pad": ("AvgPoolGrad", ("x", "gz")),
       "avggrad_average_exc_pad": ("AvgPoolGrad", ("x", "gz")),
       "gradgrad": ("MaxPoolGradGrad", ("x", "maxout", "ggx"))}
EXACT_OPS = ("fwd_max", "maxgrad", "gradgrad")


def op_mode(op):
    return op.split("_", 1)[1] if op.startswith(("fwd_", "avggrad_")) else "max"


# name -> (x shape, ws, stride, pad, ignore_border, data kind).  The pooled dimensions are the last
# len(ws) ones.  Data kinds: "normal"; "ties" (values from {0, 1, 2}); "ints" (small integers: exact
# sums, and the larger fixtures compress); "nan" (normal with two NaNs, see case_values).
OP_CASES = {
    "a": ((2, 3, 6, 6), (2, 2), (2, 2), (0, 0), True, "normal"),
    "b": ((2, 3, 7, 9), (3, 2), (3, 2), (0, 0), False, "normal"),
    "c": ((2, 3, 7, 9), (3, 3), (2, 2), (0, 0), True, "normal"),
    "c_border": ((2, 3, 7, 9), (3, 3), (2, 2), (0, 0), False, "normal"),
    "d": ((2, 3, 7, 9), (3, 3), (2, 2), (1, 2), True, "normal"),
    "e": ((2, 3, 5, 5), (2, 2), (3, 3), (0, 0), True, "normal"),
    "e_border": ((2, 3, 5, 5), (2, 2), (3, 3), (0, 0), False, "normal"),
    "f": ((2, 3, 8, 8), (2, 2), (1, 1), (0, 0), True, "normal"),
    "g": ((2, 3, 2, 3), (3, 4), (3, 4), (0, 0), False, "normal"),
    "g_empty": ((2, 3, 2, 3), (3, 4), (3, 4), (0, 0), True, "normal"),
    "h": ((2, 3, 6, 6), (2, 2), (2, 2), (0, 0), True, "ties"),
    "h3": ((2, 3, 6, 6), (3, 3), (2, 2), (0, 0), True, "ties"),
    "h_pad": ((2, 3, 6, 6), (3, 3), (2, 2), (1, 1), True, "ties"),
    "i": ((1, 1, 3, 1030), (1, 2), (1, 2), (0, 0), True, "ints"),
    "i3": ((1, 1, 3, 1030), (3, 3), (2, 2), (0, 0), True, "ints"),
    "j": ((6, 6), (2, 2), (2, 2), (0, 0), True, "normal"),
    "j5": ((2, 1, 3, 6, 6), (2, 2), (2, 2), (0, 0), True, "normal"),
    "k": ((2, 2, 5, 6, 7), (2, 3, 2), (2, 2, 1), (1, 1, 0), True, "normal"),
    "l": ((3, 11), (3,), (2,), (1,), True, "normal"),
    "n": ((2, 3, 6, 6), (2, 2), (2, 2), (0, 0), True, "nan"),
    # overlapping windows with a partial one at the far border (the second branch of out_shape)
    "o_border": ((2, 3, 8, 9), (3, 3), (2, 2), (0, 0), False, "normal"),
    # rows that are a multiple of 16 bytes in both dtypes: the smallest shapes that reach
    # pool_fwd_tile_kernel (window rows x columns 2 x 2, 4 x 4, 1 x 4), the four-column row load of
    # pool_fwd_kernel (3 x 4) and pool_grad_disjoint_kernel — with cells under no window (t23, t3),
    # a partial border window (t3_border), padding (t3_pad) and three pooled dimensions (t3d)
    "t2": ((2, 3, 8, 8), (2, 2), (2, 2), (0, 0), True, "ties"),
    "t4": ((2, 3, 8, 16), (4, 4), (4, 4), (0, 0), True, "normal"),
    "t14": ((2, 3, 8, 8), (1, 4), (1, 4), (0, 0), True, "normal"),
    "t34": ((2, 3, 9, 8), (3, 4), (3, 4), (0, 0), True, "normal"),
    "t23": ((2, 3, 8, 8), (2, 2), (3, 3), (0, 0), True, "normal"),
    "t3": ((2, 3, 8, 8), (3, 3), (3, 3), (0, 0), True, "normal"),
    "t3_border": ((2, 3, 8, 8), (3, 3), (3, 3), (0, 0), False, "normal"),
    "t3_pad": ((2, 3, 8, 8), (3, 3), (3, 3), (1, 1), True, "normal"),
    "t3d": ((2, 2, 4, 6, 8), (2, 2, 2), (2, 2, 2), (0, 0, 0), True, "normal"),
}
TIE_WITH_PADDING = ("h_pad",)      # MaxPoolGrad.perform shifts its windows here; the C windows hold


def case_ops(name):
    """The op keys a case runs: everything, except case n (max only: NaN propagation)."""
    return ("fwd_max", "maxgrad") if name == "n" else tuple(OPS)


def raises(name, op):
    """The one combination that must raise on the host instead of computing."""
    return op == "avggrad_average_exc_pad" and max(OP_CASES[name][3]) != 0


def geometry(name, mode="max"):
    from aesara_amd.exec_pool import pool_geometry
    shape, ws, stride, pad, ib, _ = OP_CASES[name]
    return pool_geometry(shape, np.asarray(ws), np.asarray(stride), np.asarray(pad), len(ws), ib, mode)


def input_specs(name, dtype):
    shape, _, _, _, _, kind = OP_CASES[name]
    out = geometry(name).out_shape
    shapes = {"x": shape, "gz": out, "ggx": shape}
    specs = {}
    for i, (k, s) in enumerate(shapes.items()):
        if kind == "ties" and k == "x":
            specs[k] = {"kind": "randint", "seed": 70 + i, "low": 0, "high": 3, "shape": list(s), "dtype": dtype}
        elif kind in ("ints", "ties"):
            specs[k] = {"kind": "randint", "seed": 70 + i, "low": -3, "high": 4, "shape": list(s), "dtype": dtype}
        else:
            specs[k] = {"kind": "normal", "seed": 70 + i, "shape": list(s), "dtype": dtype, "scale": 1.0,
                        "shift": 0.0}
    return specs


def case_values(name, dtype):
    """x, gz, ggx of a case.  Case n: a NaN that is the LAST cell of window (0, 0) of image [0, 0]
    and one that is the FIRST cell of window (1, 1) of image [1, 2]."""
    v = {k: make_input(s) for k, s in input_specs(name, dtype).items()}
    if OP_CASES[name][5] == "nan":
        v["x"][0, 0, 1, 1] = np.nan
        v["x"][1, 2, 2, 2] = np.nan
    return v


def reduction_length(name, op):
    """K of the bar (module docstring)."""
    g = geometry(name)
    if op.startswith("fwd_"):
        return int(np.prod(g.ws))
    if op.startswith("avggrad_"):
        k = 1
        for d in range(g.ndim):
            cover = np.zeros(g.img[d], int)
            for b, e in g.windows(d):
                cover[b:e] += 1
            k *= int(cover.max()) if cover.size else 0
        return k + 1
    return 1


def plan_params(name, op):
    return {"mode": op_mode(op), "ignore_border": OP_CASES[name][4], "ndim": len(OP_CASES[name][1])}


def load_pool_cases():
    with open(os.path.join(POOL_GOLDEN, "cases.json")) as f:
        return json.load(f)["cases"]


def op_plan(name, op, dtype, symbolic=False):
    """The one-node plan an op key of a case lowers to (tests/test_pool_lowering.py holds the linker
    to it): the data operands, then ws / stride / pad as int64 constants — or, ``symbolic``, as
    three more inputs."""
    _, ws, stride, pad, _, _ = OP_CASES[name]
    plan = Plan(f"op_{name}_{dtype}_{op}" + ("_sym" if symbolic else ""), {}, [], [], [])
    nd = len(OP_CASES[name][0])
    data = [plan.new_var(dtype, [None] * nd, k) for k in OPS[op][1]]
    if symbolic:
        geo = [plan.new_var("int64", [None], k) for k in ("ws", "stride", "pad")]
    else:
        geo = [plan.add_const(np.asarray(v, "int64")) for v in (ws, stride, pad)]
    out = plan.new_var(dtype, [None] * nd)
    plan.inputs, plan.outputs = data + (geo if symbolic else []), [out]
    plan.nodes.append(Node(OPS[op][0], data + geo, [out], plan_params(name, op)))
    return plan


def same_lowering(lowered, built):
    """Whether the plan the linker lowered is ``built``: one node, same op, parameters and inputs,
    the same constant ws / stride / pad."""
    if len(lowered.nodes) != 1 or len(lowered.inputs) != len(built.inputs):
        return False
    a, b = lowered.nodes[0], built.nodes[0]

    def operand(plan, v):
        var = plan.vars[v]
        return (var.dtype, var.const_value().tolist()) if var.const is not None else \
            (var.dtype, len(var.shape), plan.inputs.index(v))
    return a.op == b.op and a.params == b.params and a.outputs == lowered.outputs and \
        [operand(lowered, v) for v in a.inputs] == [operand(built, v) for v in b.inputs]


def case_inputs(c):
    return [make_input(s) for s in c["inputs"]]


def case_file(c):
    return os.path.join(POOL_GOLDEN, c["name"] + ".npz")


def same_bits(got, want):
    """np.array_equal with NaNs in the same places."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(
        np.array_equal(got, want, equal_nan=True))
