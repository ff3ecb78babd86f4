"""Shared by the convolution tests and tools/gen_conv_golden.py: the fixtures under
tests/golden/conv, the case table and the accuracy bars of the convolution Ops.

Op-level bar (derived, not tuned).  Every output element of the three Ops is a sum of K products.
A floating-point sum of K products, in any order and with or without FMA, has error at most
gamma_K * sum|a_i b_i| with gamma_K ~ K * eps / 2 (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 3.1).  The bar is twice that, element by element:

    |got - exact| <= K * eps(dtype) * L + tiny(dtype),     L = sum |a_i| |b_i|

``L`` is the same graph evaluated by the reference in float64 on |x|, |w|, |dY|; ``K`` is the
reduction length: (C/G)*kh*kw forward, N*OH*OW for the weight gradient, (O/G)*kh*kw for the image
gradient.  A wrong tap, stride or padding is off by O(1) * L and cannot pass.  float32 results are
judged against ``exact`` (the reference's graph in float64 on the same values); float64 results
against the reference's own float64 output at 2 * K * eps * L, because both carry the bound.

Graph-level bar (a whole training step; no per-element bound survives softmax / log): relative L2
error of each output against ``exact``, capped at 4 x the reference's own float32 relative L2 error
on that output, the cap never below K_max * eps with K_max the longest reduction of the graph.  Both
are float32 accumulations of the same sums in different orders, so they differ by a small factor,
not by orders of magnitude.  float64: against the reference's float64 output at 2 * K_max * eps,
for the same reason as above.  All of these numbers are computed and stored by the generator.
"""
import json
import os

import numpy as np

from aesara_amd.plan import Plan
from golden_inputs import make_input

CONV_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv")
OPS = ("fwd", "gw", "gi")
DTYPES = ("float32", "float64")

# name -> (image (N, C, H, W), kernel (O, C/G, kh, kw), settings)
_DEF = {"border_mode": "valid", "subsample": (1, 1), "filter_dilation": (1, 1), "filter_flip": True,
        "num_groups": 1}
OP_CASES = {
    "a": ((2, 4, 7, 6), (6, 4, 3, 2), {"border_mode": "half"}),
    "b": ((3, 4, 9, 8), (6, 2, 3, 3), {"border_mode": ((1, 0), (2, 1)), "subsample": (2, 1),
                                      "filter_dilation": (2, 1), "num_groups": 2, "filter_flip": False}),
    "c": ((1, 3, 2, 2), (2, 3, 3, 3), {"border_mode": "full"}),
    "d": ((2, 37, 5, 5), (5, 37, 1, 1), {}),
    "e": ((1, 1, 40, 40), (1, 1, 3, 3), {}),
    "f": ((1, 1, 3, 70000), (1, 1, 3, 3), {"border_mode": "half"}),
    "g": ((2, 2, 5, 5), (4, 2, 3, 3), {"subsample": (3, 3)}),
    "h": ((1, 1, 1, 1), (1, 1, 1, 1), {}),
    "a5": ((5, 4, 7, 6), (6, 4, 3, 2), {"border_mode": "half"}),      # case a with N = 5 (chunking)
}


def settings(name):
    return dict(_DEF, **OP_CASES[name][2])


def plan_params(name):
    """The node parameters the lowering gives the three plan ops for a case's settings."""
    s = settings(name)
    bm = s["border_mode"]
    if bm == "valid":
        bm = [[0, 0], [0, 0]]
    elif not isinstance(bm, str):
        bm = [list(p) for p in bm]
    return {"border_mode": bm, "subsample": list(s["subsample"]),
            "filter_dilation": list(s["filter_dilation"]), "filter_flip": s["filter_flip"],
            "num_groups": s["num_groups"]}


def out_hw(name):
    """(OH, OW) of a case: get_conv_shape_1axis (abstract_conv.py:110) on its settings."""
    (_, _, H, W), (_, _, kh, kw), _ = OP_CASES[name]
    s = settings(name)
    out = []
    for size, k, axis in ((H, kh, 0), (W, kw, 1)):
        dil = (k - 1) * s["filter_dilation"][axis] + 1
        bm = s["border_mode"]
        pad = {"valid": (0, 0), "half": (dil // 2,) * 2, "full": (dil - 1,) * 2}[bm] \
            if isinstance(bm, str) else bm[axis]
        out.append((size + pad[0] + pad[1] - dil) // s["subsample"][axis] + 1)
    return tuple(out)


def reduction_lengths(name):
    (N, C, _, _), (O, Cg, kh, kw), _ = OP_CASES[name]
    OH, OW = out_hw(name)
    G = settings(name)["num_groups"]
    return {"fwd": Cg * kh * kw, "gw": N * OH * OW, "gi": (O // G) * kh * kw}


def input_specs(name, dtype):
    """x, w, dy of a case.  Case f holds small integers: its sums are exact and its large fixture
    compresses; what it checks is that every column is reached, not rounding."""
    (N, C, H, W), kshape, _ = OP_CASES[name]
    OH, OW = out_hw(name)
    shapes = {"x": (N, C, H, W), "w": kshape, "dy": (N, kshape[0], OH, OW)}
    if name == "f":
        return {k: {"kind": "randint", "seed": 40 + i, "low": -1, "high": 2, "shape": list(s), "dtype": dtype}
                for i, (k, s) in enumerate(shapes.items())}
    return {k: {"kind": "normal", "seed": 40 + i, "shape": list(s), "dtype": dtype, "scale": 1.0, "shift": 0.0}
            for i, (k, s) in enumerate(shapes.items())}


def op_inputs(op, x, w, dy):
    """Operands of an op-level plan: the third one of a gradient gives only its shape."""
    return {"fwd": [x, w], "gw": [x, dy, w], "gi": [w, dy, x]}[op]


def load_conv_cases():
    with open(os.path.join(CONV_GOLDEN, "cases.json")) as f:
        return json.load(f)["cases"]


def case_plan(c, op=None):
    return Plan.from_json(c["plan"] if op is None else c["plans"][op])


def case_inputs(c):
    return [make_input(s) for s in c["inputs"]]


def case_file(c, op=None):
    return os.path.join(CONV_GOLDEN, c["name"] + ("" if op is None else "_" + op) + ".npz")


def eps(dtype):
    return float(np.finfo(dtype).eps)


def op_bar(dtype, K, L, against_reference=False):
    """Element-wise bound of the module docstring (an array like ``L``)."""
    return (2 if against_reference else 1) * K * eps(dtype) * np.asarray(L, dtype=np.float64) \
        + float(np.finfo(dtype).tiny)


def op_ratio(got, want, dtype, K, L, against_reference=False):
    """max over the elements of |got - want| / bar (<= 1 passes); 0 for an empty result."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want) / op_bar(dtype, K, L, against_reference)))


def rel_l2(got, exact):
    got = np.asarray(got, dtype=np.longdouble)
    exact = np.asarray(exact, dtype=np.longdouble)
    den = np.sqrt(np.sum(exact * exact))
    num = np.sqrt(np.sum((got - exact) ** 2))
    return float(num) if den == 0 else float(num / den)


def graph_cap(c, k):
    """Cap of output ``k`` of a graph-level case (module docstring)."""
    floor = c["K_max"] * eps(c["dtype"])
    if c["dtype"] == "float64":
        return 2 * floor
    return max(4 * c["ref_err"][k], floor)
