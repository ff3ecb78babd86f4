"""Shared by the FFT tests and tools/gen_fft_golden.py: the fixtures under tests/golden/fft and the
accuracy bar of csrc/fft.hip.

The bar is a cap derived from the a-priori bound for Cooley-Tukey transforms (Gentleman & Sande
1966: the relative L2 error of a radix-2 transform of 2^k points grows like k * eps), not a tuned
number: relative L2 error of a whole output <= 8.5 * eps(dtype) * L, where L sums, over every
transformed axis of every FFT node of the plan, log2 of the power-of-two length actually
transformed (at least 1 per axis); a Bluestein axis runs three transforms of m = next_pow2(2n - 1)
points and counts 3 * log2 m.
"""
import json
import os

import numpy as np

from aesara_amd.plan import Plan
from golden_inputs import make_input

FFT_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft")
CAP_FACTOR = 8.5


def load_fft_cases():
    with open(os.path.join(FFT_GOLDEN, "cases.json")) as f:
        return json.load(f)["cases"]


def case_plan(c):
    return Plan.from_json(c["plan"])


def case_inputs(c):
    return [make_input(s) for s in c["inputs"]]


def case_arrays(c, prefix):
    """Stored arrays of a graph-level case: ``out`` (the reference's outputs) or ``exact`` (float32
    cases: the same graph built in float64 on the same inputs)."""
    z = np.load(os.path.join(FFT_GOLDEN, c["name"] + ".npz"))
    return [z[f"{prefix}{k}"] for k in range(c["n_out"])]


def shape_plan(op, dtype, ndim):
    """What ``fft.rfft_op(a, a.shape[1:])`` / ``fft.irfft_op(A, s)`` with the even ``s`` of
    ``fft.irfft`` lower to, ``ndim`` the rank of the real array: ``s`` is ``MakeVector`` of
    ``Shape_i`` values (last entry of the inverse: ``2 * (bins - 1)``), i.e. host integer
    arithmetic, so the plan can be recorded into a launch list."""
    from aesara_amd.plan import Node, Plan, Var
    rank = ndim if op == "rfft" else ndim + 1
    vs = {0: Var(0, dtype, [None] * rank)}
    nodes, dims = [], []
    for d in range(1, ndim):
        vid = len(vs)
        vs[vid] = Var(vid, "int64", [])
        nodes.append(Node("Shape_i", [0], [vid], {"i": d}))
        dims.append(vid)
    if op == "irfft":
        vid = len(vs)
        vs[vid] = Var(vid, "int64", [])
        sc = {"n_in": 1, "nodes": [{"op": "sub", "dtype": "int64", "in": [["i", 0], ["c", 1, "int64"]]},
                                   {"op": "mul", "dtype": "int64", "in": [["t", 0], ["c", 2, "int64"]]}],
              "out": [["t", 1]]}
        nodes.append(Node("Elemwise", [dims[-1]], [vid], {"scalar": sc}))
        dims[-1] = vid
    s, out = len(vs), len(vs) + 1
    vs[s] = Var(s, "int64", [ndim - 1])
    vs[out] = Var(out, dtype, [None] * (ndim + 1 if op == "rfft" else ndim))
    nodes.append(Node("MakeVector", dims, [s], {"dtype": "int64"}))
    nodes.append(Node("RFFT" if op == "rfft" else "IRFFT", [0, s], [out], {}))
    return Plan(f"{op}_from_shape", vs, [0], [out], nodes)


def axis_cost(n):
    """log2 of the power-of-two length transformed for an axis of n points (see module docstring)."""
    if n & (n - 1) == 0:
        return max(1, n.bit_length() - 1)
    m = 1
    while m < 2 * n - 1:
        m *= 2
    return 3 * (m.bit_length() - 1)


def fft_L(s_of_nodes):
    """``s_of_nodes``: the ``s`` vector of every FFT node of a graph (one pass per entry)."""
    return sum(axis_cost(int(n)) for s in s_of_nodes for n in s)


def cap(dtype, L):
    return CAP_FACTOR * float(np.finfo(dtype).eps) * L


def rel_l2(got, exact):
    got = np.asarray(got, dtype=np.longdouble)
    exact = np.asarray(exact, dtype=np.longdouble)
    den = np.sqrt(np.sum(exact * exact))
    num = np.sqrt(np.sum((got - exact) ** 2))
    if den == 0:
        return float(num)
    return float(num / den)
