#!/usr/bin/env python
"""Generate the convolution fixtures under tests/golden/conv/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like tools/gen_fft_golden.py).  Every graph
is built with the reference, rewritten with the HIP linker's query and evaluated with the
reference's ``Mode("py", HIP_QUERY)``: the abstract convolution Ops' own ``perform`` (SciPy's
``convolve2d``) — the compiled CorrMM / ConvOp path is broken at the reference's revision (see
linker.HIP_QUERY).  Two kinds of case go into tests/golden/conv/cases.json:

* ``op``: the cases of tests/conv_util.OP_CASES, each in float32 and float64, with one plan per Op
  (``fwd`` AbstractConv2d, ``gw`` AbstractConv2d_gradWeights, ``gi`` AbstractConv2d_gradInputs; the
  ``shape`` operand of a gradient is taken from the shape of a third input, as ``aesara.grad``
  builds it).  Per Op one file with ``out`` (the reference's output), ``exact`` (float32 cases:
  the same graph in float64 on the same values) and ``L`` (the float64 graph on |x|, |w|, |dY|);
  the reduction length K goes into cases.json.
* ``graph``: a CNN training step (conv + bias + relu, strided conv + relu, dense layer, softmax
  cross-entropy; outputs: the loss and the gradients of both kernels, the bias, the dense weight
  and the image) and a second one with ``filter_flip=False``, two groups and dilation (2, 2); with
  ``out<k>``, ``exact<k>``, the reference's own float32 relative L2 error ``ref_err`` and the
  longest reduction ``K_max``.

Self-check: every stored reference output must be inside the op-level bar of tests/conv_util.py;
a case that is not is refused (nothing is written).

Usage:  python tools/gen_conv_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_overlay  # noqa: E402

ae = ref_overlay.import_reference()
import aesara.tensor as at  # noqa: E402
from aesara.compile.mode import Mode  # noqa: E402
from aesara.tensor.nnet import abstract_conv as ac  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import conv_util  # noqa: E402
from golden_inputs import make_input  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

REF_MODE = Mode("py", HIP_QUERY)
CONV_OPS = (ac.AbstractConv2d, ac.AbstractConv2d_gradWeights, ac.AbstractConv2d_gradInputs)


def T4(dtype, name):
    return TensorType(dtype, shape=(None,) * 4)(name)


def op_graph(op, dtype, s):
    """(inputs, [output]) of one Op with the settings ``s`` (conv_util.settings)."""
    x, w, dy = T4(dtype, "x"), T4(dtype, "w"), T4(dtype, "dy")
    kw = dict(border_mode=s["border_mode"], subsample=s["subsample"], filter_flip=s["filter_flip"],
              filter_dilation=s["filter_dilation"], num_groups=s["num_groups"])
    if op == "fwd":
        return [x, w], [ac.AbstractConv2d(**kw)(x, w)]
    if op == "gw":
        return [x, dy, w], [ac.AbstractConv2d_gradWeights(**kw)(x, dy, w.shape[2:])]
    return [w, dy, x], [ac.AbstractConv2d_gradInputs(**kw)(w, dy, x.shape[2:])]


def cnn(dtype, variant):
    """The training step of the graph-level cases: (inputs, outputs, input specs)."""
    second = variant == "grouped"
    C = 4 if second else 3
    kw1 = dict(border_mode="half")
    kw2 = dict(border_mode="valid", subsample=(2, 2))
    if second:
        kw1.update(filter_flip=False, num_groups=2, filter_dilation=(2, 2))
        kw2.update(filter_flip=False, num_groups=2)
    x, w1, w2 = T4(dtype, "x"), T4(dtype, "w1"), T4(dtype, "w2")
    b1 = TensorType(dtype, shape=(None,))("b1")
    wd = TensorType(dtype, shape=(None, None))("wd")
    y = at.lvector("y")
    h1 = at.nnet.relu(ac.conv2d(x, w1, **kw1) + b1.dimshuffle("x", 0, "x", "x"))
    h2 = at.nnet.relu(ac.conv2d(h1, w2, **kw2))
    p = at.nnet.softmax(at.dot(h2.flatten(2), wd))
    loss = at.nnet.categorical_crossentropy(p, y).mean()
    outs = [loss] + ae.grad(loss, [w1, w2, b1, wd, x])

    def N(shape, seed, scale=1.0):
        return {"kind": "normal", "seed": seed, "shape": list(shape), "dtype": dtype, "scale": scale,
                "shift": 0.0}
    specs = [N((4, C, 12, 12), 1), N((8, C // (2 if second else 1), 3, 3), 2, 0.3),
             N((8, 8 // (2 if second else 1), 3, 3), 3, 0.2), N((8,), 4, 0.1), N((200, 5), 5, 0.1),
             {"kind": "randint", "seed": 6, "low": 0, "high": 5, "shape": [4], "dtype": "int64"}]
    return [x, w1, w2, b1, wd, y], outs, specs


def lower(ins, outs, name):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore",
                    accept_inplace=True)
    plan = f.maker.linker.plan
    plan.name = name
    return plan


def reference(ins, outs):
    return ae.function(ins, outs, mode=REF_MODE, on_unused_input="ignore", accept_inplace=True)


def longest_reduction(f, xs):
    """K_max of a compiled reference function: over its convolution nodes (forward (C/G)*kh*kw,
    weight gradient N*OH*OW, image gradient (O/G)*kh*kw) and its matrix products (inner size)."""
    from aesara.tensor.blas import Dot22, Dot22Scalar, Gemm
    from aesara.tensor.math import Dot
    want, kinds = [], []
    for n in f.maker.fgraph.toposort():
        if isinstance(n.op, CONV_OPS):
            want += [n.inputs[0].shape, n.inputs[1].shape, n.outputs[0].shape]
            kinds.append(n.op)
        elif isinstance(n.op, (Dot22, Dot22Scalar, Dot)):
            want += [n.inputs[0].shape, n.inputs[1].shape, n.outputs[0].shape]
            kinds.append("dot")
        elif isinstance(n.op, Gemm):
            want += [n.inputs[2].shape, n.inputs[3].shape, n.outputs[0].shape]
            kinds.append("dot")
    g = ae.function(f.maker.fgraph.inputs, want, mode=Mode("py", None), on_unused_input="ignore")
    shapes = [tuple(int(v) for v in s) for s in g(*xs)]
    ks = []
    for i, kind in enumerate(kinds):
        a, b, o = shapes[3 * i:3 * i + 3]
        if kind == "dot":
            ks.append(a[-1])
        elif isinstance(kind, ac.AbstractConv2d):
            ks.append(b[1] * b[2] * b[3])
        elif isinstance(kind, ac.AbstractConv2d_gradWeights):
            ks.append(b[0] * b[2] * b[3])                      # topgrad: N * OH * OW
        else:
            ks.append((a[0] // kind.num_groups) * a[2] * a[3])   # kern: (O/G) * kh * kw
    return max(ks)


def main():
    os.makedirs(conv_util.CONV_GOLDEN, exist_ok=True)
    cases, files, worst = [], {}, 0.0
    for name in conv_util.OP_CASES:
        s = conv_util.settings(name)
        Ks = conv_util.reduction_lengths(name)
        for dt in conv_util.DTYPES:
            specs = conv_util.input_specs(name, dt)
            v = {k: make_input(sp) for k, sp in specs.items()}
            v64 = {k: a.astype("float64") for k, a in v.items()}
            c = {"name": f"op_{name}_{dt}", "kind": "op", "case": name, "dtype": dt, "specs": specs,
                 "K": Ks, "plans": {}}
            for op in conv_util.OPS:
                ins, outs = op_graph(op, dt, s)
                plan = lower(ins, outs, f"{c['name']}_{op}")
                want_op = {"fwd": "Conv2d", "gw": "Conv2dGradW", "gi": "Conv2dGradI"}[op]
                assert [n.op for n in plan.nodes].count(want_op) == 1 and plan.nodes[-1].op == want_op, \
                    plan.pretty()
                c["plans"][op] = plan.to_json()
                (out,) = reference(ins, outs)(*conv_util.op_inputs(op, v["x"], v["w"], v["dy"]))
                f64 = reference(*op_graph(op, "float64", s))
                (exact,) = f64(*conv_util.op_inputs(op, v64["x"], v64["w"], v64["dy"]))
                (L,) = f64(*conv_util.op_inputs(op, *(np.abs(v64[k]) for k in ("x", "w", "dy"))))
                out, exact, L = np.asarray(out), np.asarray(exact), np.asarray(L)
                assert out.dtype == np.dtype(dt) and exact.dtype == np.float64 and L.dtype == np.float64
                ratio = conv_util.op_ratio(out, exact, dt, Ks[op], L)
                if dt == "float32":
                    worst = max(worst, ratio)
                if not ratio <= 1.0:
                    raise SystemExit(f"{c['name']} {op}: the reference itself is at {ratio:.3f} of the "
                                     "bar — case refused, nothing written")
                arrays = {"out": out, "L": L}
                if dt == "float32":
                    arrays["exact"] = exact
                files[conv_util.case_file(c, op)] = arrays
                print(f"[ok] {c['name']} {op}: K = {Ks[op]}, reference at {ratio:.3f} of the bar")
            cases.append(c)
    for variant in ("plain", "grouped"):
        for dt in conv_util.DTYPES:
            name = f"cnn_{variant}_{dt}"
            ins, outs, specs = cnn(dt, variant)
            xs = [make_input(sp) for sp in specs]
            plan = lower(ins, outs, name)
            ops = [n.op for n in plan.nodes]
            assert ops.count("Conv2d") == 2 and ops.count("Conv2dGradW") == 2 and ops.count("Conv2dGradI") == 2, ops
            f = reference(ins, outs)
            ref = [np.asarray(o) for o in f(*xs)]
            assert all(o.dtype == np.dtype(dt) for o in ref), [o.dtype for o in ref]
            c = {"name": name, "kind": "graph", "dtype": dt, "plan": plan.to_json(), "inputs": specs,
                 "n_out": len(ref), "K_max": longest_reduction(f, xs)}
            arrays = {f"out{k}": r for k, r in enumerate(ref)}
            if dt == "float32":
                ins64, outs64, _ = cnn("float64", variant)
                exact = reference(ins64, outs64)(*[x.astype("float64") if x.dtype.kind == "f" else x
                                                   for x in xs])
                c["ref_err"] = [conv_util.rel_l2(r, e) for r, e in zip(ref, exact)]
                arrays.update({f"exact{k}": np.asarray(e) for k, e in enumerate(exact)})
            files[conv_util.case_file(c)] = arrays
            cases.append(c)
            print(f"[ok] {name}: {len(plan.nodes)} nodes, K_max = {c['K_max']}, "
                  f"ref_err = {c.get('ref_err')}")
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
    with open(os.path.join(conv_util.CONV_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_conv_golden.py", "ref_mode": "Mode('py', HIP_QUERY)",
                   "cases": cases}, f)
    print(f"{len(cases)} cases written; reference float32 outputs at most {worst:.3f} of the op-level bar")


if __name__ == "__main__":
    main()
