#!/usr/bin/env python
"""Generate the pooling fixtures under tests/golden/pool/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like tools/gen_conv_golden.py).  Every graph
is built with the reference, rewritten with the HIP linker's query and evaluated twice: with the
reference's C linker (what a user of the reference gets by default; its windows are the contract) and
with ``Mode("py", HIP_QUERY)`` (the Ops' ``perform``).  Two kinds of case go into
tests/golden/pool/cases.json:

* ``op``: the cases of tests/pool_util.OP_CASES, each in float32 and float64, for every op key of
  pool_util.OPS (``Pool`` per mode, ``MaxPoolGrad``, ``AveragePoolGrad`` per mode,
  ``DownsampleFactorMaxGradGrad``; ``maxout`` is the stored forward result; the one-node plans are
  pool_util.op_plan, and the linker's lowering is held to them).  One file per case with
  ``<op>_out`` (the C linker's output) and, for the ops judged against a bar, ``<op>_exact`` (float32
  cases: the same graph in float64 on the same values) and ``<op>_L`` (the float64 graph on absolute
  values).  ``perform_agrees`` in cases.json says per op whether ``perform`` gave the same bits.  For
  the exact ops (``max`` forward, ``MaxPoolGrad``, grad-of-grad) a case whose two implementations
  differ is refused, with two documented exceptions: the tie-with-padding cases
  (pool_util.TIE_WITH_PADDING: ``MaxPoolGrad.perform`` shifts its windows) and the ``max`` forward of
  the NaN case, where ``perform`` (``np.max``: NaN wins) is what is stored and the C loop may differ.
  A ``MaxPoolGrad`` case outside those that differs in the last bit is listed under ``inexact`` and
  judged against the bar with ``L`` = |reference output| (none is expected; it is printed).
* ``graph``: two CNN training steps with pooling layers (outputs: the loss and the gradients of both
  kernels, the bias, the dense weight and the image), ``max_pool_2d_same_size``, a Hessian-vector
  product of a max pool (reaches ``DownsampleFactorMaxGradGrad`` through ``aesara.grad``) and the
  losses of ten SGD steps of the first CNN; with ``out<k>``, ``exact<k>``, the reference's own
  float32 relative L2 error ``ref_err`` and the longest reduction ``K_max``.

Self-check: every stored reference output of a bar op must be inside the bar of tests/pool_util.py,
and so must ``perform``; a case that is not is refused (nothing is written).

Usage:  python tools/gen_pool_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_overlay  # noqa: E402

ae = ref_overlay.import_reference()
import aesara.tensor as at  # noqa: E402
from aesara.compile.mode import Mode  # noqa: E402
from aesara.tensor.nnet import abstract_conv as ac  # noqa: E402
from aesara.tensor.signal import pool as rp  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import pool_util  # noqa: E402
from golden_inputs import make_input  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

C_MODE = Mode("c", HIP_QUERY)            # op cases: every pooling Op has C code
CPY_MODE = Mode("c|py", HIP_QUERY)       # graphs: C where an Op has it (the pooling Ops), else perform
PY_MODE = Mode("py", HIP_QUERY)
SGD_STEPS, SGD_RATE = 10, 0.1


def T(dtype, ndim, name):
    return TensorType(dtype, shape=(None,) * ndim)(name)


def op_graph(name, op, dtype, symbolic=False):
    """(inputs, [output]) of one op key on the settings of a case."""
    shape, ws, stride, pad, ib, _ = pool_util.OP_CASES[name]
    nd, n = len(ws), len(shape)
    x, maxout, gz, ggx = (T(dtype, n, k) for k in ("x", "maxout", "gz", "ggx"))
    geo = [at.lvector(k) for k in ("ws", "stride", "pad")] if symbolic else [ws, stride, pad]
    mode = pool_util.op_mode(op)
    if op.startswith("fwd_"):
        ins, out = [x], rp.Pool(ignore_border=ib, mode=mode, ndim=nd)(x, *geo)
    elif op == "maxgrad":
        ins, out = [x, maxout, gz], rp.MaxPoolGrad(ignore_border=ib, ndim=nd)(x, maxout, gz, *geo)
    elif op.startswith("avggrad_"):
        ins, out = [x, gz], rp.AveragePoolGrad(ignore_border=ib, mode=mode, ndim=nd)(x, gz, *geo)
    else:
        ins, out = [x, maxout, ggx], rp.DownsampleFactorMaxGradGrad(ignore_border=ib, ndim=nd)(
            x, maxout, ggx, *geo)
    return ins + (geo if symbolic else []), [out]


def cnn(dtype, variant):
    """The training step of the graph-level cases: (inputs, outputs, input specs)."""
    padded = variant == "padded"
    x, w1, w2 = (T(dtype, 4, k) for k in ("x", "w1", "w2"))
    b1, wd, y = T(dtype, 1, "b1"), T(dtype, 2, "wd"), at.lvector("y")
    loss = cnn_loss(x, w1, w2, b1, wd, y, padded)
    outs = [loss] + ae.grad(loss, [w1, w2, b1, wd, x])
    return [x, w1, w2, b1, wd, y], outs, cnn_specs(dtype, padded)


def cnn_loss(x, w1, w2, b1, wd, y, padded):
    h1 = at.nnet.relu(ac.conv2d(x, w1, border_mode="half") + b1.dimshuffle("x", 0, "x", "x"))
    p1 = rp.pool_2d(h1, (2, 2), ignore_border=True, mode="max", pad=(1, 1) if padded else (0, 0))
    h2 = at.nnet.relu(ac.conv2d(p1, w2, border_mode="valid"))
    if padded:
        p2 = rp.pool_2d(h2, (3, 3), ignore_border=True, stride=(2, 2), pad=(1, 1), mode="average_inc_pad")
    else:
        p2 = rp.pool_2d(h2, (3, 3), ignore_border=True, stride=(2, 2), mode="average_exc_pad")
    p = at.nnet.softmax(at.dot(p2.flatten(2), wd))
    return at.nnet.categorical_crossentropy(p, y).mean()


def cnn_specs(dtype, padded):
    def N(shape, seed, scale=1.0):
        return {"kind": "normal", "seed": seed, "shape": list(shape), "dtype": dtype, "scale": scale,
                "shift": 0.0}
    # 16 x 16 -> pool -> 8 (9 padded) -> valid conv -> 6 (7) -> pool -> 2 (4)
    feats = 8 * (16 if padded else 4)
    return [N((4, 3, 16, 16), 1), N((8, 3, 3, 3), 2, 0.3), N((8, 8, 3, 3), 3, 0.2), N((8,), 4, 0.1),
            N((feats, 5), 5, 0.1),
            {"kind": "randint", "seed": 6, "low": 0, "high": 5, "shape": [4], "dtype": "int64"}]


def same_size(dtype):
    x = T(dtype, 4, "x")
    spec = {"kind": "normal", "seed": 11, "shape": [2, 3, 6, 6], "dtype": dtype, "scale": 1.0, "shift": 0.0}
    return [x], [rp.max_pool_2d_same_size(x, (2, 2))], [spec]


def hvp(dtype):
    x, v = T(dtype, 4, "x"), T(dtype, 4, "v")
    g = ae.grad((rp.pool_2d(x, (3, 3), ignore_border=True, stride=(2, 2)) ** 2).sum(), x)
    specs = [{"kind": "normal", "seed": 12 + i, "shape": [2, 3, 7, 7], "dtype": dtype, "scale": 1.0,
              "shift": 0.0} for i in range(2)]
    return [x, v], [ae.grad((g * v).sum(), x)], specs


def sgd_function(dtype, mode):
    """(function (x, y) -> loss with the SGD updates of the plain CNN on shared variables, the
    shared variables, the input specs of x and y)."""
    specs = cnn_specs(dtype, False)
    x, y = T(dtype, 4, "x"), at.lvector("y")
    params = [ae.shared(make_input(s), name=n) for n, s in zip(("w1", "w2", "b1", "wd"), specs[1:5])]
    w1, w2, b1, wd = params
    loss = cnn_loss(x, w1, w2, b1, wd, y, False)
    rate = np.asarray(SGD_RATE, dtype)
    updates = [(p, p - rate * g) for p, g in zip(params, ae.grad(loss, params))]
    return ae.function([x, y], loss, updates=updates, mode=mode), params, [specs[0], specs[5]]


GRAPHS = {"cnn_plain": lambda dt: cnn(dt, "plain"), "cnn_padded": lambda dt: cnn(dt, "padded"),
          "same_size": same_size, "hvp": hvp}
GRAPH_OPS = {"cnn_plain": {"Pool": 2, "MaxPoolGrad": 1, "AvgPoolGrad": 1},
             "cnn_padded": {"Pool": 2, "MaxPoolGrad": 1, "AvgPoolGrad": 1},
             "same_size": {"Pool": 1, "MaxPoolGrad": 1},
             "hvp": {"MaxPoolGradGrad": 1}}


def lower(ins, outs, name):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore",
                    accept_inplace=True)
    plan = f.maker.linker.plan
    plan.name = name
    return plan


def reference(ins, outs, mode=C_MODE):
    return ae.function(ins, outs, mode=mode, on_unused_input="ignore", accept_inplace=True)


def longest_reduction(f, xs, default):
    import gen_conv_golden
    try:
        return max(default, gen_conv_golden.longest_reduction(f, xs))
    except ValueError:            # no convolution and no product in the graph
        return default


def geo_values(name):
    return [np.asarray(v, "int64") for v in pool_util.OP_CASES[name][1:4]]


def op_case(name, dt):
    """(cases.json entry, arrays) of one op case in one dtype."""
    v = pool_util.case_values(name, dt)
    v64 = {k: a.astype("float64") for k, a in v.items()}
    c = {"name": f"op_{name}_{dt}", "kind": "op", "case": name, "dtype": dt, "perform_agrees": {},
         "raises": [], "inexact": []}
    arrays = {}
    for op in pool_util.case_ops(name):
        want_op, operands = pool_util.OPS[op]
        ins, outs = op_graph(name, op, dt)
        plan = lower(ins, outs, f"{c['name']}_{op}")
        assert pool_util.same_lowering(plan, pool_util.op_plan(name, op, dt)), plan.pretty()
        K = pool_util.reduction_length(name, op)

        def args(vals):
            return [arrays["fwd_max_out"].astype(vals["x"].dtype) if k == "maxout" else vals[k]
                    for k in operands]
        if pool_util.raises(name, op):
            for mode in (C_MODE, PY_MODE):
                try:
                    reference(ins, outs, mode)(*args(v))
                except (ValueError, NotImplementedError):
                    continue
                raise SystemExit(f"{c['name']} {op}: the reference did not raise")
            c["raises"].append(op)
            print(f"[ok] {c['name']} {op}: the reference raises")
            continue
        (out,) = reference(ins, outs)(*args(v))
        (py,) = reference(ins, outs, PY_MODE)(*args(v))
        out, py = np.array(out), np.array(py)
        assert out.dtype == np.dtype(dt) and out.shape == py.shape, (out.dtype, out.shape, py.shape)
        agrees = pool_util.same_bits(out, py)
        c["perform_agrees"][op] = agrees
        if op in pool_util.EXACT_OPS:
            if name == "n" and op == "fwd_max":
                out = py                                   # np.max: a NaN in the window wins
                assert np.isnan(out[0, 0, 0, 0]) and np.isnan(out[1, 2, 1, 1]) and np.isnan(out).sum() == 2
            elif not agrees:
                if op == "maxgrad" and name in pool_util.TIE_WITH_PADDING:
                    print(f"[note] {c['name']} {op}: perform differs (shifted windows), the C result is stored")
                elif op == "maxgrad" and np.allclose(out, py, rtol=4 * pool_util.eps(dt), atol=0):
                    c["inexact"].append(op)
                    arrays[f"{op}_L"] = np.abs(out.astype("float64"))
                    print(f"[INEXACT] {c['name']} {op}: C and perform differ in the last bit")
                else:
                    raise SystemExit(f"{c['name']} {op}: C and perform differ — case refused")
            arrays[f"{op}_out"] = out
            print(f"[ok] {c['name']} {op}: exact, perform agrees: {agrees}")
            continue
        f64 = reference(*op_graph(name, op, "float64"))
        data = "x" if op.startswith("fwd_") else "gz"
        (exact,) = f64(*[v64[k] for k in operands])
        (L,) = f64(*[np.abs(v64[k]) if k == data else v64[k] for k in operands])
        exact, L = np.array(exact), np.array(L)
        assert exact.dtype == np.float64 and L.dtype == np.float64
        for what, r in (("the reference", out), ("perform", py)):
            ratio = pool_util.op_ratio(r, exact, dt, K, L)
            if not ratio <= 1.0:
                raise SystemExit(f"{c['name']} {op}: {what} itself is at {ratio:.3f} of the bar — "
                                 "case refused, nothing written")
        arrays[f"{op}_out"], arrays[f"{op}_L"] = out, L
        if dt == "float32":
            arrays[f"{op}_exact"] = exact
        print(f"[ok] {c['name']} {op}: K = {K}, reference at "
              f"{pool_util.op_ratio(out, exact, dt, K, L):.3f} of the bar, perform agrees: {agrees}")
    return c, arrays


def graph_case(gname, dt):
    name = f"{gname}_{dt}"
    ins, outs, specs = GRAPHS[gname](dt)
    xs = [make_input(sp) for sp in specs]
    plan = lower(ins, outs, name)
    ops = [n.op for n in plan.nodes]
    for k, n in GRAPH_OPS[gname].items():
        assert ops.count(k) >= n, (name, k, ops)
    mode = CPY_MODE
    try:
        f = reference(ins, outs, mode)
    except ValueError as e:
        # the reference's C linker cannot instantiate MaxPoolGrad in the Hessian-vector graph
        # ("expected an ndarray, not None"); its perform has the C windows wherever pad == 0 (the
        # op cases above check that bit for bit), which holds for every graph without padding
        assert gname in ("hvp", "same_size"), (name, e)
        mode = PY_MODE
        f = reference(ins, outs, mode)
        print(f"[note] {name}: evaluated with perform ({str(e).splitlines()[-1]})")
    ref = [np.array(o) for o in f(*xs)]
    assert all(o.dtype == np.dtype(dt) for o in ref), [o.dtype for o in ref]
    c = {"name": name, "kind": "graph", "graph": gname, "dtype": dt, "inputs": specs, "n_out": len(ref), "K_max": longest_reduction(f, xs, 9),
         "ref_linker": "py" if mode is PY_MODE else "c|py"}
    arrays = {f"out{k}": r for k, r in enumerate(ref)}
    if dt == "float32":
        ins64, outs64, _ = GRAPHS[gname]("float64")
        exact = reference(ins64, outs64, mode)(*[x.astype("float64") if x.dtype.kind == "f" else x
                                                     for x in xs])
        c["ref_err"] = [pool_util.rel_l2(r, e) for r, e in zip(ref, exact)]
        arrays.update({f"exact{k}": np.array(e) for k, e in enumerate(exact)})
    print(f"[ok] {name}: {len(plan.nodes)} nodes, K_max = {c['K_max']}, ref_err = {c.get('ref_err')}")
    return c, arrays


def sgd_losses(dtype, mode=CPY_MODE, cast=None):
    f, _, specs = sgd_function(dtype, mode)
    x, y = (make_input(s) for s in specs)
    if cast:
        x = x.astype(cast)
    return np.array([f(x, y) for _ in range(SGD_STEPS)])


def sgd_case(dt, k_max):
    """The losses of SGD_STEPS steps: one output (the sequence); float32 ``exact`` is the float64
    run from the float32 starting values."""
    name = f"sgd_{dt}"
    ref = sgd_losses(dt)
    assert ref.dtype == np.dtype(dt) and ref[-1] < ref[0], ref
    c = {"name": name, "kind": "sgd", "dtype": dt, "steps": SGD_STEPS, "rate": SGD_RATE, "n_out": 1,
         "K_max": k_max}
    arrays = {"out0": ref}
    if dt == "float32":
        f, params, specs = sgd_function("float64", CPY_MODE)
        for p, s in zip(params, cnn_specs("float32", False)[1:5]):
            p.set_value(make_input(s).astype("float64"))
        x, y = make_input(dict(specs[0], dtype="float32")).astype("float64"), make_input(specs[1])
        exact = np.array([f(x, y) for _ in range(SGD_STEPS)])
        c["ref_err"] = [pool_util.rel_l2(ref, exact)]
        arrays["exact0"] = exact
    print(f"[ok] {name}: losses {ref[0]:.4f} -> {ref[-1]:.4f}, ref_err = {c.get('ref_err')}")
    return c, arrays


def main():
    os.makedirs(pool_util.POOL_GOLDEN, exist_ok=True)
    cases, files = [], {}
    for name in pool_util.OP_CASES:
        for dt in pool_util.DTYPES:
            c, arrays = op_case(name, dt)
            cases.append(c)
            files[pool_util.case_file(c)] = arrays
    for dt in pool_util.DTYPES:
        k_max = None
        for gname in GRAPHS:
            c, arrays = graph_case(gname, dt)
            cases.append(c)
            files[pool_util.case_file(c)] = arrays
            if gname == "cnn_plain":
                k_max = c["K_max"]
        c, arrays = sgd_case(dt, k_max)
        cases.append(c)
        files[pool_util.case_file(c)] = arrays
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
    with open(os.path.join(pool_util.POOL_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_pool_golden.py",
                   "ref_mode": "Mode('c', HIP_QUERY) (graphs: 'c|py'), checked against Mode('py', HIP_QUERY)",
                   "cases": cases}, f)
    inexact = [(c["name"], op) for c in cases for op in c.get("inexact", ())]
    print(f"{len(cases)} cases written; MaxPoolGrad cases off the exact list: {inexact or 'none'}")


if __name__ == "__main__":
    main()
