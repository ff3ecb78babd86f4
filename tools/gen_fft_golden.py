#!/usr/bin/env python
"""Generate the FFT fixtures under tests/golden/fft/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like oracle/gen_golden.py).  Two kinds of
case go into tests/golden/fft/cases.json:

* ``op``: one plan each for ``rfft_op(a, s)`` / ``irfft_op(A, s)`` in float32 and float64 for
  ``a.ndim`` 2, 3 and 4, all shapes symbolic and ``s`` an explicit graph input.  No outputs are
  stored: tests/test_gpu_fft.py drives these plans at many shapes against NumPy evaluated at
  higher precision on the spot.
* ``graph``: ``fft.rfft`` / ``fft.irfft`` with every ``norm``, ``irfft(is_odd=True)``, the round
  trip and the gradients of scalar losses through ``rfft``, ``irfft`` and both, at a few small
  shapes.  Every graph is lowered with the HIP linker's rewrite query and evaluated with the
  reference's ``Mode("cvm", "fast_run")``; its outputs are stored as ``out<k>``.  For float32
  cases the same graph is also built in float64 and evaluated on the same inputs: ``exact<k>``.
  ``L`` of the accuracy bound sums over the ``s`` of every FFT node of the REFERENCE's rewritten graph.

Self-check: the reference's own float32 outputs must meet the accuracy cap of tests/fft_util.py
against the float64 evaluation on every case — if they do not, the case is wrong, not the cap.
(float64 cases are compared with the reference's float64 output itself, at twice the cap.)

Usage:  python tools/gen_fft_golden.py
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
from aesara.tensor import fft  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import fft_util  # noqa: E402
from golden_inputs import make_input  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

REF_MODE = Mode("cvm", "fast_run")
SHAPES = [(2, 4, 8), (3, 5, 6), (2, 7, 10), (1, 1, 2)]
DTYPES = ("float32", "float64")


def T(dtype, ndim, name):
    return TensorType(dtype, shape=(None,) * ndim)(name)


def N(shape, dtype, seed):
    return {"kind": "normal", "seed": seed, "shape": list(shape), "dtype": dtype, "scale": 1.0,
            "shift": 0.0}


def spectrum_shape(shape):
    return tuple(shape[:-1]) + (shape[-1] // 2 + 1, 2)


def op_cases():
    """(name, builder): builder() -> (inputs, outputs)."""
    for dt in DTYPES:
        for nd in (2, 3, 4):
            def mk_r(dt=dt, nd=nd):
                a, s = T(dt, nd, "a"), at.lvector("s")
                return [a, s], [fft.rfft_op(a, s)]

            def mk_i(dt=dt, nd=nd):
                a, s = T(dt, nd + 1, "A"), at.lvector("s")
                return [a, s], [fft.irfft_op(a, s)]
            yield f"op_rfft_{dt}_{nd}d", mk_r
            yield f"op_irfft_{dt}_{nd}d", mk_i


def graph_cases():
    """(name, dtype, builder, input specs): builder(dtype) -> (inputs, outputs); the specs are in
    the case's dtype (the float64 "exact" evaluation casts the same values up)."""
    for dt in DTYPES:
        for shape in SHAPES:
            tag = dt + "_" + "x".join(map(str, shape))
            nd, spec, odd = len(shape), spectrum_shape(shape), bool(shape[-1] % 2)

            def fwd(d, nd=nd):
                x = T(d, nd, "x")
                return [x], [fft.rfft(x), fft.rfft(x, norm="ortho"), fft.rfft(x, norm="no_norm")]

            def inv(d, nd=nd):
                A = T(d, nd + 1, "A")
                return [A], [fft.irfft(A), fft.irfft(A, norm="ortho"), fft.irfft(A, norm="no_norm"),
                             fft.irfft(A, is_odd=True)]

            def rnd(d, nd=nd, odd=odd):
                x = T(d, nd, "x")
                return [x], [fft.irfft(fft.rfft(x), is_odd=odd)]

            def grd(d, nd=nd, odd=odd):
                x, A, G, w = T(d, nd, "x"), T(d, nd + 1, "A"), T(d, nd + 1, "G"), T(d, nd, "w")
                l1 = (fft.rfft(x, norm="ortho") * G).sum()
                l2 = (fft.irfft(A, is_odd=odd) * w).sum()
                l3 = ((fft.irfft(fft.rfft(x, norm="ortho"), norm="ortho", is_odd=odd) ** 2) * w).sum()
                return [x, A, G, w], [ae.grad(l1, x), ae.grad(l2, A), ae.grad(l3, x)]

            yield f"fft_fwd_{tag}", dt, fwd, [N(shape, dt, 1)]
            yield f"fft_inv_{tag}", dt, inv, [N(spec, dt, 2)]
            yield f"fft_round_{tag}", dt, rnd, [N(shape, dt, 3)]
            yield f"fft_grad_{tag}", dt, grd, [N(shape, dt, 4), N(spec, dt, 5), N(spec, dt, 6),
                                               N(shape, dt, 7)]


def lower(ins, outs, name):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore",
                    accept_inplace=True)
    plan = f.maker.linker.plan
    plan.name = name
    return plan


def reference_outputs(ins, outs, xs):
    """(outputs, ``s`` of every RFFTOp / IRFFTOp node of the reference's own rewritten graph): the
    accuracy bound is derived from the reference's graph, not from the code under test."""
    f = ae.function(ins, outs, mode=REF_MODE, on_unused_input="ignore", accept_inplace=True)
    ffts = [n for n in f.maker.fgraph.toposort() if isinstance(n.op, (fft.RFFTOp, fft.IRFFTOp))]
    g = ae.function(ins, [n.inputs[1] for n in ffts], mode=Mode("py", None), on_unused_input="ignore",
                    accept_inplace=True)
    return [np.asarray(o) for o in f(*xs)], [[int(v) for v in s] for s in g(*xs)]


def main():
    os.makedirs(fft_util.FFT_GOLDEN, exist_ok=True)
    cases = []
    for name, mk in op_cases():
        ins, outs = mk()
        plan = lower(ins, outs, name)
        assert [n.op for n in plan.nodes] in (["RFFT"], ["IRFFT"]), plan.pretty()
        cases.append({"name": name, "kind": "op", "plan": plan.to_json()})
        print(f"[ok] {name}")
    worst = 0.0
    for name, dt, mk, specs in graph_cases():
        ins, outs = mk(dt)
        xs = [make_input(s) for s in specs]
        plan = lower(ins, outs, name)
        ref, s_of_nodes = reference_outputs(ins, outs, xs)
        assert all(o.dtype == np.dtype(dt) for o in ref), [o.dtype for o in ref]
        n_fft = sum(n.op in ("RFFT", "IRFFT") for n in plan.nodes)
        assert n_fft == len(s_of_nodes), (name, n_fft, s_of_nodes)     # same FFT nodes as the reference
        L = fft_util.fft_L(s_of_nodes)
        arrays = {f"out{k}": r for k, r in enumerate(ref)}
        if dt == "float32":
            ins64, outs64 = mk("float64")
            exact, _ = reference_outputs(ins64, outs64, [x.astype("float64") for x in xs])
            for k, (r, e) in enumerate(zip(ref, exact)):
                err, bound = fft_util.rel_l2(r, e), fft_util.cap(dt, L)
                worst = max(worst, err / bound)
                assert err <= bound, f"{name} output {k}: the reference misses the cap: {err} > {bound}"
                arrays[f"exact{k}"] = e
        np.savez_compressed(os.path.join(fft_util.FFT_GOLDEN, name + ".npz"), **arrays)
        cases.append({"name": name, "kind": "graph", "dtype": dt, "plan": plan.to_json(),
                      "inputs": specs, "n_out": len(ref), "L": L})
        print(f"[ok] {name}: {len(plan.nodes)} nodes, L = {L}")
    with open(os.path.join(fft_util.FFT_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_fft_golden.py", "ref_mode": "Mode('cvm','fast_run')",
                   "cases": cases}, f)
    print(f"{len(cases)} cases written; reference float32 error at most {worst:.3f} of the cap")


if __name__ == "__main__":
    main()
