#!/usr/bin/env python
"""Generate the sparse fixtures under tests/golden/sparse/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like tools/gen_linalg_golden.py).  Every case
of tests/sparse_util.CASES, in float32 and float64, is built with the reference, rewritten with the
HIP linker's query and evaluated with ``Mode("py", HIP_QUERY)`` — the Ops' own ``perform`` (SciPy).
The plans are sparse_util.op_plan, and the linker's lowering is held to them.

One file per case and dtype: the inputs (the sparse operand as ``data`` / ``indices`` / ``indptr`` /
``shape``, dense operands as ``dense0``, ``dense1``), ``out`` — the reference's output in the case's
dtype (``data`` of a sparse output; ``out_indices`` / ``out_indptr`` / ``out_shape`` next to it) — and
``x64``, the same graph in float64 on the same values.

Self-check: the reference's own output must be inside every bar of tests/sparse_util.py; a case that
is not is refused (nothing is written).

Usage:  python tools/gen_sparse_golden.py
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
import aesara.sparse as sp  # noqa: E402
from aesara.compile.mode import Mode  # noqa: E402
from aesara.sparse import basic as S  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import sparse_util  # noqa: E402
from sparse_util import CASES  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

PY_MODE = Mode("py", HIP_QUERY)


def T(dtype, ndim, name):
    return TensorType(dtype, shape=(None,) * ndim)(name)


def op_graph(name, dtype, all64=False):
    """(inputs, [output]) of a case; the sparse operand comes first.  ``all64``: every operand in
    float64 (the exact evaluation of a mixed case)."""
    c = CASES[name]
    op, fmt, n = c["op"], c["format"], c["n"]
    sdt, odt = sparse_util.data_dtype(name, dtype), sparse_util.out_dtype(name, dtype)
    if all64:
        sdt = odt = "float64"
    if op == "sfd":
        w = T(odt, 2, "w")
        return [w], [(sp.csr_from_dense if fmt == "csr" else sp.csc_from_dense)(w)]
    x = (sp.csr_matrix if fmt == "csr" else sp.csc_matrix)("x", sdt)
    if op in ("sdot", "dot", "dotr"):
        w = T(odt, 1 if n == "vec" else 2, "w")
        if op == "sdot":
            return [x, w], [sp.structured_dot(x, w.T if c.get("bt") else w)]
        return [x, w], [S._dot(x, w) if op == "dot" else S._dot(w, x)]
    if op == "sdg":
        b, g = T(odt, 2, "b"), T(odt, 2, "g")
        sdg = S.sdg_csr if fmt == "csr" else S.sdg_csc
        return [x, b, g], [sdg(sp.csm_indices(x), sp.csm_indptr(x), b, g)]
    if op == "dfs":
        return [x], [sp.dense_from_sparse(x)]
    if op == "sum":
        return [x], [sp.sp_sum(x, axis=c["axis"])]
    if op == "mul":
        y = T(odt, 2, "y")
        return [x, y], [S.mul_s_d(x, y)]
    raise KeyError(op)


def lower(ins, outs, name):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore", accept_inplace=True)
    plan = f.maker.linker.plan
    plan.name = name
    return plan


def reference(ins, outs):
    return ae.function(ins, outs, mode=PY_MODE, on_unused_input="ignore", accept_inplace=True)


def graph_args(name, xs, dtype=None):
    """The reference function's arguments from the plan inputs ``xs`` (``dtype``: cast the floats)."""
    def fl(a):
        return a if dtype is None else a.astype(dtype)
    if CASES[name]["op"] == "sfd":
        return [fl(xs[0])]
    m = sparse_util.to_scipy(xs[:5], CASES[name]["format"], dtype)
    return [m] + [fl(a) for a in xs[5:]]


def members(out):
    """(float output, extra arrays) of a reference result."""
    if hasattr(out, "indptr"):
        return np.array(out.data), {"out_indices": np.array(out.indices), "out_indptr": np.array(out.indptr),
                                    "out_shape": np.array(out.shape, "int64")}
    return np.array(out), {}


def case(name, dt):
    assert sparse_util.same_lowering(lower(*op_graph(name, dt), f"sparse_{name}_{dt}"),
                                     sparse_util.op_plan(name, dt)), name
    xs = sparse_util.operands(name, dt)
    (out,) = reference(*op_graph(name, dt))(*graph_args(name, xs))
    (x64,) = reference(*op_graph(name, dt, all64=True))(*graph_args(name, xs, "float64"))
    out, extra = members(out)
    x64, _ = members(x64)
    odt = sparse_util.out_dtype(name, dt)
    assert out.dtype == np.dtype(odt), (name, out.dtype)
    if "out_indices" in extra:
        assert extra["out_indices"].dtype == np.int32 and extra["out_indptr"].dtype == np.int32, name
    arrays = dict(sparse_util.store_inputs(xs), out=out, x64=x64, **extra)
    r = sparse_util.ratio(name, dt, out, xs, arrays)
    if not r <= 1.0:
        raise SystemExit(f"{name} {dt}: the reference itself is at {r} of its bar — case refused, nothing written")
    print(f"[ok] {name} {dt}: reference at {r:.3f} of the bar")
    return {"name": name, "dtype": dt, "op": CASES[name]["op"], "ref_ratio": r}, arrays


def main():
    os.makedirs(sparse_util.SPARSE_GOLDEN, exist_ok=True)
    cases, files = [], {}
    for name in CASES:
        for dt in sparse_util.case_dtypes(name):
            entry, arrays = case(name, dt)
            cases.append(entry)
            files[sparse_util.case_file(name, dt)] = arrays
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
    with open(os.path.join(sparse_util.SPARSE_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_sparse_golden.py", "ref_mode": "Mode('py', HIP_QUERY)",
                   "cases": cases}, f)
    print(f"{len(cases)} cases written")


if __name__ == "__main__":
    main()
