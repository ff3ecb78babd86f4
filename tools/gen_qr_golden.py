#!/usr/bin/env python
"""Generate the QR fixtures under tests/golden/qr/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like tools/gen_linalg_golden.py).  Every case
of tests/qr_util.CASES, in the dtypes it names, is built with the reference, rewritten with the HIP
linker's query and evaluated with ``Mode("py", HIP_QUERY)`` — ``QRFull.perform``, ``np.linalg.qr``.
The one-node plans are qr_util.op_plan, and the linker's lowering is held to them.

One file per case and dtype:

* ``out0`` (, ``out1``): the reference's outputs in the case's dtype;
* ``R64`` (and ``tau64`` for 'raw'): the same graph in float64 on the same values;
* ``kappa2`` = kappa_2(A) (inf for a rank-deficient matrix, 0 for an empty one);
* ``rho_res`` / ``rho_orth``: the two ratios of the float64 reference's own factorisation of the case
  ('complete' for a 'complete' case, else 'reduced'), in units of eps64, evaluated in longdouble.

Self-check: the reference's own outputs must be inside every bar of tests/qr_util.py; a case that is
not is refused (nothing is written).  Every case but the rank-deficient ones must have kappa2 <= 300.

Usage:  python tools/gen_qr_golden.py
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
from aesara.compile.mode import Mode  # noqa: E402
from aesara.tensor import nlinalg, slinalg  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import qr_util  # noqa: E402
from qr_util import CASES  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

PY_MODE = Mode("py", HIP_QUERY)
RANK_DEFICIENT = ("zero_col", "equal_cols")
MAX_FILE = 321443                      # the largest file under tests/golden/linalg


def T(dtype, ndim, name):
    return TensorType(dtype, shape=(None,) * ndim)(name)


def qr_graph(mode, dtype):
    """(inputs, outputs) of ``nlinalg.qr(A, mode)``."""
    A = T(dtype, 2, "A")
    out = nlinalg.qr(A, mode)
    return [A], list(out) if isinstance(out, (list, tuple)) else [out]


def op_graph(name, dtype):
    return qr_graph(CASES[name]["mode"], dtype)


def lower(ins, outs, name):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore", accept_inplace=True)
    plan = f.maker.linker.plan
    plan.name = name
    return plan


def reference(ins, outs):
    return ae.function(ins, outs, mode=PY_MODE, on_unused_input="ignore", accept_inplace=True)


def run(mode, dtype, a):
    return [np.array(o) for o in reference(*qr_graph(mode, dtype))(a.astype(dtype))]


def kappa2(a):
    if a.size == 0:
        return 0.0
    s = np.linalg.svd(a, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


def yardstick(a, mode):
    """(rho_res, rho_orth) of the float64 reference on ``a``, in units of eps64."""
    Q, R = run("complete" if mode == "complete" else "reduced", "float64", a)
    return qr_util.rho_res(a, Q, R, "float64"), qr_util.rho_orth(Q, "float64")


def case(name, dt):
    c = CASES[name]
    mode = c["mode"]
    assert qr_util.same_lowering(lower(*op_graph(name, dt), f"{name}_{dt}"), qr_util.op_plan(name, dt)), name
    a = qr_util.matrix(name, dt)
    outs = run(mode, dt, a)
    outs64 = run(mode, "float64", a)
    shapes = qr_util.out_shapes(c["m"], c["n"], mode)
    assert [o.shape for o in outs] == shapes and all(o.dtype == np.dtype(dt) for o in outs), (name, dt)
    _, R64, tau64 = qr_util.factors(mode, outs64)
    kap = kappa2(a)
    assert kap <= qr_util.KAPPA_CAP or (name in RANK_DEFICIENT and kap > 1e12), (name, kap)
    rr, ro = yardstick(a, mode)
    arrays = {f"out{i}": o for i, o in enumerate(outs)}
    arrays.update(R64=R64, kappa2=np.asarray(kap), rho_res=np.asarray(rr), rho_orth=np.asarray(ro))
    if tau64 is not None:
        arrays["tau64"] = tau64
    r = qr_util.ratios(name, dt, outs, arrays)
    if not all(v <= 1.0 for v in r.values()):
        raise SystemExit(f"{name} {dt}: the reference itself is at {r} of its bars — case refused, "
                         "nothing written")
    print(f"[ok] {name} {dt}: kappa2 {kap:.3g}, rho_res {rr:.2f}, rho_orth {ro:.2f}; "
          + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    entry = {"name": name, "dtype": dt, "mode": mode, "m": c["m"], "n": c["n"], "kappa2": kap if np.isfinite(kap) else "inf",
             "rho_res": rr, "rho_orth": ro, "ref_ratio": r}
    return entry, arrays


def lstsq_graph(dtype):
    A, b = T(dtype, 2, "A"), T(dtype, 1, "b")
    Q, R = nlinalg.qr(A)
    return [A, b], [slinalg.solve_triangular(R, Q.T.dot(b))]


def r_graph(dtype):
    return qr_graph("r", dtype)


def graph_cases(dt):
    A, b = qr_util.lstsq_values(dt)
    a64 = A.astype("float64")
    (x,) = reference(*lstsq_graph(dt))(A, b)
    (x64,) = reference(*lstsq_graph("float64"))(a64, b.astype("float64"))
    rr, ro = yardstick(a64, "reduced")
    kap = kappa2(a64)
    ops = [n.op for n in lower(*lstsq_graph(dt), f"g_lstsq_{dt}").nodes]
    assert "QR" in ops and "SolveTriangular" in ops, ops
    z = {"out": np.array(x), "x64": np.array(x64), "kappa2": np.asarray(kap), "rho_res": np.asarray(rr),
         "rho_orth": np.asarray(ro)}
    err = qr_util._rel(z["out"], z["x64"])
    cap = qr_util.lstsq_cap(z, dt)
    if dt == "float32" and not err <= cap:
        raise SystemExit(f"g_lstsq {dt}: the reference itself is at {err / cap:.3f} of the cap")
    print(f"[ok] g_lstsq {dt}: kappa2 {kap:.2f}, reference at {err / cap:.4f} of the cap")
    (R,) = reference(*r_graph(dt))(A)
    (R64,) = reference(*r_graph("float64"))(a64)
    zr = {"out": np.array(R), "R64": np.array(R64), "kappa2": np.asarray(kap), "rho_res": np.asarray(rr),
          "rho_orth": np.asarray(ro)}
    return {qr_util.graph_file("g_lstsq", dt): z, qr_util.graph_file("g_r", dt): zr}


def main():
    os.makedirs(qr_util.QR_GOLDEN, exist_ok=True)
    cases, files = [], {}
    for dt in qr_util.DTYPES:
        files.update(graph_cases(dt))
    for name, dt in qr_util.all_cases():
        entry, arrays = case(name, dt)
        cases.append(entry)
        files[qr_util.case_file(name, dt)] = arrays
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) <= MAX_FILE, (path, os.path.getsize(path))
    with open(os.path.join(qr_util.QR_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_qr_golden.py", "ref_mode": "Mode('py', HIP_QUERY)",
                   "cases": cases}, f)
    print(f"{len(cases)} cases written")


if __name__ == "__main__":
    main()
