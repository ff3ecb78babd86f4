#!/usr/bin/env python
"""Generate the dense-solve fixtures under tests/golden/linalg/ by RUNNING THE REFERENCE.

TEST INFRASTRUCTURE ONLY (needs the reference front end, like tools/gen_pool_golden.py).  Every case
of tests/linalg_util.CASES, in float32 and float64, is built with the reference, rewritten with the
HIP linker's query and evaluated with ``Mode("py", HIP_QUERY)`` — the Ops' own ``perform``
(``scipy.linalg.solve_triangular`` / ``cho_solve`` / ``solve``, ``np.linalg.inv`` / ``det``).  The
one-node plans are linalg_util.op_plan, and the linker's lowering is held to them.

One file per case and dtype:

* ``out``: the reference's output in the case's dtype;
* ``x64``: the same graph in float64 on the same values;
* ``kappa`` = || |op(M)^-1| E ||_inf (the forward check), and for the LU Ops ``E`` = P |L| |U| from
  ``scipy.linalg.lu`` of the matrix in float64 (stored as float32, enlarged by 1e-6);
* ``Det``: ``S`` = sum_ij |A^-1|_ji E_ij and, in cases.json, ``parity`` (the determinant of the row
  permutation).  The generator asserts 1e-20 < |det| < 1e20.

Self-check: the reference's own output must be inside every bar of tests/linalg_util.py; a case that
is not is refused (nothing is written).

Usage:  python tools/gen_linalg_golden.py
"""
import json
import os
import sys

import numpy as np
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_overlay  # noqa: E402

ae = ref_overlay.import_reference()
import aesara.tensor as at  # noqa: E402
from aesara.compile.mode import Mode  # noqa: E402
from aesara.tensor import nlinalg, slinalg  # noqa: E402
from aesara.tensor.type import TensorType  # noqa: E402

import linalg_util  # noqa: E402
from linalg_util import CASES  # noqa: E402

from aesara_amd.linker import HIP_QUERY, HipLinker  # noqa: E402

PY_MODE = Mode("py", HIP_QUERY)


def T(dtype, ndim, name):
    return TensorType(dtype, shape=(None,) * ndim)(name)


def op_graph(name, dtype):
    """(inputs, [output]) of a case."""
    c = CASES[name]
    A = T(dtype, 2, "A")
    if c["rhs"] is None:
        return [A], [(nlinalg.MatrixInverse() if c["op"] == "inv" else nlinalg.Det())(A)]
    b = T(dtype, 1 if c["rhs"] == "vec" else 2, "b")
    op = {"tri": slinalg.SolveTriangular, "chol": slinalg.CholeskySolve, "solve": slinalg.Solve}[c["op"]]
    return [A, b], [op(**c["params"])(A, b)]


def lower(ins, outs, name):
    linker = HipLinker(executor_factory=lambda plan: (lambda *a: None))
    f = ae.function(ins, outs, mode=Mode(linker, HIP_QUERY), on_unused_input="ignore", accept_inplace=True)
    plan = f.maker.linker.plan
    plan.name = name
    return plan


def reference(ins, outs):
    return ae.function(ins, outs, mode=PY_MODE, on_unused_input="ignore", accept_inplace=True)


def case(name, dt):
    c = CASES[name]
    n = c["n"]
    assert linalg_util.same_lowering(lower(*op_graph(name, dt), f"{name}_{dt}"), linalg_util.op_plan(name, dt)), name
    xs = linalg_util.operands(name, dt)
    (out,) = reference(*op_graph(name, dt))(*xs)
    (x64,) = reference(*op_graph(name, "float64"))(*[x.astype("float64") for x in xs])
    out, x64 = np.array(out), np.array(x64)
    assert out.dtype == np.dtype(dt) and out.shape == linalg_util.out_shape(name), (name, out.dtype, out.shape)
    M, E, _ = linalg_util.system(name, dt)
    entry = {"name": name, "dtype": dt, "op": c["op"], "n": n}
    arrays = {"out": out, "x64": x64}
    if E is None:
        P, L, U = scipy.linalg.lu(M) if n else (M, M, M)
        E = P @ (np.abs(L) @ np.abs(U))
        arrays["E"] = (E * (1.0 + 1e-6)).astype("float32")
        entry["parity"] = int(round(np.linalg.det(P))) if n else 1
    Minv = np.linalg.inv(M) if n else M
    if c["op"] == "det":
        arrays["S"] = np.asarray(np.sum(np.abs(Minv).T * E))
        assert 1e-20 < abs(float(x64)) < 1e20, (name, float(x64))
        assert n == 0 or np.sign(float(x64)) == np.sign(np.prod(np.sign(np.diag(U)))) * entry["parity"]
    else:
        arrays["kappa"] = np.asarray(np.max(np.sum(np.abs(Minv) @ E, axis=1)) if n else 0.0)
    z = {k: np.asarray(v) for k, v in arrays.items()}
    r = linalg_util.ratios(name, dt, out, z)
    if not all(v <= 1.0 for v in r.values()):
        raise SystemExit(f"{name} {dt}: the reference itself is at {r} of its bars — case refused, "
                         "nothing written")
    entry["ref_ratio"] = r
    print(f"[ok] {name} {dt}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    return entry, arrays


def g_solve(dt):
    A, b, w = T(dt, 2, "A"), T(dt, 1, "b"), T(dt, 1, "w")
    x = slinalg.solve(A, b)
    return [A, b, w], [x] + ae.grad((x * w).sum(), [A, b])


def g_tri(dt):
    A, b, w = T(dt, 2, "A"), T(dt, 1, "b"), T(dt, 1, "w")
    x = slinalg.solve_triangular(A, b, lower=True)
    return [A, b, w], [x] + ae.grad((x * w).sum(), [A, b])


def g_inv_det(dt):
    A, V = T(dt, 2, "A"), T(dt, 2, "V")
    inv, d = nlinalg.matrix_inverse(A), nlinalg.det(A)
    return [A, V], [inv, d, ae.grad((inv * V).sum(), A), ae.grad(d, A)]


def g_nll(dt):
    """Gaussian negative log-likelihood 1/2 r^T S^-1 r + 1/2 log |det S| with S = L L^T + I, and its
    gradient with respect to the factor L."""
    L, r = T(dt, 2, "L"), T(dt, 1, "r")
    S = at.dot(L, L.T) + at.eye(L.shape[0], dtype=dt)
    nll = 0.5 * at.dot(r, slinalg.solve(S, r, assume_a="pos")) + 0.5 * at.log(abs(nlinalg.det(S)))
    return [L, r], [nll, ae.grad(nll, L)]


def g_map(dt):
    import aesara
    As, bs = T(dt, 3, "As"), T(dt, 2, "bs")
    xs, _ = aesara.map(lambda a, b: slinalg.solve(a, b), [As, bs])
    return [As, bs], [xs]


GRAPHS = {"g_solve": g_solve, "g_tri": g_tri, "g_inv_det": g_inv_det, "g_nll": g_nll, "g_map": g_map}


def graph_matrix(gname, xs):
    """The float64 matrix whose solves the graph chains (its kappa enters the cap)."""
    a = xs[0].astype("float64")
    if gname == "g_nll":
        return a @ a.T + np.eye(a.shape[0])
    return a


def graph_case(gname, dt):
    ins, outs = GRAPHS[gname](dt)
    plan = lower(ins, outs, f"{gname}_{dt}")
    ops = [n.op for n in plan.nodes]
    for k, cnt in linalg_util.GRAPHS[gname][0].items():
        assert ops.count(k) >= cnt, (gname, k, ops)
    xs = linalg_util.graph_values(gname, dt)
    ref = [np.array(o) for o in reference(ins, outs)(*xs)]
    assert all(o.dtype == np.dtype(dt) for o in ref), [o.dtype for o in ref]
    exact = [np.array(o) for o in reference(*GRAPHS[gname]("float64"))(*[x.astype("float64") for x in xs])]
    kappa = 0.0
    M = graph_matrix(gname, xs)
    for m in (M if M.ndim == 3 else [M]):
        if gname == "g_tri":
            E = np.abs(m)
        else:
            P, L, U = scipy.linalg.lu(m)
            E = P @ (np.abs(L) @ np.abs(U))
        kappa = max(kappa, float(np.max(np.sum(np.abs(np.linalg.inv(m)) @ E, axis=1))))
    n = M.shape[-1]
    entry = {"name": gname, "dtype": dt, "op": "graph", "n": n, "kappa": kappa, "n_out": len(ref), "ref_ratio": []}
    for k, (r, e) in enumerate(zip(ref, exact)):
        ratio = linalg_util.rel_max(r, e) / linalg_util.graph_cap(gname, k, dt, kappa, n)
        if dt == "float32" and not ratio <= 1.0:
            raise SystemExit(f"{gname} {dt} output {k}: the reference itself is at {ratio:.3f} of the cap")
        entry["ref_ratio"].append(ratio)
    print(f"[ok] {gname} {dt}: kappa = {kappa:.1f}, reference at {entry['ref_ratio']} of the caps")
    arrays = {f"out{k}": r for k, r in enumerate(ref)}
    arrays.update({f"exact{k}": e for k, e in enumerate(exact)})
    return entry, arrays


def main():
    os.makedirs(linalg_util.LINALG_GOLDEN, exist_ok=True)
    cases, files = [], {}
    for gname in GRAPHS:
        for dt in linalg_util.DTYPES:
            entry, arrays = graph_case(gname, dt)
            cases.append(entry)
            files[linalg_util.graph_file(gname, dt)] = arrays
    for name in CASES:
        for dt in linalg_util.DTYPES:
            entry, arrays = case(name, dt)
            cases.append(entry)
            files[linalg_util.case_file(name, dt)] = arrays
    parities = {c["parity"] for c in cases if c["op"] == "det" and c["n"] > 1}
    assert parities == {1, -1}, parities
    for path, arrays in files.items():
        np.savez_compressed(path, **arrays)
    with open(os.path.join(linalg_util.LINALG_GOLDEN, "cases.json"), "w") as f:
        json.dump({"generator": "tools/gen_linalg_golden.py", "ref_mode": "Mode('py', HIP_QUERY)",
                   "cases": cases}, f)
    print(f"{len(cases)} cases written")


if __name__ == "__main__":
    main()
