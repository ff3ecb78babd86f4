"""Shared by the dense-solve tests and tools/gen_linalg_golden.py: the fixtures under
tests/golden/linalg, the case table, the one-node plans and the accuracy bars of ``SolveTriangular``,
``CholeskySolve``, ``Solve``, ``MatrixInverse`` and ``Det``.

Bars (derived, not tuned; the conv_util convention: twice the textbook bound with eps = 2u).  All
residuals are evaluated in extended precision on the float64 values of the operands.

* Triangular solve (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 8.5: the
  computed x satisfies (T + dT) x = b with |dT| <= gamma_n |T|), element by element:

      |b - op(T) x|_i <= 2 n eps (|op(T)| |x|)_i + tiny

  ``CholeskySolve`` is two such solves: the residual against L L^T at 2 (2n) eps (|L| |L^T| |x|)_i.
* ``Solve`` / ``MatrixInverse`` (Thm 9.4: (A + dA) x = b with |dA| <= gamma_3n |L| |U|):

      |b - A x|_i <= 2 3n eps (E |x|)_i + tiny,      E = |L| |U|

  with E from the float64 ``scipy.linalg.lu`` of the case's matrix, stored in the fixture (as float32,
  enlarged by 1e-6 so that the rounding never lowers a bar).  Both sides pivot by the same rule, so E
  is theirs up to rounding; nothing asks for LAPACK's digits, only for backward stability.
* Forward check (a residual cannot catch a transposed or mis-permuted result of a symmetric case).
  x - x_true = -A^-1 r with |r| below the bar above gives, per column,

      ||x - x64||_inf <= c n eps  || |A^-1| E ||_inf  ||x||_inf + tiny        (c n = 2n, 4n, 6n as above)

  with ``kappa`` = || |A^-1| E ||_inf stored per case (E = |T| for the triangular Ops, |L| |L^T| for
  ``CholeskySolve``).  x64 is the reference in float64 on the same values; a float64 result is judged
  against it at twice the limit, because both carry the bound.
* ``Det``: d = det(A + dA) = det(A) (1 + tr(A^-1 dA) + ...), |dA| <= gamma_3n E, so to first order

      |d - d64| / |d64| <= 2 n eps (S + 1),      S = sum_ij |A^-1|_ji E_ij

  (the + 1: the n roundings of the product); float64 again at twice the limit.

A CPU test holds the reference's OWN outputs to every bar, so a bar that only the kernels miss is a
kernel fault.
"""
import json
import os

import numpy as np

from aesara_amd.plan import Node, Plan
from golden_inputs import make_input

LINALG_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linalg")
DTYPES = ("float32", "float64")
NB = 64                                   # the shipped block size (aesara_amd.exec_linalg.NB)
SIZES = (0, 1, 2, 3, NB - 1, NB, NB + 1, 2 * NB + 2, 4 * NB + 1)
RHS = ("vec", 1, 5, NB + 6)
PLAN_OPS = {"tri": "SolveTriangular", "chol": "CholeskySolve", "solve": "Solve", "inv": "MatrixInverse",
            "det": "Det"}
GARBAGE = 1e30                            # what an entry that must not be read holds (finite)


def _c(op, n, rhs="vec", kind="gauss", **params):
    return dict(op=op, n=n, rhs=rhs, kind=kind, params=params)


def _cases():
    """name -> case.  ``kind``: how the matrix is made (see :func:`matrix`)."""
    t = {}
    for i, n in enumerate(SIZES):
        rhs = RHS[i % 4]
        t[f"tri_n{n}"] = _c("tri", n, rhs, lower=bool(i % 2), trans=(i // 2) % 2, unit_diagonal=False,
                            check_finite=True)
        t[f"solve_n{n}"] = _c("solve", n, RHS[(i + 1) % 4], assume_a="gen", lower=False, check_finite=True)
        t[f"det_n{n}"] = _c("det", n, None, kind="det")
        if n <= 2 * NB + 2:
            t[f"inv_n{n}"] = _c("inv", n, None)
            t[f"chol_n{n}"] = _c("chol", n, RHS[(i + 2) % 4], lower=bool(i % 2), check_finite=True)
    for n in (NB + 1, 2 * NB + 2):
        for lower in (False, True):
            for trans in (0, 1):
                for rhs in RHS:
                    t[f"tri_n{n}_l{int(lower)}t{trans}_{rhs}"] = _c(
                        "tri", n, rhs, lower=lower, trans=trans, unit_diagonal=False, check_finite=True)
            # the diagonal holds garbage and must not be read
            t[f"tri_n{n}_l{int(lower)}_unit"] = _c("tri", n, 5 if lower else "vec", lower=lower, trans=0,
                                                    unit_diagonal=True, check_finite=True)
            # NaN in the triangle that must not be referenced
            t[f"tri_n{n}_l{int(lower)}_nan"] = _c("tri", n, "vec" if lower else 5, kind="nan_other", lower=lower,
                                                   trans=1 - int(lower), unit_diagonal=False, check_finite=False)
            for a in ("sym", "pos"):
                t[f"solve_n{n}_{a}_l{int(lower)}"] = _c("solve", n, 5 if lower else "vec", kind=a, assume_a=a,
                                                        lower=lower, check_finite=True)
        for rhs in RHS:
            t[f"solve_n{n}_{rhs}"] = _c("solve", n, rhs, assume_a="gen", lower=False, check_finite=True)
    # must pivot: a zero leading entry; a scaled permutation matrix; the pivot of column 0 in the LAST
    # row, two blocks below its column
    t["solve_zero_lead"] = _c("solve", 5, "vec", kind="zero_lead", assume_a="gen", lower=False, check_finite=True)
    t["solve_perm"] = _c("solve", NB + 1, 5, kind="perm", assume_a="gen", lower=False, check_finite=True)
    t["solve_far_pivot"] = _c("solve", 2 * NB + 2, 5, kind="reversed", assume_a="gen", lower=False,
                              check_finite=True)
    t["inv_far_pivot"] = _c("inv", 2 * NB + 2, None, kind="reversed")
    # the sign after an odd and after an even number of interchanges
    t["det_swap1"] = _c("det", 4, None, kind="swap1")
    t["det_swap2"] = _c("det", 4, None, kind="swap2")
    t["det_far_pivot"] = _c("det", 2 * NB + 2, None, kind="reversed")
    return t


CASES = _cases()


def eps(dtype):
    return float(np.finfo(dtype).eps)


def tiny(dtype):
    return float(np.finfo(dtype).tiny)


# ------------------------------------------------------------------ inputs ------------
def _gauss(n, m, seed, dtype):
    return make_input({"kind": "normal", "seed": seed, "shape": [n, m], "dtype": dtype, "scale": 1.0,
                       "shift": 0.0}).astype("float64")


def _well(n, seed, dtype):
    """G / sqrt(n) + 2 I: eigenvalues in the disc of radius 1 about 2."""
    return _gauss(n, n, seed, dtype) / np.sqrt(max(n, 1)) + 2.0 * np.eye(n)


def triangular(n, lower, seed, dtype):
    """A well-conditioned triangular matrix: strict triangle N(0, 1/n) (the Neumann series of its
    inverse has terms ~ 1 / (k + 1)!), diagonal +-(1 + |g|)."""
    g = _gauss(n, n, seed, dtype)
    d = np.sign(np.diag(g)) * (1.0 + np.abs(np.diag(g)))
    t = np.tril(g, -1) / np.sqrt(max(n, 1)) + np.diag(d)
    return t if lower else t.T


def matrix(name, dtype):
    """(the matrix operand as handed to the Op, the matrix M the Op stands for): both float64 values
    representable in ``dtype``.  They differ where the Op must not read something."""
    c = CASES[name]
    n, p, kind, seed = c["n"], c["params"], c["kind"], 100 + sorted(CASES).index(name)
    r = lambda a: a.astype(dtype).astype("float64")                      # noqa: E731
    if c["op"] in ("tri", "chol"):
        lower = p["lower"]
        eff = r(triangular(n, lower, seed, dtype))
        other = _gauss(n, n, seed + 1000, dtype)
        if kind == "nan_other":
            other = np.full((n, n), np.nan)
        given = eff + (np.triu(other, 1) if lower else np.tril(other, -1))
        if p.get("unit_diagonal"):
            eff = eff - np.diag(np.diag(eff)) + np.eye(n)
            given = given - np.diag(np.diag(given)) + GARBAGE * np.eye(n)
        return given, eff
    if kind == "gauss":
        a = _gauss(n, n, seed, dtype)
        return a, a
    if kind == "det":
        # sqrt(e / n) brings the geometric mean of |u_ii| of a Gaussian matrix to about 1
        a = r(_gauss(n, n, seed, dtype) * np.sqrt(np.e / max(n, 1)))
        return a, a
    if kind in ("sym", "pos"):
        g = _gauss(n, n, seed, dtype)
        s = r(g @ g.T / n + np.eye(n)) if kind == "pos" else r((g + g.T) / np.sqrt(2.0 * n) + np.diag(np.diag(g)))
        s = np.tril(s) + np.tril(s, -1).T
        other = GARBAGE * np.ones((n, n))
        given = np.tril(s) + np.triu(other, 1) if p["lower"] else np.triu(s) + np.tril(other, -1)
        return given, s
    w = r(_well(n, seed, dtype))
    if kind == "zero_lead":
        a = w[::-1].copy()
        a[0, 0] = 0.0
    elif kind == "reversed":
        a = w[::-1].copy()
        a[-1, 0] = 8.0                    # the pivot of column 0: the last row, in the last block
    elif kind == "perm":
        a = np.zeros((n, n))
        perm = np.random.default_rng(seed).permutation(n)
        a[np.arange(n), perm] = r(1.0 + np.arange(n) / 7.0) * np.where(np.arange(n) % 3, 1.0, -1.0)
    elif kind in ("swap1", "swap2"):
        a = w.copy()
        a[[0, 1]] = a[[1, 0]]
        if kind == "swap2":
            a[[2, 3]] = a[[3, 2]]
    else:
        raise ValueError(kind)
    if c["op"] == "det":
        a = a * 0.5                       # eigenvalues about 1: |det| stays far inside the float32 range
    return a, a


def rhs(name, dtype):
    c = CASES[name]
    if c["rhs"] is None:
        return None
    m = 1 if c["rhs"] == "vec" else c["rhs"]
    b = _gauss(c["n"], m, 5000 + sorted(CASES).index(name), dtype)
    return b[:, 0] if c["rhs"] == "vec" else b


def operands(name, dtype):
    """The operands of a case, contiguous, in ``dtype``."""
    given, _ = matrix(name, dtype)
    b = rhs(name, dtype)
    return [np.ascontiguousarray(given.astype(dtype))] + ([] if b is None else [np.ascontiguousarray(b.astype(dtype))])


def system(name, dtype):
    """(M, E, c): the matrix with ``op(M) x = b`` in float64, the matrix of the bar and its factor
    c (bar = c eps E |x|), ``E`` still missing for the LU Ops (it is the stored one)."""
    c = CASES[name]
    _, eff = matrix(name, dtype)
    n = c["n"]
    if c["op"] == "tri":
        M = eff.T if c["params"]["trans"] else eff
        return M, np.abs(M), 2 * n
    if c["op"] == "chol":
        L = eff if c["params"]["lower"] else eff.T
        return L @ L.T, np.abs(L) @ np.abs(L.T), 4 * n
    return eff, None, 6 * n


# ------------------------------------------------------------------ bars --------------
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def residual_ratio(M, E, x, b, cn, dtype):
    """max_i |b - M x|_i / (cn eps (E |x|)_i + tiny); 0 for an empty system."""
    if np.size(x) == 0:
        return 0.0
    x2 = _ld(x).reshape(M.shape[0], -1)
    b2 = _ld(b).reshape(x2.shape)
    bar = cn * eps(dtype) * (_ld(E) @ np.abs(x2)) + tiny(dtype)
    return float(np.max(np.abs(b2 - _ld(M) @ x2) / bar))


def forward_ratio(x, x64, kappa, cn, dtype):
    """max over the columns of ||x - x64||_inf / (cn eps kappa ||x||_inf + tiny), a float64 result
    at twice the limit."""
    if np.size(x) == 0:
        return 0.0
    x2 = np.asarray(x, "float64").reshape(np.shape(x)[0], -1)
    w2 = np.asarray(x64, "float64").reshape(x2.shape)
    both = 2.0 if np.dtype(dtype) == np.float64 else 1.0
    lim = both * cn * eps(dtype) * kappa * np.max(np.abs(x2), axis=0) + tiny(dtype)
    return float(np.max(np.max(np.abs(x2 - w2), axis=0) / lim))


def det_ratio(d, d64, S, n, dtype):
    both = 2.0 if np.dtype(dtype) == np.float64 else 1.0
    return float(abs(float(d) - float(d64)) / (both * 2 * n * eps(dtype) * (S + 1.0) * abs(float(d64)) + tiny(dtype)))


def ratios(name, dtype, got, z):
    """{check: ratio} of a result ``got`` of a case against its bars (``z``: the loaded fixture);
    every ratio <= 1 passes."""
    c = CASES[name]
    got = np.asarray(got)
    if c["op"] == "det":
        return {"det": det_ratio(got, z["x64"], float(z["S"]), c["n"], dtype)}
    M, E, cn = system(name, dtype)
    if E is None:
        E = z["E"].astype("float64")
    b = np.eye(c["n"]) if c["op"] == "inv" else rhs(name, dtype)
    return {"residual": residual_ratio(M, E, got, b, cn, dtype),
            "forward": forward_ratio(got, z["x64"], float(z["kappa"]), cn, dtype)}


def out_shape(name):
    c = CASES[name]
    if c["op"] == "det":
        return ()
    if c["op"] == "inv":
        return (c["n"], c["n"])
    return (c["n"],) if c["rhs"] == "vec" else (c["n"], c["rhs"])


# ------------------------------------------------------------------ fixtures, plans ---
def _all_cases():
    with open(os.path.join(LINALG_GOLDEN, "cases.json")) as f:
        return json.load(f)["cases"]


def load_cases():
    """The op-level entries of cases.json."""
    return [c for c in _all_cases() if c["op"] != "graph"]


def load_graph_cases():
    """(graph, dtype) -> the graph-level entries of cases.json."""
    return {(c["name"], c["dtype"]): c for c in _all_cases() if c["op"] == "graph"}


def case_file(name, dtype):
    return os.path.join(LINALG_GOLDEN, f"{name}_{dtype}.npz")


def op_plan(name, dtype):
    """The one-node plan a case lowers to (tests/test_linalg_lowering.py holds the linker to it)."""
    c = CASES[name]
    plan = Plan(f"linalg_{name}_{dtype}", {}, [], [], [])
    ins = [plan.new_var(dtype, [None, None], "A")]
    if c["rhs"] is not None:
        ins.append(plan.new_var(dtype, [None] if c["rhs"] == "vec" else [None, None], "b"))
    out = plan.new_var(dtype, [None] * len(out_shape(name)))
    plan.inputs, plan.outputs = list(ins), [out]
    plan.nodes.append(Node(PLAN_OPS[c["op"]], list(ins), [out], dict(c["params"])))
    return plan


def same_lowering(lowered, built):
    """Whether the plan the linker lowered is ``built``: one node, same op, parameters, operands."""
    if len(lowered.nodes) != 1 or len(lowered.inputs) != len(built.inputs):
        return False
    a, b = lowered.nodes[0], built.nodes[0]

    def operand(plan, v):
        return plan.vars[v].dtype, len(plan.vars[v].shape), plan.inputs.index(v)
    return a.op == b.op and a.params == b.params and a.outputs == lowered.outputs and \
        [operand(lowered, v) for v in a.inputs] == [operand(built, v) for v in b.inputs]


# ------------------------------------------------------------------ graph-level cases -
# Whole graphs under mode="HIP" (tests/test_gpu_linalg_function.py), all at n = NB + 1 (``map``: three
# 5 x 5 systems) on well-conditioned matrices.  Every output is a chain of at most ``stages`` dense
# solves and products of their results, so its error is at most the sum of the forward limits of
# the module docstring, one per stage:
#
#     max |got - exact| / max |exact| <= stages * 6 n eps kappa       (float64 against the reference's
#                                                                       float64 output: twice that)
#
# with kappa = || |A^-1| E ||_inf of the graph's matrix, computed by the generator and stored.
GRAPH_N = NB + 1
# graph -> (plan ops it must hold, stages of each output)
GRAPHS = {
    "g_solve": ({"Solve": 2}, (1, 2, 2)),                       # x, d cost / d A, d cost / d b
    "g_tri": ({"SolveTriangular": 2}, (1, 2, 2)),
    "g_inv_det": ({"MatrixInverse": 1, "Det": 1}, (1, 1, 3, 2)),   # inverse, det, and their gradients
    "g_nll": ({"Solve": 1, "Det": 1}, (3, 3)),                  # the likelihood and its gradient
    "g_map": ({"Scan": 1}, (1,)),
}


def graph_values(gname, dtype):
    """The input values of a graph-level case (float64 values representable in ``dtype``)."""
    n = GRAPH_N
    r = lambda a: a.astype(dtype)                                         # noqa: E731
    vec = lambda seed: r(_gauss(n, 1, seed, dtype)[:, 0])                 # noqa: E731
    if gname == "g_solve":
        return [r(_well(n, 901, dtype)), vec(902), vec(903)]
    if gname == "g_tri":
        return [r(triangular(n, True, 911, dtype)), vec(912), vec(913)]
    if gname == "g_inv_det":
        return [r(_well(n, 921, dtype) * 0.5), r(_gauss(n, n, 922, dtype))]
    if gname == "g_nll":
        # (halved: det(L L^T + I) stays inside the float32 range)
        return [r(triangular(n, True, 931, dtype) * 0.5), vec(932)]
    if gname == "g_map":
        return [r(np.stack([_well(5, 941 + i, dtype) for i in range(3)])), r(_gauss(3, 5, 945, dtype))]
    raise ValueError(gname)


def graph_file(gname, dtype):
    return os.path.join(LINALG_GOLDEN, f"{gname}_{dtype}.npz")


def rel_max(got, exact):
    got, exact = np.asarray(got, "float64"), np.asarray(exact, "float64")
    den = float(np.max(np.abs(exact))) if exact.size else 0.0
    num = float(np.max(np.abs(got - exact))) if exact.size else 0.0
    return num if den == 0 else num / den


def graph_cap(gname, k, dtype, kappa, n):
    both = 2.0 if np.dtype(dtype) == np.float64 else 1.0
    return both * GRAPHS[gname][1][k] * 6 * n * eps(dtype) * kappa
