"""Shared by the QR tests and tools/gen_qr_golden.py: the fixtures under tests/golden/qr, the case
table, the one-node plans and the accuracy bars of ``QR`` (``nlinalg.qr``, every mode).

Bars (ratios <= 1 pass; everything is evaluated in ``longdouble`` on the float64 values).  The yardstick
is the float64 reference ITSELF on the same case (``np.linalg.qr``: LAPACK geqrf + orgqr), not the
textbook bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 19.4: columnwise
gamma~_mn with an unspecified constant, about 1000 times too loose to catch anything):

* residual, per column:   rho_res = max_j ||(A - Q R)_j||_2 / (eps ||a_j||_2)   (a zero column must be
  reproduced exactly).  The float64 reference sits at a few eps64 (at most 6.4 on these cases); its ratio of the SAME
  case, ``rho_res`` in units of eps64, is stored.  Device bar: 4 max(rho_res, 1) eps(dtype).  The 4 pays
  for another block size and summation order (tree folds, GEMM updates): they change the constant,
  not the growth.
* orthogonality:          ||Q^T Q - I||_2 <= 4 max(rho_orth, 1) eps(dtype), ``rho_orth`` stored likewise.
* forward, for kappa2 = kappa_2(A) <= 300:   ||R - R64||_F / ||R64||_F <= 2 sqrt(2) kappa2 (residual bar),
  the first-order QR perturbation bound, doubled; the signs of diag(R) are those of R64; ``tau`` of
  'raw' is held to the same bar against ``tau64``.
* 'raw': Q is rebuilt on the host in float64 from (h, tau) and held to the same bars; 'r' has no Q, so
  it is held to the forward check alone.

A rank-deficient matrix has no unique R: the cases ``equal_cols`` and ``zero_col`` (kappa2 = inf) are
outside the forward check by the kappa2 cap, and they are the only ones — every other matrix is
G / sqrt(max(M, N)) + 2 I with random column signs, kappa2 below 10.

A CPU test holds the reference's OWN outputs to every bar, so a bar that only the kernels miss is a
kernel fault.
"""
import json
import os

import numpy as np

from aesara_amd.plan import Node, Plan
from golden_inputs import make_input

QR_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qr")
DTYPES = ("float32", "float64")
NB = 64                                   # the shipped block size (aesara_amd.exec_linalg.NB)
MODES = ("reduced", "complete", "r", "raw")
KAPPA_CAP = 300.0
MARGIN = 4.0


def _c(m, n, mode="reduced", kind="well", dtypes=DTYPES):
    return dict(m=m, n=n, mode=mode, kind=kind, dtypes=tuple(dtypes))


def _cases():
    t = {}
    for n in (0, 1, 2, 3, NB - 1, NB, NB + 1, 2 * NB + 2):
        t[f"sq_n{n}"] = _c(n, n)
    shapes = {"sq": (NB + 1, NB + 1), "tall": (2 * NB + 2, NB + 1), "wide": (NB + 1, 2 * NB + 2)}
    for mode in MODES:
        for s, (m, n) in shapes.items():
            if not (mode == "reduced" and s == "sq"):
                t[f"{s}_{mode}"] = _c(m, n, mode)
    t["tall_thin"] = _c(4 * NB + 1, 3)
    t["wide_thin"] = _c(3, 4 * NB + 1)
    t["tall_thin_complete"] = _c(2 * NB + 2, 3, "complete")
    # empty extents, as NumPy has them
    t["empty_rows"] = _c(0, 3)
    t["empty_cols_complete"] = _c(3, 0, "complete")
    # already upper triangular: every tau is exactly 0, diag(R) = diag(A), Q = I exactly
    t["triu_reduced"] = _c(NB + 2, NB + 2, "reduced", "triu")
    t["triu_raw"] = _c(NB + 2, NB + 2, "raw", "triu")
    # zero columns inside the first panel and at the start of the second
    t["zero_col"] = _c(NB + 6, NB + 2, "reduced", "zero_col")
    # column 50 repeats column 10: rank deficient
    t["equal_cols"] = _c(NB + 6, NB + 2, "reduced", "equal_cols")
    # the column norm must neither overflow nor vanish
    t["huge"] = _c(2 * NB + 2, NB + 1, "reduced", "huge", ("float32",))
    t["tiny"] = _c(2 * NB + 2, NB + 1, "reduced", "tiny", ("float32",))
    return t


CASES = _cases()
ZERO_COLS = (30, NB)
EQUAL_COLS = (10, 50)
NAN_AT = (5, 40)                           # the NaN of :func:`nan_matrix`


def eps(dtype):
    return float(np.finfo(dtype).eps)


# ------------------------------------------------------------------ inputs ------------
def _gauss(m, n, seed, dtype):
    return make_input({"kind": "normal", "seed": seed, "shape": [m, n], "dtype": dtype, "scale": 1.0,
                       "shift": 0.0}).astype("float64")


def well(m, n, seed, dtype):
    """(G / sqrt(max(m, n)) + 2 I) D with D = diag(+-1): singular values about [1, 3], diag(R) of
    both signs; float64 values representable in ``dtype``."""
    a = _gauss(m, n, seed, dtype) / np.sqrt(max(m, n, 1)) + 2.0 * np.eye(m, n)
    signs = np.where(np.random.default_rng(seed).random(n) < 0.5, -1.0, 1.0)
    return (a * signs).astype(dtype).astype("float64")


def matrix(name, dtype):
    """The matrix of a case: float64 values representable in ``dtype``."""
    c = CASES[name]
    seed = 300 + sorted(CASES).index(name)
    a = well(c["m"], c["n"], seed, dtype)
    kind = c["kind"]
    if kind == "triu":
        a = np.triu(a)
    elif kind == "zero_col":
        a[:, list(ZERO_COLS)] = 0.0
    elif kind == "equal_cols":
        a[:, EQUAL_COLS[1]] = a[:, EQUAL_COLS[0]]
    elif kind in ("huge", "tiny"):
        a = (a * (1e30 if kind == "huge" else 1e-30)).astype(dtype).astype("float64")
    elif kind != "well":
        raise ValueError(kind)
    return a


def operand(name, dtype):
    return np.ascontiguousarray(matrix(name, dtype).astype(dtype))


def nan_matrix(dtype):
    a = well(NB + 6, NB + 2, 999, dtype).astype(dtype)
    a[NAN_AT] = np.nan
    return a


def out_shapes(m, n, mode):
    k = min(m, n)
    return {"reduced": [(m, k), (k, n)], "complete": [(m, m), (m, n)], "r": [(k, n)],
            "raw": [(n, m), (k,)]}[mode]


# ------------------------------------------------------------------ bars --------------
def _ld(a):
    return np.asarray(a, dtype=np.longdouble)


def rho_res(A, Q, R, dtype):
    """max_j ||(A - Q R)_j||_2 / (eps ||a_j||_2), in units of eps(dtype); a zero column of A must be
    reproduced exactly (inf otherwise); 0 for an empty matrix."""
    A = _ld(A)
    if A.size == 0:
        return 0.0
    d = np.sqrt(np.sum((A - _ld(Q) @ _ld(R)) ** 2, axis=0))
    na = np.sqrt(np.sum(A ** 2, axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(na > 0, d / np.where(na > 0, na, 1), np.where(d > 0, np.inf, 0.0))
    return float(np.max(r) / eps(dtype))


def rho_orth(Q, dtype):
    """||Q^T Q - I||_2 in units of eps(dtype)."""
    Q = _ld(Q)
    if Q.shape[1] == 0:
        return 0.0
    e = Q.T @ Q - np.eye(Q.shape[1], dtype=np.longdouble)
    return float(np.linalg.norm(np.asarray(e, "float64"), 2) / eps(dtype))


def rebuild(h, tau):
    """(Q, R) of the reduced factorisation in float64 from the 'raw' pair (LAPACK orgqr by hand)."""
    Hf = np.asarray(h, "float64").T
    m, n = Hf.shape
    k = min(m, n)
    Q = np.eye(m, k)
    for j in reversed(range(k)):
        v = np.zeros(m)
        v[j] = 1.0
        v[j + 1:] = Hf[j + 1:, j]
        Q -= float(tau[j]) * np.outer(v, v @ Q)
    return Q, np.triu(Hf[:k])


def factors(mode, outs):
    """(Q or None, R, tau or None) as float64 from the outputs of a mode."""
    if mode == "r":
        return None, np.asarray(outs[0], "float64"), None
    if mode == "raw":
        Q, R = rebuild(outs[0], outs[1])
        return Q, R, np.asarray(outs[1], "float64")
    return np.asarray(outs[0], "float64"), np.asarray(outs[1], "float64"), None


def res_bar(z, dtype):
    return MARGIN * max(float(z["rho_res"]), 1.0) * eps(dtype)


def _rel(x, ref):
    x, ref = _ld(x), _ld(ref)
    den = np.sqrt(np.sum(ref ** 2))
    num = np.sqrt(np.sum((x - ref) ** 2))
    return float(num if den == 0 else num / den)


def ratios(name, dtype, outs, z):
    """{check: ratio} of the outputs of a case against its bars (``z``: the loaded fixture)."""
    c = CASES[name]
    A = matrix(name, dtype)
    Q, R, tau = factors(c["mode"], outs)
    r = {}
    if Q is not None:
        r["residual"] = rho_res(A, Q, R, dtype) * eps(dtype) / res_bar(z, dtype)
        r["orthogonality"] = rho_orth(Q, dtype) / (MARGIN * max(float(z["rho_orth"]), 1.0))
    kappa = float(z["kappa2"])
    if kappa <= KAPPA_CAP and R.size:
        fbar = 2.0 * np.sqrt(2.0) * kappa * res_bar(z, dtype)
        k = min(R.shape)
        R64 = np.asarray(z["R64"], "float64")
        r["forward"] = _rel(R, R64) / fbar
        r["signs"] = 0.0 if np.array_equal(np.sign(np.diag(R)[:k]), np.sign(np.diag(R64)[:k])) else np.inf
        if tau is not None:
            r["tau"] = _rel(tau, z["tau64"]) / fbar
    return r


# ------------------------------------------------------------------ fixtures, plans ---
def load_cases():
    with open(os.path.join(QR_GOLDEN, "cases.json")) as f:
        return json.load(f)["cases"]


def case_file(name, dtype):
    return os.path.join(QR_GOLDEN, f"{name}_{dtype}.npz")


def all_cases():
    return [(name, dt) for name in sorted(CASES) for dt in CASES[name]["dtypes"]]


def plan_of(mode, dtype, name="qr"):
    """The one-node plan ``nlinalg.qr(A, mode)`` lowers to (tests/test_qr_lowering.py holds the linker
    to it)."""
    plan = Plan(name, {}, [], [], [])
    A = plan.new_var(dtype, [None, None], "A")
    outs = [plan.new_var(dtype, [None] * len(s)) for s in out_shapes(1, 1, mode)]
    plan.inputs, plan.outputs = [A], list(outs)
    plan.nodes.append(Node("QR", [A], list(outs), {"mode": mode}))
    return plan


def op_plan(name, dtype):
    return plan_of(CASES[name]["mode"], dtype, f"qr_{name}_{dtype}")


def same_lowering(lowered, built):
    """Whether the plan the linker lowered is ``built``: one node, same op, parameters, operands."""
    if len(lowered.nodes) != 1 or len(lowered.inputs) != 1:
        return False
    a, b = lowered.nodes[0], built.nodes[0]
    var = lambda plan, v: (plan.vars[v].dtype, len(plan.vars[v].shape))          # noqa: E731
    return a.op == b.op and a.params == b.params and a.inputs == lowered.inputs and \
        a.outputs == lowered.outputs and \
        [var(lowered, v) for v in a.inputs + a.outputs] == [var(built, v) for v in b.inputs + b.outputs]


# ------------------------------------------------------------------ graph-level cases -
# x = solve_triangular(R, Q^T b) with Q, R = qr(A) on a 130 x 66 well-conditioned A and b = A x0: a
# zero-residual least-squares problem, whose forward error is at most kappa2 times the backward
# error to first order.  The backward error is the relative residual bar of QR plus that of the
# triangular solve and the product Q^T b (2 N eps); doubled:
#
#     ||x - x64||_2 / ||x64||_2 <= 2 kappa2 (4 max(rho_res, 1) eps + 2 N eps)
LSTSQ_M, LSTSQ_N = 2 * NB + 2, NB + 2


def lstsq_values(dtype):
    A = well(LSTSQ_M, LSTSQ_N, 951, dtype)
    x0 = _gauss(LSTSQ_N, 1, 952, dtype)[:, 0]
    return [A.astype(dtype), (A @ x0).astype(dtype)]


def lstsq_cap(z, dtype):
    return 2.0 * float(z["kappa2"]) * (res_bar(z, dtype) + 2.0 * LSTSQ_N * eps(dtype))


def graph_file(gname, dtype):
    return os.path.join(QR_GOLDEN, f"{gname}_{dtype}.npz")
