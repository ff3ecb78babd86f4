"""Cases, bars and plans of the sparse Ops (tests/test_sparse_lowering.py, tests/test_gpu_sparse.py,
tools/gen_sparse_golden.py).  NumPy / SciPy only: no front end is needed here.

A case names an Op, a pattern, a format and the dense operand's width.  A PATTERN is given for the
compressed view — ``(major, minor)`` with its ``indptr`` over the major axis — and is read as csr
(shape ``(major, minor)``) or csc (shape ``(minor, major)``), so both formats walk the same rows:

* ``lens``: 8 compressed rows of lengths 0, 1, 63, 0, 64, 65, 257, 0 (an empty first, middle and last
  row; one entry; one short of, exactly and one more than a wave; several passes of a wave);
* ``r1`` / ``r65`` / ``r130``: 1, 65 and 130 compressed rows (one workgroup holds 4: a partly filled
  last workgroup, more than one workgroup);
* ``r0`` (no compressed row), ``c0`` (minor extent 0), ``empty`` (3 rows, no entry);
* ``dup``: rows that are not sorted and hold duplicate entries.

Dense widths 1, 2, 3 take the narrow kernels, 64, 65, 130 the wide ones (65 and 130 end in a partly
filled tile; 130 is a second tile in float64), ``vec`` the vector form.

Bars (derived, not measured).  ``indices``, ``indptr``, ``MulSD`` (one rounding), ``SparseFromDense`` and
``DenseFromSparse`` without duplicates are bit-exact.  Every sum of k terms is held, per element, to

    |got - exact| <= (k + 2) eps sum |a| |b|        (k: the longest row the sums run over)

— the classic bound k eps sum|a||b| (1 + O(eps)) of a recursive sum in ANY order, plus one eps for each
of the product and the final rounding.  float32 is judged against the same graph in float64, float64
against the reference's own float64 output at twice the bar (both sides round).
"""
import json
import os

import numpy as np
import scipy.sparse

from aesara_amd.plan import Node, Plan

SPARSE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse")
DTYPES = ("float32", "float64")
FORMATS = ("csr", "csc")
LENS = (0, 1, 63, 0, 64, 65, 257, 0)
PLAN_OPS = {"sdot": "StructuredDot", "dot": "SparseDot", "dotr": "SparseDot", "sdg": "SampledDot",
            "dfs": "DenseFromSparse", "sfd": "SparseFromDense", "sum": "SpSum", "mul": "MulSD"}


# ------------------------------------------------------------------ patterns ----------
def _rows_of_lengths(lens, minor, rng):
    indices = [np.sort(rng.choice(minor, size=n, replace=False)) for n in lens]
    indptr = np.concatenate([[0], np.cumsum(lens)])
    return np.concatenate(indices + [np.zeros(0, int)]).astype("int32"), indptr.astype("int32")


def pattern(name):
    """(indices, indptr, major, minor) of a pattern, int32 arrays."""
    rng = np.random.default_rng({"lens": 1, "r1": 2, "r65": 3, "r130": 4, "dup": 5}.get(name, 0))
    if name == "lens":
        return _rows_of_lengths(LENS, 260, rng) + (len(LENS), 260)
    if name == "r1":
        return _rows_of_lengths([3], 7, rng) + (1, 7)
    if name == "r65":
        return _rows_of_lengths(rng.integers(0, 12, size=65), 40, rng) + (65, 40)
    if name == "r130":
        return _rows_of_lengths(rng.integers(0, 6, size=130), 33, rng) + (130, 33)
    if name == "r0":
        return np.zeros(0, "int32"), np.zeros(1, "int32"), 0, 5
    if name == "c0":
        return np.zeros(0, "int32"), np.zeros(6, "int32"), 5, 0
    if name == "empty":
        return np.zeros(0, "int32"), np.zeros(4, "int32"), 3, 9
    if name == "dup":       # unsorted rows, duplicate entries (column 4 three times in row 0), an empty row
        indices = np.array([4, 1, 4, 0, 4, 5, 2, 2, 3, 0, 5, 5], "int32")
        return indices, np.array([0, 5, 5, 8, 9, 12], "int32"), 5, 6
    raise KeyError(name)


def has_duplicates(name):
    return name == "dup"


def _c(op, pat, fmt, n=None, **kw):
    return dict(op=op, pattern=pat, format=fmt, n=n, **kw)


def _cases():
    c = {}

    def add(name, *a, **kw):
        c[name] = _c(*a, **kw)
    # ---- StructuredDot: sparse x dense matrix
    for fmt in FORMATS:
        add(f"sdot_lens_{fmt}_n1", "sdot", "lens", fmt, 1)
        add(f"sdot_lens_{fmt}_n65", "sdot", "lens", fmt, 65)
        add(f"sdot_r130_{fmt}_n130", "sdot", "r130", fmt, 130)
        add(f"sdot_dup_{fmt}_n3", "sdot", "dup", fmt, 3)
        add(f"sdot_r0_{fmt}_n3", "sdot", "r0", fmt, 3)
        add(f"sdot_c0_{fmt}_n3", "sdot", "c0", fmt, 3)
    add("sdot_lens_csr_n3", "sdot", "lens", "csr", 3)
    add("sdot_r65_csr_n2", "sdot", "r65", "csr", 2)
    add("sdot_r65_csc_n64", "sdot", "r65", "csc", 64)
    add("sdot_r130_csc_n3", "sdot", "r130", "csc", 3)
    add("sdot_r1_csr_n64", "sdot", "r1", "csr", 64)
    add("sdot_empty_csr_n65", "sdot", "empty", "csr", 65)
    add("sdot_empty_csc_n2", "sdot", "empty", "csc", 2)
    add("sdot_dup_csc_n65", "sdot", "dup", "csc", 65)
    add("sdot_r65_csr_n64_bt", "sdot", "r65", "csr", 64, bt=True)       # B handed over as a transposed view
    add("sdot_r65_csc_n65_bt", "sdot", "r65", "csc", 65, bt=True)
    add("sdot_r65_csr_n3_mixed", "sdot", "r65", "csr", 3, mixed=True)   # float32 sparse, float64 dense
    add("sdot_r65_csc_n65_mixed", "sdot", "r65", "csc", 65, mixed=True)
    # ---- Dot: sparse x vector / matrix, dense x sparse
    for fmt in FORMATS:
        add(f"dot_r65_{fmt}_vec", "dot", "r65", fmt, "vec")
        add(f"dot_lens_{fmt}_n2", "dot", "lens", fmt, 2)
        add(f"dotr_r65_{fmt}_n3", "dotr", "r65", fmt, 3)
        add(f"dotr_lens_{fmt}_vec", "dotr", "lens", fmt, "vec")
        add(f"dotr_r130_{fmt}_n65", "dotr", "r130", fmt, 65)
    # ---- StructuredDotGradCSR / CSC: the sampled product
    for fmt in FORMATS:
        add(f"sdg_lens_{fmt}_n3", "sdg", "lens", fmt, 3)
        add(f"sdg_lens_{fmt}_n65", "sdg", "lens", fmt, 65)
        add(f"sdg_dup_{fmt}_n2", "sdg", "dup", fmt, 2)
    add("sdg_r130_csr_n130", "sdg", "r130", "csr", 130)
    add("sdg_r65_csc_n1", "sdg", "r65", "csc", 1)
    add("sdg_r65_csr_n64", "sdg", "r65", "csr", 64)
    add("sdg_empty_csr_n3", "sdg", "empty", "csr", 3)
    # ---- DenseFromSparse, SpSum, MulSD
    for fmt in FORMATS:
        add(f"dfs_lens_{fmt}", "dfs", "lens", fmt)
        add(f"dfs_dup_{fmt}", "dfs", "dup", fmt)
        add(f"dfs_r130_{fmt}", "dfs", "r130", fmt)
        for axis in (0, 1):
            add(f"sum_lens_{fmt}_a{axis}", "sum", "lens", fmt, axis=axis)
        add(f"sum_dup_{fmt}_a1", "sum", "dup", fmt, axis=1)
        add(f"mul_lens_{fmt}", "mul", "lens", fmt)
        add(f"mul_dup_{fmt}", "mul", "dup", fmt)
    add("dfs_r0_csr", "dfs", "r0", "csr")
    add("dfs_c0_csc", "dfs", "c0", "csc")
    add("dfs_empty_csr", "dfs", "empty", "csr")
    add("sum_empty_csr_a0", "sum", "empty", "csr", axis=0)
    add("sum_r130_csr_a0", "sum", "r130", "csr", axis=0)
    add("mul_r65_csr", "mul", "r65", "csr")
    # ---- SparseFromDense: the dense matrix is the pattern's, made dense (plus -0.0 and NaN in `special`)
    for fmt in FORMATS:
        add(f"sfd_r65_{fmt}", "sfd", "r65", fmt)
        add(f"sfd_lens_{fmt}", "sfd", "lens", fmt)
        add(f"sfd_special_{fmt}", "sfd", "dup", fmt, special=True)
    add("sfd_r0_csr", "sfd", "r0", "csr")
    add("sfd_c0_csr", "sfd", "c0", "csr")
    add("sfd_empty_csc", "sfd", "empty", "csc")
    return c


CASES = _cases()


def eps(dtype):
    return float(np.finfo(dtype).eps)


def data_dtype(name, dtype):
    return "float32" if CASES[name].get("mixed") else dtype


def out_dtype(name, dtype):
    return "float64" if CASES[name].get("mixed") else dtype


def case_dtypes(name):
    """The dtypes a case runs in (a mixed case is one case: float32 sparse, float64 dense)."""
    return ("float64",) if CASES[name].get("mixed") else DTYPES


def shape_of(name):
    """(rows, cols) of the case's sparse matrix."""
    c = CASES[name]
    _i, _p, major, minor = pattern(c["pattern"])
    return (major, minor) if c["format"] == "csr" else (minor, major)


def operands(name, dtype):
    """The inputs of a case in plan order.  A sparse operand is data, indices, indptr, rows, cols."""
    c = CASES[name]
    indices, indptr, major, minor = pattern(c["pattern"])
    rows, cols = shape_of(name)
    rng = np.random.default_rng(abs(hash_name(name)) % (2 ** 31))
    data = rng.standard_normal(len(indices)).astype(data_dtype(name, dtype))
    sp = [data, indices, indptr, np.asarray(rows, "int64"), np.asarray(cols, "int64")]
    odt = out_dtype(name, dtype)

    def dense(*shape):
        return rng.standard_normal(shape).astype(odt)
    n, op = c["n"], c["op"]
    if op in ("sdot", "dot"):
        if n == "vec":
            return sp + [dense(cols)]
        return sp + [dense(n, cols) if c.get("bt") else dense(cols, n)]
    if op == "dotr":
        return sp + [dense(rows) if n == "vec" else dense(n, rows)]
    if op == "sdg":
        return sp + [dense(cols, n), dense(rows, n)]          # b, g_ab
    if op == "mul":
        return sp + [dense(rows, cols)]
    if op == "sfd":
        m = to_scipy(sp, c["format"]).toarray().astype(odt)
        if c.get("special"):
            m[0, 0], m[1, 1], m[m.shape[0] - 1, m.shape[1] - 1] = -0.0, np.nan, np.nan
            m[2, 3] = -0.0
        return [m]
    return sp


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % 1000003


def to_scipy(sp, fmt, dtype=None):
    data, indices, indptr, rows, cols = sp
    cls = scipy.sparse.csr_matrix if fmt == "csr" else scipy.sparse.csc_matrix
    # (copies: SciPy sorts and merges a matrix's arrays in place when an operation asks for it)
    return cls((np.array(data, dtype=dtype or data.dtype), np.array(indices), np.array(indptr)),
               shape=(int(rows), int(cols)))


# ------------------------------------------------------------------ bars --------------
def _row_of_entry(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def terms(name, xs):
    """(sum |a| |b| per output element in float64, k = the longest row the sums run over)."""
    c = CASES[name]
    op, fmt = c["op"], c["format"]
    sp = xs[:5]
    indices, indptr = sp[1], sp[2]
    A = abs(to_scipy(sp, fmt, "float64"))
    per_major = int(np.diff(indptr).max()) if len(indptr) > 1 else 0
    per_minor = int(np.bincount(indices, minlength=1).max()) if len(indices) else 0
    per_row, per_col = (per_major, per_minor) if fmt == "csr" else (per_minor, per_major)
    if op in ("sdot", "dot"):
        B = np.abs(xs[5].astype("float64"))
        return np.asarray(A @ (B.T if c.get("bt") else B)), per_row
    if op == "dotr":
        return np.asarray((A.T @ np.abs(xs[5].astype("float64")).T).T), per_col
    if op == "sdg":
        b, g = (np.abs(x.astype("float64")) for x in xs[5:7])
        major_of = _row_of_entry(indptr)
        r, cidx = (major_of, indices) if fmt == "csr" else (indices, major_of)
        return np.sum(g[r] * b[cidx], axis=1), b.shape[1]
    if op == "dfs":
        return A.toarray(), max(per_row, per_col)
    if op == "sum":
        axis = c["axis"]
        return np.asarray(A.sum(axis=axis)).ravel(), per_col if axis == 0 else per_row
    raise KeyError(op)


def exact_case(name):
    c = CASES[name]
    return c["op"] in ("mul", "sfd") or (c["op"] == "dfs" and not has_duplicates(c["pattern"]))


def ratio(name, dtype, got, xs, z):
    """The worst |got - exact| / bar over the elements of the float output (0 where both are 0; inf
    where an element that must be exact is not).  ``z``: the case's stored arrays."""
    got = np.asarray(got)
    if exact_case(name):
        same = got.tobytes() == np.asarray(z["out"]).tobytes() and got.shape == z["out"].shape
        return 0.0 if same else np.inf
    f32 = out_dtype(name, dtype) == "float32"
    exact = z["x64"] if f32 else z["out"]
    absum, k = terms(name, xs)
    bar = (k + 2) * eps(out_dtype(name, dtype)) * absum.reshape(got.shape) * (1.0 if f32 else 2.0)
    err = np.abs(got.astype("float64") - exact.astype("float64"))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------ fixtures ----------
def load_cases():
    with open(os.path.join(SPARSE_GOLDEN, "cases.json")) as f:
        return json.load(f)["cases"]


def case_file(name, dtype):
    return os.path.join(SPARSE_GOLDEN, f"{name}_{dtype}.npz")


def store_inputs(xs):
    """The arrays a case file holds for the plan inputs ``xs``: the sparse operand as ``data`` /
    ``indices`` / ``indptr`` / ``shape``, the dense ones as ``dense0``, ``dense1``."""
    arrays, dense = {}, list(xs)
    if len(xs) >= 5 and xs[1].dtype == np.int32:
        arrays = {"data": xs[0], "indices": xs[1], "indptr": xs[2], "shape": np.array([xs[3], xs[4]], "int64")}
        dense = list(xs[5:])
    arrays.update({f"dense{k}": d for k, d in enumerate(dense)})
    return arrays


def load_inputs(z):
    """The plan's inputs from a stored case."""
    xs = []
    if "data" in z.files:
        xs = [z["data"], z["indices"], z["indptr"], np.asarray(z["shape"][0], "int64"),
              np.asarray(z["shape"][1], "int64")]
    k = 0
    while f"dense{k}" in z.files:
        xs.append(z[f"dense{k}"])
        k += 1
    return xs


# ------------------------------------------------------------------ plans -------------
def _cast(dtype):
    return {"scalar": {"n_in": 1, "nodes": [{"op": "cast", "in": [["i", 0]], "dtype": dtype}], "out": [["t", 0]]}}


def op_plan(name, dtype):
    """The plan a case lowers to (tests/test_sparse_lowering.py holds the linker to it): the Op's node,
    behind a cast of ``data`` (mixed) or a transposing DimShuffle of the dense operand (bt)."""
    c = CASES[name]
    op, fmt = c["op"], c["format"]
    sdt, odt = data_dtype(name, dtype), out_dtype(name, dtype)
    plan = Plan(f"sparse_{name}_{dtype}", {}, [], [], [])
    new = plan.new_var

    def emit(opname, ins, outs, params):
        plan.nodes.append(Node(opname, list(ins), list(outs), params))
    if op == "sfd":
        x = new(odt, [None, None], "w")
        members = [new(odt, [None]), new("int32", [None]), new("int32", [None])]
        emit("SparseFromDense", [x], members, {"format": fmt})
        rows, cols = new("int64", []), new("int64", [])
        emit("Shape_i", [x], [rows], {"i": 0})
        emit("Shape_i", [x], [cols], {"i": 1})
        plan.inputs, plan.outputs = [x], members + [rows, cols]
        plan.sparse = {"inputs": [], "outputs": [[0, fmt, 0]]}
        return plan
    sp = [new(sdt, [None], "x.data"), new("int32", [None], "x.indices"), new("int32", [None], "x.indptr"),
          new("int64", []), new("int64", [])]
    plan.inputs = list(sp)
    plan.sparse = {"inputs": [[0, fmt, 0]], "outputs": []}
    data = sp[0]
    if sdt != odt:
        data = new(odt, [None])
        emit("Elemwise", [sp[0]], [data], _cast(odt))
    named = {"format": fmt, "name": "x"}
    if op in ("sdot", "dot", "dotr"):
        vec = c["n"] == "vec"
        d = new(odt, [None] if vec else [None, None], "w")
        plan.inputs.append(d)
        dd = d
        if c.get("bt"):
            dd = new(odt, [None, None])
            emit("DimShuffle", [d], [dd], {"new_order": [1, 0]})
        out = new(odt, [None] if vec else [None, None])
        emit(PLAN_OPS[op], [data] + sp[1:] + [dd], [out], dict(named, sparse_first=op != "dotr"))
        plan.outputs = [out]
    elif op == "sdg":
        b, g = new(odt, [None, None], "b"), new(odt, [None, None], "g")
        plan.inputs += [b, g]
        out = new(odt, [None])
        emit("SampledDot", [sp[1], sp[2]] + ([g, b] if fmt == "csr" else [b, g]), [out], {"name": "x"})
        plan.outputs = [out]
    elif op == "dfs":
        out = new(odt, [None, None])
        emit("DenseFromSparse", sp, [out], named)
        plan.outputs = [out]
    elif op == "sum":
        out = new(odt, [None])
        emit("SpSum", sp, [out], dict(named, axis=c["axis"]))
        plan.outputs = [out]
    elif op == "mul":
        y = new(odt, [None, None], "y")
        plan.inputs.append(y)
        out = new(odt, [None])
        emit("MulSD", sp + [y], [out], named)
        plan.outputs = [out] + sp[1:]
        plan.sparse["outputs"] = [[0, fmt, 0]]
    return plan


def same_lowering(lowered, built):
    """Whether two plans are the same up to the numbering and the names of their variables: the same
    nodes in the same order, each operand the same input position, constant or earlier result."""
    def describe(plan):
        where = {v: ("in", k) for k, v in enumerate(plan.inputs)}
        out = []
        for ni, n in enumerate(plan.nodes):
            ins = []
            for v in n.inputs:
                var = plan.vars[v]
                src = where.get(v) or (("const", json.dumps(var.const.get("data"))) if var.const else ("?",))
                ins.append((var.dtype, len(var.shape), src))
            for k, o in enumerate(n.outputs):
                where[o] = ("node", ni, k)
            out.append((n.op, json.dumps(n.params, sort_keys=True), ins,
                        [(plan.vars[o].dtype, len(plan.vars[o].shape)) for o in n.outputs]))
        return out, [where.get(v) for v in plan.outputs], plan.sparse
    return describe(lowered) == describe(built)
