"""Lowering of ``aesara/sparse``: CSR / CSC operands with float32 / float64 data.

A sparse variable never becomes one plan variable.  While a graph is lowered it is a
:class:`SparseRec` in ``ctx.sparse``: the format and five ordinary plan variables — ``data``
(``[nnz]``), ``indices`` and ``indptr`` (int32) and the two extents as 0-d host integers, like
``Shape_i`` results.  A sparse graph input contributes those five as plan inputs, a sparse graph
output as plan outputs, a ``SparseConstant`` as plan constants; ``Plan.sparse`` says which positions
belong together (aesara_amd/sparse.py puts them together again at the boundary).

* relabelling only, no node: ``CSMProperties``, ``CSM``, ``Transpose`` (csr <-> csc with the extents
  swapped), ``Shape_i`` of a sparse variable; ``Shape`` / ``csm_shape`` are one host ``MakeVector``;
* Elemwise on ``data``: ``Neg``, ``MulSD`` with a 0-d operand, ``SpSum`` over everything (a
  ``CAReduce``); ``structured_*`` Ops are Elemwise on ``csm_data`` in the graph already;
* kernels (csrc/sparse.hip, exec_sparse.py): ``StructuredDot`` and ``Dot`` with one sparse and one dense
  operand (plan ops ``StructuredDot`` / ``SparseDot``), ``StructuredDotGradCSR`` / ``...CSC`` (plan op
  ``SampledDot`` on the CSR view), ``DenseFromSparse``, ``SparseFromDense``, ``SpSum`` along an axis,
  ``MulSD`` with a matrix.

Mixed float32 / float64 operands go to the dtype ``make_node`` declared through the cast Elemwise,
as the reference's ``perform`` does through SciPy's upcast.

Refused by name: ``bsr``, integer / complex / float16 data, every Op with two sparse operands, and
every Op without a handler here (``AddSD``, ``MulSV``, ``SamplingDot``, ``Usmm``, ``HStack``, ``GetItem*``,
``Remove0``, ``Cast``, ``TrueDot`` ...), in the wording of ``lower_linalg.family``.

Registered by ``lower._register_handlers``; every handler cites the reference Op it restates
(line numbers: aesara/sparse/basic.py).
"""
from dataclasses import dataclass

import numpy as np

from .lower_linalg import family
from .plan import Node

FLOATS = ("float32", "float64")
FORMATS = ("csr", "csc")


@dataclass
class SparseRec:
    format: str
    dtype: str
    data: int
    indices: int
    indptr: int
    rows: int
    cols: int
    name: str

    def members(self):
        return [self.data, self.indices, self.indptr, self.rows, self.cols]


def is_sparse(v):
    return hasattr(v.type, "format") and type(v.type).__name__.startswith("Sparse")


def _check_type(t, unsupported, what):
    if t.format not in FORMATS or str(t.dtype) not in FLOATS:
        raise unsupported(f"{family(what)} for a sparse value of format {t.format} and dtype {t.dtype} "
                          f"(csr / csc with float32 / float64 data only)")


def new_input(ctx, v, k, unsupported):
    """The record of a sparse graph input: five new plan variables."""
    _check_type(v.type, unsupported, f"SparseTensorType{{{v.type.format},{v.type.dtype}}}")
    new = ctx.plan.new_var
    name = getattr(v, "name", None)
    rec = SparseRec(v.type.format, str(v.type.dtype),
                    new(v.type.dtype, [None], name and name + ".data"), new("int32", [None], name and name + ".indices"),
                    new("int32", [None], name and name + ".indptr"), new("int64", [], None), new("int64", [], None),
                    name or f"input {k}")
    ctx.sparse[v] = rec
    return rec


def record(ctx, v, unsupported):
    """The record of a sparse variable; a ``SparseConstant`` becomes plan constants here."""
    from aesara.graph.basic import Constant
    rec = ctx.sparse.get(v)
    if rec is None and isinstance(v, Constant) and is_sparse(v):
        _check_type(v.type, unsupported, "SparseConstant")
        m = v.data
        if m.format not in FORMATS:
            raise unsupported(f"{family('SparseConstant')} for format {m.format}")
        if m.indices.dtype != np.int32 or m.indptr.dtype != np.int32:
            raise unsupported(f"{family('SparseConstant')} for {m.indices.dtype} index arrays (int32 only)")
        c = ctx.plan.add_const
        rec = ctx.sparse[v] = SparseRec(
            m.format, str(v.type.dtype), c(np.asarray(m.data), str(v.type.dtype)), c(m.indices, "int32"),
            c(m.indptr, "int32"), c(int(m.shape[0]), "int64"), c(int(m.shape[1]), "int64"),
            getattr(v, "name", None) or "constant")
        for vid in rec.members()[:3]:           # (a vector of one entry is not broadcastable here)
            ctx.plan.vars[vid].shape = [None]
    if rec is None:
        raise KeyError(f"sparse variable {v} not produced by any lowered node")
    return rec


def register(hip_lower, static_shape, UnsupportedOp):                       # noqa: N803
    from aesara.compile.ops import DeepCopyOp, ViewOp
    from aesara.graph.basic import Constant
    from aesara.sparse import basic as S
    from aesara.tensor.shape import Shape, Shape_i

    from .lower_more import _B

    def rec_of(ctx, v):
        return record(ctx, v, UnsupportedOp)

    def out_rec(ctx, v, opname, fmt, data, indices, indptr, rows, cols, name):
        _check_type(v.type, UnsupportedOp, opname)
        if v.type.format != fmt:                                            # pragma: no cover
            raise UnsupportedOp(f"{family(opname)}: a {fmt} record for a {v.type.format} variable")
        ctx.sparse[v] = SparseRec(fmt, str(v.type.dtype), data, indices, indptr, rows, cols, name)
        return ctx.sparse[v]

    def dense_only(op, v):
        if is_sparse(v):
            raise UnsupportedOp(f"{family(type(op).__name__)} for two sparse operands (one sparse, one dense "
                                "only)")

    def float_out(op, node):
        odt = str(node.outputs[0].type.dtype)
        dts = [str(i.type.dtype) for i in node.inputs]
        if odt not in FLOATS:
            raise UnsupportedOp(f"{family(type(op).__name__)} for operands of dtypes {dts} giving {odt} "
                                "(float32 / float64 only)")
        return odt

    def shape_vector(ctx, rows, cols, dtype):
        return ctx.raw("MakeVector", [rows, cols], dtype, [2], {"dtype": dtype})

    # ---- relabelling -----------------------------------------------------------------------------
    @hip_lower.register(S.CSMProperties)
    def _(op, node, ctx):
        # reference: :529 CSMProperties (perform :585: views of x.data, x.indices, x.indptr and a
        # new array of x.shape) — the record's members; the shape vector only if something reads it
        r = rec_of(ctx, node.inputs[0])
        d, i, p, shp = node.outputs
        ctx.vmap[d], ctx.vmap[i], ctx.vmap[p] = r.data, r.indices, r.indptr
        ctx.sparse_shape[shp] = (r.rows, r.cols)
        ctx.lazy[shp] = lambda: shape_vector(ctx, r.rows, r.cols, str(shp.type.dtype))

    @hip_lower.register(S.CSM)
    def _(op, node, ctx):
        # reference: :648 CSM (perform :725: csr_matrix / csc_matrix((data, indices, indptr), shape),
        # a view of its members) — a new record over the same variables
        data, indices, indptr, shape = node.inputs
        b = _B(ctx, static_shape, UnsupportedOp)
        ext = ctx.sparse_shape.get(shape)
        if ext is None and isinstance(shape, Constant):
            ext = tuple(b.const(int(s), "int64") for s in np.asarray(shape.data).reshape(-1)[:2])
        if ext is None:
            sv = ctx.vid(shape)
            ext = tuple(ctx.raw("Subtensor", [sv], str(shape.type.dtype), [], {"idx_list": [{"index": k}]})
                        for k in (0, 1))
        out_rec(ctx, node.outputs[0], "CSM", op.format, ctx.vid(data), b.cast(ctx.vid(indices), "int32"),
                b.cast(ctx.vid(indptr), "int32"), ext[0], ext[1], node.outputs[0].name or "CSM result")

    @hip_lower.register(S.Transpose)
    def _(op, node, ctx):
        # reference: :1461 Transpose (perform :1502 x.transpose(): the same arrays read as the other
        # format, extents swapped)
        r = rec_of(ctx, node.inputs[0])
        out_rec(ctx, node.outputs[0], "Transpose", op.format_map[r.format], r.data, r.indices, r.indptr,
                r.cols, r.rows, r.name)

    def sparse_aware(cls, build):
        """Let the handler of a dense Op class see sparse operands first."""
        dense = hip_lower.dispatch(cls)

        @hip_lower.register(cls)
        def _(op, node, ctx):
            if is_sparse(node.inputs[0]):
                return build(op, node, ctx, rec_of(ctx, node.inputs[0]))
            return dense(op, node, ctx)

    def _shape_i(op, node, ctx, r):
        # reference: tensor/shape.py:189 Shape_i of a sparse matrix: the record's extent
        ctx.vmap[node.outputs[0]] = (r.rows, r.cols)[int(op.i)]

    def _shape(op, node, ctx, r):
        ctx.vmap[node.outputs[0]] = shape_vector(ctx, r.rows, r.cols, "int64")

    def _view(op, node, ctx, r):
        # compile/ops.py:54 ViewOp: the same record
        ctx.sparse[node.outputs[0]] = r

    def _deepcopy(op, node, ctx, r):
        # compile/ops.py:149 DeepCopyOp (a sparse output that is an input): copies of the members
        cp = [ctx.raw("DeepCopyOp", [v], ctx.plan.vars[v].dtype, [None]) for v in r.members()[:3]]
        ctx.sparse[node.outputs[0]] = SparseRec(r.format, r.dtype, cp[0], cp[1], cp[2], r.rows, r.cols, r.name)

    sparse_aware(Shape_i, _shape_i)
    sparse_aware(Shape, _shape)
    sparse_aware(ViewOp, _view)
    sparse_aware(DeepCopyOp, _deepcopy)

    # ---- Elemwise on data ------------------------------------------------------------------------
    @hip_lower.register(S.Neg)
    def _(op, node, ctx):
        # reference: :1521 Neg (perform :1548 ``-x``): the pattern unchanged
        r = rec_of(ctx, node.inputs[0])
        b = _B(ctx, static_shape, UnsupportedOp)
        data = b.ew([r.data], r.dtype, [None], [("neg", r.dtype, [["i", 0]])])
        out_rec(ctx, node.outputs[0], "Neg", r.format, data, r.indices, r.indptr, r.rows, r.cols, r.name)

    # ---- products --------------------------------------------------------------------------------
    def product(opname, op, node, ctx):
        x, y = node.inputs
        if is_sparse(x) and is_sparse(y):
            dense_only(op, y)
        first = is_sparse(x)
        sp, dense = (x, y) if first else (y, x)
        odt = float_out(op, node)
        r = rec_of(ctx, sp)
        b = _B(ctx, static_shape, UnsupportedOp)
        ins = [b.cast(r.data, odt), r.indices, r.indptr, r.rows, r.cols, b.cast(ctx.vid(dense), odt)]
        ctx.plan.nodes.append(Node(opname, ins, [ctx.new(node.outputs[0])],
                                   {"format": r.format, "sparse_first": first, "name": r.name}))

    @hip_lower.register(S.StructuredDot)
    def _(op, node, ctx):
        # reference: :3424 StructuredDot (make_node :3435 upcasts; perform :3448 ``a * b`` and the
        # ValueError("shape mismatch in StructuredDot.perform", ...) for a.shape[1] != b.shape[0])
        product("StructuredDot", op, node, ctx)

    @hip_lower.register(S.Dot)
    def _(op, node, ctx):
        # reference: :3920 Dot (make_node :3939: one operand sparse, the other a matrix or a vector;
        # perform :3991 ``x * y``; output shapes infer_shape :3926)
        product("SparseDot", op, node, ctx)

    def sampled(op, node, ctx, g_first):
        a_indices, a_indptr, bmat, g_ab = node.inputs
        for v in (bmat, g_ab):
            dense_only(op, v)
        odt = float_out(op, node)
        b = _B(ctx, static_shape, UnsupportedOp)
        bv, gv = b.cast(ctx.vid(bmat), odt), b.cast(ctx.vid(g_ab), odt)
        G, Bm = (gv, bv) if g_first else (bv, gv)
        ins = [b.cast(ctx.vid(a_indices), "int32"), b.cast(ctx.vid(a_indptr), "int32"), G, Bm]
        ctx.plan.nodes.append(Node("SampledDot", ins, [ctx.new(node.outputs[0])],
                                   {"name": getattr(a_indices.owner and a_indices.owner.inputs[0], "name", None)
                                    or "pattern"}))

    @hip_lower.register(S.StructuredDotGradCSR)
    def _(op, node, ctx):
        # reference: :3691 StructuredDotGradCSR (perform :3712: g_a_data[k] = g_ab[row(k)] . b[indices[k]])
        sampled(op, node, ctx, True)

    @hip_lower.register(S.StructuredDotGradCSC)
    def _(op, node, ctx):
        # reference: :3558 StructuredDotGradCSC (perform :3579: g_a_data[k] = g_ab[indices[k]] . b[col(k)]):
        # on the CSR view of the transpose the compressed axis selects the rows of b
        sampled(op, node, ctx, False)

    # ---- conversions, sums, MulSD ----------------------------------------------------------------
    @hip_lower.register(S.DenseFromSparse)
    def _(op, node, ctx):
        # reference: :945 DenseFromSparse (perform :986 ``x.toarray()``: duplicate entries add)
        r = rec_of(ctx, node.inputs[0])
        ctx.plan.nodes.append(Node("DenseFromSparse", r.members(), [ctx.new(node.outputs[0])],
                                   {"format": r.format, "name": r.name}))

    @hip_lower.register(S.SparseFromDense)
    def _(op, node, ctx):
        # reference: :1025 SparseFromDense (perform :1068 csr_matrix(x) / csc_matrix(x): the entries
        # with value != 0, row-major / column-major, int32 index arrays)
        x = node.inputs[0]
        out = node.outputs[0]
        _check_type(out.type, UnsupportedOp, "SparseFromDense")
        if x.type.ndim != 2 or str(x.type.dtype) != str(out.type.dtype):                 # pragma: no cover
            raise UnsupportedOp(f"{family('SparseFromDense')} for a {x.type} operand")
        b = _B(ctx, static_shape, UnsupportedOp)
        xv = ctx.vid(x)
        data, indices, indptr = b.multi("SparseFromDense", [xv], [(str(out.type.dtype), [None]), ("int32", [None]),
                                                                ("int32", [None])], {"format": op.format})
        rows = ctx.raw("Shape_i", [xv], "int64", [], {"i": 0})
        cols = ctx.raw("Shape_i", [xv], "int64", [], {"i": 1})
        out_rec(ctx, out, "SparseFromDense", op.format, data, indices, indptr, rows, cols,
                out.name or "SparseFromDense result")

    @hip_lower.register(S.SpSum)
    def _(op, node, ctx):
        # reference: :1717 SpSum (perform :1748 ``x.sum()`` / ``x.sum(axis)``; shapes (), (cols,), (rows,))
        r = rec_of(ctx, node.inputs[0])
        if op.axis is None:
            ctx.vmap[node.outputs[0]] = ctx.raw("CAReduce", [r.data], r.dtype, [],
                                                {"scalar_op": "add", "axis": [0], "acc_dtype": r.dtype})
            return
        ctx.plan.nodes.append(Node("SpSum", r.members(), [ctx.new(node.outputs[0])],
                                   {"format": r.format, "axis": int(op.axis), "name": r.name}))

    @hip_lower.register(S.MulSD)
    def _(op, node, ctx):
        # reference: :2327 MulSD (make_node :2338 upcasts; perform :2348: a 0-d ``y`` scales ``data``, a
        # matrix of the same shape multiplies entry by entry; the pattern is unchanged)
        x, y = node.inputs
        dense_only(op, y)
        out = node.outputs[0]
        _check_type(out.type, UnsupportedOp, "MulSD")
        odt = str(out.type.dtype)
        r = rec_of(ctx, x)
        b = _B(ctx, static_shape, UnsupportedOp)
        data, yv = b.cast(r.data, odt), b.cast(ctx.vid(y), odt)
        if y.type.ndim == 0:
            new = b.ew([data, yv], odt, [None], [("mul", odt, [["i", 0], ["i", 1]])])
        elif y.type.ndim == 2:
            new = ctx.raw("MulSD", [data, r.indices, r.indptr, r.rows, r.cols, yv], odt, [None],
                          {"format": r.format, "name": r.name})
        else:
            raise UnsupportedOp(f"{family('MulSD')} for a dense operand of rank {y.type.ndim} (0 or 2)")
        out_rec(ctx, out, "MulSD", r.format, new, r.indices, r.indptr, r.rows, r.cols, r.name)
