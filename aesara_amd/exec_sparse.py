"""The sparse Ops of a PlanExecutor: ``StructuredDot``, ``SparseDot``, ``SampledDot``,
``DenseFromSparse``, ``SparseFromDense``, ``SpSum`` and ``MulSD`` (reference: aesara/sparse/basic.py
:3424 / :3920 / :3558 + :3691 / :945 / :1025 / :1717 / :2327) on the kernels of csrc/sparse.hip.

A sparse value is never one plan variable: a node takes its members ``data, indices, indptr`` and
the two extents ``rows, cols`` (0-d host integers, like ``Shape_i`` results) as ordinary inputs and
names the format in its params.  The kernels only know the CSR view — ``(major, minor)`` is
``(rows, cols)`` for csr and ``(cols, rows)`` for csc, where the view is the transpose — so the
format decides which strides and extents are swapped here, nothing else.

A product along the uncompressed axis (csc x dense, dense x csr) goes through the orientation flip:
the stable argsort of ``indices`` (K13) and ``ahip_csr_flip_finish`` give the permutation, indices and
indptr of the other orientation, and the gather product reads ``data`` through the permutation.
After the flip every sum runs in ascending original position; no float atomics, so three calls give
the same bits.

Errors.  A malformed operand (an index outside the minor extent, a row range outside ``[0, nnz]``)
is recorded by the kernels in the step's error word and the entry is skipped; the executor raises
``ValueError`` naming the operand where it examines error words (exec_replay.py): eager, recorded
or replayed.  Everything but ``SparseFromDense`` (whose output length is read on the host, like
``Nonzero``) records into a launch list.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_linalg.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401

INFO_TAG = 1 << 62            # AHIP_LINALG_INFO_TAG (the tag of every info word)
MALFORMED = 1                 # AHIP_SPARSE_MALFORMED
BAD_INDEX, BAD_INDPTR = 1, 2  # AHIP_SPARSE_BAD_*
FORMATS = ("csr", "csc")
SPARSE_OPS = ("StructuredDot", "SparseDot", "SampledDot", "DenseFromSparse", "SparseFromDense", "SpSum",
              "MulSD")


def is_sparse_code(code):
    """Whether an error word holds the info code of a sparse kernel (the tag bit, kind 1)."""
    return code > 0 and (code >> 34) == (INFO_TAG >> 34) and ((code >> 32) & 3) == MALFORMED


def sparse_error(code, opname=None, operand=None):
    what = {BAD_INDEX: "an index outside the extent it addresses",
            BAD_INDPTR: "an indptr that is not a sequence of ranges 0 <= start <= end <= nnz"}.get(
                code & 0xFFFFFFFF, "malformed members")
    return ValueError(f"{opname or 'sparse Op'}: malformed sparse operand {operand or ''}".rstrip()
                      + f": {what}")


def _t(a: DevArray) -> DevArray:
    return a.view((a.shape[1], a.shape[0]), (a.strides[1], a.strides[0]))


class SparseMixin:

    # ------------------------------------------------------------------ operands ------
    def _sp_members(self, node, args, dtype=None):
        """(data, indices, indptr, rows, cols) of the sparse operand in ``args[:5]``, checked."""
        data, indices, indptr = (self.to_device(a) for a in args[:3])
        rows, cols = self.host_int(args[3]), self.host_int(args[4])
        fmt = node.params["format"]
        if fmt not in FORMATS:
            raise ValueError(f"{node.op}: format {fmt!r} (one of {', '.join(FORMATS)})")
        if dtype is not None and data.dtype != dtype:
            raise TypeError(f"{node.op}: sparse data of dtype {data.dtype} for a {dtype} result")
        if data.dtype not in ("float32", "float64") or indices.dtype != "int32" or indptr.dtype != "int32":
            raise TypeError(f"{node.op}: members of dtypes {data.dtype}, {indices.dtype}, {indptr.dtype} "
                            "(float32 / float64 data with int32 indices and indptr)")
        major = rows if fmt == "csr" else cols
        if data.ndim != 1 or indices.ndim != 1 or indptr.ndim != 1 or rows < 0 or cols < 0 \
                or indices.shape[0] != data.shape[0] or indptr.shape[0] != major + 1:
            raise ValueError(f"{node.op}: members of shapes {tuple(data.shape)}, {tuple(indices.shape)}, "
                             f"{tuple(indptr.shape)} do not make a {fmt} matrix of shape {(rows, cols)}")
        return self.contiguous(data), self.contiguous(indices), self.contiguous(indptr), rows, cols

    def _sp_info(self):
        return _VP(self._bad_ptr())

    # ------------------------------------------------------------------ kernels -------
    def _sp_flip(self, indices: DevArray, indptr: DevArray, major, minor):
        """(perm int64, new indices, new indptr) of the other orientation: minor + 1 row starts."""
        nnz = indices.shape[0]
        perm = self.alloc((nnz,), "int64")
        keys = self.alloc((nnz,), "int32")
        code = dtype_code("int32")
        if nnz > int(lib.ahip_sort_max_row(code)):
            need = int(lib.ahip_sort_large_ws_bytes(code, 1, nnz))
            ws = self.alloc((need,), "uint8")
            self._launch("ahip_sort_rows_large", (code, _VP(indices.ptr), 1, nnz, nnz, 1, _VP(keys.ptr),
                                                  _VP(perm.ptr), _VP(ws.ptr), need, self._stream()))
        elif nnz:
            self._launch("ahip_sort_rows", (code, _VP(indices.ptr), 1, nnz, nnz, 1, _VP(keys.ptr),
                                            _VP(perm.ptr), self._stream()))
        nidx, nptr = self.alloc((nnz,), "int32"), self.alloc((minor + 1,), "int32")
        self._launch("ahip_csr_flip_finish", (major, minor, nnz, _VP(keys.ptr), _VP(perm.ptr), _VP(indptr.ptr),
                                              _VP(nidx.ptr), _VP(nptr.ptr), self._sp_info(), self._stream()))
        return perm, nidx, nptr

    def _sp_spmm(self, data, perm, indices, indptr, major, minor, B: DevArray, out: DevArray):
        """``out[major, n] = S B`` for the CSR view ``S`` and the matrix view ``B[minor, n]``."""
        n = B.shape[1]
        if major == 0 or n == 0:
            return
        self._launch("ahip_csr_spmm", (dtype_code(data.dtype), major, minor, n, data.shape[0], _VP(data.ptr),
                                       _VP(perm.ptr) if perm is not None else None, _VP(indices.ptr),
                                       _VP(indptr.ptr), _VP(B.ptr), B.strides[0], B.strides[1], _VP(out.ptr),
                                       out.strides[0], out.strides[1], self._sp_info(), self._stream()))

    def _sp_rows_view(self, fmt, want_rows, data, indices, indptr, rows, cols):
        """The CSR view whose major axis is the matrix's rows (``want_rows``) or its columns:
        (data, perm, indices, indptr, major, minor) — as stored, or through the flip."""
        major, minor = (rows, cols) if fmt == "csr" else (cols, rows)
        if (fmt == "csr") == want_rows:
            return data, None, indices, indptr, major, minor
        perm, nidx, nptr = self._sp_flip(indices, indptr, major, minor)
        return data, perm, nidx, nptr, minor, major

    # ------------------------------------------------------------------ the Ops -------
    def _sp_dot(self, node, args):
        """inputs (data, indices, indptr, rows, cols, dense); ``sparse_first``: S . dense, else dense . S;
        the dense operand is a matrix or a vector."""
        dt = self.plan.vars[node.outputs[0]].dtype
        data, indices, indptr, rows, cols = self._sp_members(node, args, dt)
        d = self.to_device(args[5])
        if d.dtype != dt or d.ndim not in (1, 2):
            raise TypeError(f"{node.op}: a dense operand of dtype {d.dtype} and rank {d.ndim} for a {dt} result")
        first = bool(node.params["sparse_first"])
        inner_s = cols if first else rows
        inner_d = d.shape[0] if first else d.shape[-1]
        if inner_s != inner_d:
            shapes = ((rows, cols), tuple(d.shape)) if first else (tuple(d.shape), (rows, cols))
            if node.op == "StructuredDot":
                raise ValueError("shape mismatch in StructuredDot.perform", shapes)
            raise ValueError(f"dimension mismatch: shapes {shapes[0]} and {shapes[1]}")
        vec = d.ndim == 1
        if first:
            B = d.view((d.shape[0], 1), (d.strides[0], 0)) if vec else d
            out = self.alloc((rows,) if vec else (rows, B.shape[1]), dt)
            O = out.view((rows, 1), (1, 0)) if vec else out
        else:       # out = d S  <=>  out^T = S^T d^T: the view whose major axis is S's columns
            B = d.view((d.shape[0], 1), (d.strides[0], 0)) if vec else _t(d)
            out = self.alloc((cols,) if vec else (d.shape[0], cols), dt)
            O = out.view((cols, 1), (1, 0)) if vec else _t(out)
        view = self._sp_rows_view(node.params["format"], first, data, indices, indptr, rows, cols)
        self._sp_spmm(*view, B, O)
        return [out]

    def _op_StructuredDot(self, node, args):
        """reference: sparse/basic.py:3448 StructuredDot.perform (``a * b``, SciPy's csr_matvecs)."""
        return self._sp_dot(node, args)

    def _op_SparseDot(self, node, args):
        """reference: sparse/basic.py:3991 Dot.perform (``x * y`` with one sparse operand)."""
        return self._sp_dot(node, args)

    def _op_SampledDot(self, node, args):
        """reference: sparse/basic.py:3712 StructuredDotGradCSR.perform / :3579 ...CSC.perform:
        inputs (indices, indptr, G, B) of the CSR view; out[k] = G[major(k)] . B[indices[k]]."""
        dt = self.plan.vars[node.outputs[0]].dtype
        indices, indptr = (self.contiguous(self.to_device(a)) for a in args[:2])
        G, B = self.to_device(args[2]), self.to_device(args[3])
        if G.dtype != dt or B.dtype != dt or dt not in ("float32", "float64") or G.ndim != 2 or B.ndim != 2:
            raise TypeError(f"{node.op}: dense operands of dtypes {G.dtype}, {B.dtype} for a {dt} result")
        if indices.dtype != "int32" or indptr.dtype != "int32" or indptr.shape[0] < 1:
            raise TypeError(f"{node.op}: int32 indices and indptr (got {indices.dtype}, {indptr.dtype})")
        major, minor, nnz = indptr.shape[0] - 1, B.shape[0], indices.shape[0]
        if G.shape[0] != major or G.shape[1] != B.shape[1]:
            raise ValueError(f"{node.op}: dense operands of shapes {tuple(G.shape)} and {tuple(B.shape)} for a "
                             f"pattern of {major} compressed rows")
        out = self.alloc((nnz,), dt)
        if nnz and major:
            self._launch("ahip_csr_sddmm", (dtype_code(dt), major, minor, G.shape[1], nnz, _VP(indices.ptr),
                                            _VP(indptr.ptr), _VP(G.ptr), G.strides[0], G.strides[1], _VP(B.ptr),
                                            B.strides[0], B.strides[1], _VP(out.ptr), self._sp_info(),
                                            self._stream()))
        return [out]

    def _op_DenseFromSparse(self, node, args):
        """reference: sparse/basic.py:986 DenseFromSparse.perform (``x.toarray()``: duplicates add)."""
        dt = self.plan.vars[node.outputs[0]].dtype
        data, indices, indptr, rows, cols = self._sp_members(node, args, dt)
        out = self.alloc((rows, cols), dt)
        self.fill_zero(out)
        D = out if node.params["format"] == "csr" else _t(out)
        if D.shape[0] and D.shape[1]:
            self._launch("ahip_csr_to_dense", (dtype_code(dt), D.shape[0], D.shape[1], data.shape[0], _VP(data.ptr),
                                               _VP(indices.ptr), _VP(indptr.ptr), _VP(D.ptr), D.strides[0],
                                               D.strides[1], self._sp_info(), self._stream()))
        return [out]

    def _op_SparseFromDense(self, node, args):
        """reference: sparse/basic.py:1068 SparseFromDense.perform (``csr_matrix(x)`` / ``csc_matrix(x)``:
        the entries with value != 0 in row-major / column-major order).  Outputs (data, indices,
        indptr); the output length is read on the host, so a plan with this Op is not replayed."""
        x = self.to_device(args[0])
        dt = self.plan.vars[node.outputs[0]].dtype
        if x.ndim != 2 or x.dtype != dt or dt not in ("float32", "float64"):
            raise TypeError(f"{node.op}: a {x.dtype} operand of rank {x.ndim} for {dt} data")
        D = x if node.params["format"] == "csr" else _t(x)
        major, minor = D.shape
        indptr = self.alloc((major + 1,), "int32")
        counts = self.alloc((major + 1,), "int32")
        self.fill_zero(counts.view((1,), (1,)))
        code = dtype_code(dt)
        if major:
            self._launch("ahip_dense_count_rows", (code, major, minor, _VP(D.ptr), D.strides[0], D.strides[1],
                                                   _VP(counts.view((major,), (1,), counts.offset + 1).ptr),
                                                   self._stream()))
        need = int(lib.ahip_cumulative_ws_bytes(dtype_code("int32"), 1, major + 1, 1))
        ws = self.alloc((need,), "uint8") if need else None
        self._launch("ahip_cumulative", (dtype_code("int32"), 0, _VP(counts.ptr), 1, major + 1, 1, 0, 1, 0,
                                         _VP(indptr.ptr), _VP(ws.ptr) if ws is not None else None, need,
                                         self._stream()))
        if self.dry_run:
            nnz = major * minor     # value unknown in a dry run: the largest possible count
        else:
            nnz = int(self.host_array(indptr.view((1,), (1,), indptr.offset + major))[0])
        data, indices = self.alloc((nnz,), dt), self.alloc((nnz,), "int32")
        if nnz and major:
            self._launch("ahip_dense_fill_csr", (code, major, minor, nnz, _VP(D.ptr), D.strides[0], D.strides[1],
                                                 _VP(indptr.ptr), _VP(data.ptr), _VP(indices.ptr), self._stream()))
        return [data, indices, indptr]

    def _op_SpSum(self, node, args):
        """reference: sparse/basic.py:1748 SpSum.perform (``x.sum(axis)``): the gather product with a
        vector of ones read through a zero stride — a row's sum in the product's fixed order."""
        dt = self.plan.vars[node.outputs[0]].dtype
        data, indices, indptr, rows, cols = self._sp_members(node, args, dt)
        axis = node.params["axis"]
        if axis not in (0, 1):
            raise ValueError(f"{node.op}: axis {axis!r} (0 or 1; the full sum is a reduction over data)")
        view = self._sp_rows_view(node.params["format"], axis == 1, data, indices, indptr, rows, cols)
        major, minor = view[4], view[5]
        out = self.alloc((major,), dt)
        ones = self._one(dt).view((minor, 1), (0, 0))
        self._sp_spmm(*view, ones, out.view((major, 1), (1, 0)))
        return [out]

    def _op_MulSD(self, node, args):
        """reference: sparse/basic.py:2348 MulSD.perform with a matrix ``y`` of the same shape:
        out_data[k] = data[k] * y[row(k), col(k)], the pattern unchanged."""
        dt = self.plan.vars[node.outputs[0]].dtype
        data, indices, indptr, rows, cols = self._sp_members(node, args, dt)
        y = self.to_device(args[5])
        if y.dtype != dt or y.ndim != 2:
            raise TypeError(f"{node.op}: a dense operand of dtype {y.dtype} and rank {y.ndim} for {dt} data")
        if tuple(y.shape) != (rows, cols):
            raise ValueError(f"{node.op}: shapes {(rows, cols)} and {tuple(y.shape)} differ")
        D = y if node.params["format"] == "csr" else _t(y)
        out = self.alloc(data.shape, dt)
        if data.shape[0] and D.shape[0]:
            self._launch("ahip_csr_mul_dense", (dtype_code(dt), D.shape[0], D.shape[1], data.shape[0],
                                                _VP(data.ptr), _VP(indices.ptr), _VP(indptr.ptr), _VP(D.ptr),
                                                D.strides[0], D.strides[1], _VP(out.ptr), self._sp_info(),
                                                self._stream()))
        return [out]
