"""Sparse values at the boundary of a HIP-linked function.

Inside a plan a sparse value is five ordinary variables (lower_sparse.py): ``data``, ``indices``,
``indptr`` and the two extents.  This module takes a SciPy ``csr_matrix`` / ``csc_matrix`` or a
:class:`DeviceSparse` argument apart in front of the executor call and puts sparse results together
again behind it, following ``Plan.sparse``.

The members of a SciPy matrix are attributes of the matrix (the same ndarray objects on every
call), so the executor's replay memo on argument identity keeps working; a :class:`DeviceSparse`
holds three device tensors, so the design matrix of a training loop is uploaded once.

No front end is needed here: the module also runs on a box without Aesara.
"""
from __future__ import annotations

import numpy as np
import torch

FORMATS = ("csr", "csc")
FLOATS = ("float32", "float64")


class DeviceSparse:
    """A CSR / CSC matrix whose ``data`` (float32 / float64), ``indices`` and ``indptr`` (int32) are
    torch tensors, usually on the device; ``shape`` is a pair of Python integers."""
    __slots__ = ("format", "data", "indices", "indptr", "shape", "_ext")

    def __init__(self, format, data, indices, indptr, shape):
        if format not in FORMATS:
            raise TypeError(f"DeviceSparse: format {format!r} (one of {', '.join(FORMATS)})")
        for name, t in (("data", data), ("indices", indices), ("indptr", indptr)):
            if not isinstance(t, torch.Tensor) or t.ndim != 1:
                raise TypeError(f"DeviceSparse: {name} must be a 1-d torch tensor")
        if str(data.dtype).replace("torch.", "") not in FLOATS:
            raise TypeError(f"DeviceSparse: data of dtype {data.dtype} (float32 / float64 only)")
        for name, t in (("indices", indices), ("indptr", indptr)):
            if t.dtype != torch.int32:
                raise TypeError(f"DeviceSparse: {name} of dtype {t.dtype}: 64-bit (or other) index arrays are "
                                "not supported, int32 only")
        rows, cols = (int(s) for s in shape)
        major = rows if format == "csr" else cols
        if rows < 0 or cols < 0 or indices.shape[0] != data.shape[0] or indptr.shape[0] != major + 1:
            raise ValueError(f"DeviceSparse: members of lengths {data.shape[0]}, {indices.shape[0]}, "
                             f"{indptr.shape[0]} do not make a {format} matrix of shape {(rows, cols)}")
        self.format, self.data, self.indices, self.indptr = format, data, indices, indptr
        self.shape = (rows, cols)
        # (the extents as the SAME 0-d arrays on every call: host integers of the plan)
        self._ext = (np.asarray(rows, dtype="int64"), np.asarray(cols, dtype="int64"))

    @property
    def dtype(self):
        return str(self.data.dtype).replace("torch.", "")

    @property
    def nnz(self):
        return int(self.data.shape[0])

    @classmethod
    def from_scipy(cls, m, device=None):
        fmt, members = split_scipy(m)
        data, indices, indptr = (torch.from_numpy(np.ascontiguousarray(a)) for a in members[:3])
        if device is not None:
            data, indices, indptr = data.to(device), indices.to(device), indptr.to(device)
        return cls(fmt, data, indices, indptr, m.shape)

    def to_scipy(self):
        import scipy.sparse
        cls = scipy.sparse.csr_matrix if self.format == "csr" else scipy.sparse.csc_matrix
        parts = tuple(t.detach().cpu().numpy() for t in (self.data, self.indices, self.indptr))
        return cls(parts, shape=self.shape)

    def members(self):
        return [self.data, self.indices, self.indptr, self._ext[0], self._ext[1]]

    def __repr__(self):
        return f"<DeviceSparse {self.format} {self.dtype}{list(self.shape)}, {self.nnz} stored on {self.data.device}>"


def is_scipy_sparse(x):
    return hasattr(x, "getnnz") and hasattr(x, "indptr") and hasattr(x, "format")


def split_scipy(m):
    """(format, [data, indices, indptr, rows, cols]) of a SciPy csr / csc matrix; the arrays are the
    matrix's own attributes.  64-bit index arrays are refused: SciPy narrows them whenever the
    extents and the number of entries allow it."""
    if not is_scipy_sparse(m) or m.format not in FORMATS:
        raise TypeError(f"expected a scipy.sparse csr_matrix / csc_matrix, got {type(m).__name__}"
                        + (f" of format {m.format}" if hasattr(m, "format") else ""))
    if m.indices.dtype != np.int32 or m.indptr.dtype != np.int32:
        raise TypeError(f"sparse argument with {m.indices.dtype} / {m.indptr.dtype} index arrays: 64-bit index "
                        "arrays are not supported, int32 only")
    return m.format, [m.data, m.indices, m.indptr, np.asarray(m.shape[0], dtype="int64"),
                      np.asarray(m.shape[1], dtype="int64")]


def check_argument(value, fmt, dtype, what="sparse argument"):
    """A sparse argument of a function whose graph input is ``fmt`` / ``dtype``: a DeviceSparse or a SciPy
    matrix of that format and data dtype with int32 index arrays (what ``SparseTensorType.filter``
    checks in strict mode, sparse/type.py:98, without converting anything)."""
    if isinstance(value, DeviceSparse):
        got = (value.format, value.dtype)
    elif is_scipy_sparse(value):
        split_scipy(value)
        got = (value.format, value.dtype.name)
    else:
        raise TypeError(f"{what}: expected a scipy.sparse matrix or a DeviceSparse, got {type(value).__name__}")
    if got != (fmt, dtype):
        raise TypeError(f"{what}: a {got[0]} matrix with {got[1]} data where the graph has {fmt} / {dtype}")
    return value


def expand_args(args, spec):
    """The executor's argument list: every sparse argument replaced by its five members.
    ``spec`` = ``Plan.sparse["inputs"]``: [[graph position, format, first plan position], ...]."""
    fmts = {k: fmt for k, fmt, _p in spec}
    out = []
    for k, a in enumerate(args):
        if k not in fmts:
            out.append(a)
            continue
        if isinstance(a, DeviceSparse):
            if a.format != fmts[k]:
                raise TypeError(f"sparse argument {k}: a {a.format} matrix where the graph has {fmts[k]}")
            out.extend(a.members())
        else:
            fmt, members = split_scipy(a)
            if fmt != fmts[k]:
                raise TypeError(f"sparse argument {k}: a {fmt} matrix where the graph has {fmts[k]}")
            out.extend(members)
    return out


def collect_results(res, spec, n_outputs):
    """The graph's outputs from the executor's: five results from ``first plan position`` on become
    one :class:`DeviceSparse` (``spec`` = ``Plan.sparse["outputs"]``); what follows the graph's own
    outputs (hidden write-back results) is appended as it is."""
    starts = {p: (k, fmt) for k, fmt, p in spec}
    out, p = [], 0
    while len(out) < n_outputs:
        if p in starts:
            data, indices, indptr, rows, cols = res[p:p + 5]
            out.append(DeviceSparse(starts[p][1], _tensor(data), _tensor(indices), _tensor(indptr),
                                    (int(np.asarray(_host(rows))), int(np.asarray(_host(cols))))))
            p += 5
        else:
            out.append(res[p])
            p += 1
    return out + list(res[p:])


def _tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
