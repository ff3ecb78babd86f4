"""The dense solves of a PlanExecutor: ``SolveTriangular``, ``CholeskySolve``, ``Solve``,
``MatrixInverse`` and ``Det`` (reference: tensor/slinalg.py :280 / :130 / :365, tensor/nlinalg.py
:100 / :196) on the kernels of csrc/linalg.hip plus ``ahip_gemm`` / ``ahip_gemv``.

The block loops live here.  A triangular solve walks the diagonal in blocks of ``NB`` rows: the
substitution on the diagonal block (``ahip_trsm_diag``), then ``X_rest -= T_rest,k X_k`` as a product
on sub-blocks (pointer offset, the same strides, alpha = -1, beta = 1, in place).  The LU is
right-looking: per ``NB``-wide panel the one-workgroup panel kernel, the row interchanges left and
right of it, the unit-lower solve for ``U12`` and the product ``A22 -= L21 U12``.  Nothing reads a
pivot or an info word on the host while a call runs, so the whole sequence records into a launch
list; workspaces (the LU copy, the pivots) are ordinary allocations whose sizes come from the shapes,
so the replay arena owns them.

Errors.  Every node has one info word (the step's error word, ``OpsMixin._bad_ptr``); the kernels
record a zero diagonal / pivot or a non-finite operand there and the executor raises where it
examines error words (exec_replay.py): in the call that computed them, eager, recorded or replayed.

``assume_a`` = sym / her / pos read the triangle ``lower`` names, complete the copy from it and go
through the same LU: a ``pos`` matrix that is not positive definite is SOLVED, not refused (the one
deliberate difference from ``scipy.linalg.solve``'s ``posv``; it keeps Cholesky out of this family).

``QR`` (reference: tensor/nlinalg.py:403 QRFull, ``np.linalg.qr``: LAPACK geqrf + orgqr) is blocked
Householder on the kernels of csrc/qr.hip.  The workspace is a private copy of ``A`` held as an
``(N, M)`` contiguous buffer and viewed as ``M x N`` with strides ``(1, M)``: the ``raw`` result without
another copy, and contiguous columns for the one-workgroup panel kernel.  Per ``NB``-wide panel: the
panel kernel (``tau``, and a clean copy ``V`` of the reflectors), ``G = V^T V`` and ``ahip_larft`` for the
factor ``T`` of ``H_1 ... H_nb = I - V T V^T``, then the trailing block ``C -= V (T^T (V^T C))`` as three
products.  Q starts as the identity and takes the panels in reverse order, ``I - V T V^T`` each, on the
rows and columns from the panel's first on (the rest is still zero).  QR cannot fail: no info word,
non-finite input gives non-finite output.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_pool.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401

NB = 64                       # AHIP_LINALG_NB: rows of a diagonal block / columns of a panel
INFO_TAG = 1 << 62            # AHIP_LINALG_INFO_TAG
SINGULAR, NONFINITE = 2, 3    # AHIP_LINALG_SINGULAR / _NONFINITE
LINALG_OPS = ("SolveTriangular", "CholeskySolve", "Solve", "MatrixInverse", "Det")
QR_MODES = ("reduced", "complete", "r", "raw")


def is_linalg_code(code):
    """Whether an error word holds an info code of these kernels and not a bad index of the index
    kernels, which share the step's word (index + 1, saturated at 2^63 - 1 for a uint64 index beyond
    int64): the tag bit alone above a kind of two bits — every other bit from 34 up is zero."""
    return code > 0 and (code >> 34) == (INFO_TAG >> 34) and ((code >> 32) & 3) in (SINGULAR, NONFINITE)


def linalg_error(code, opname=None):
    """The exception an info word stands for, worded like the library the reference's ``perform``
    calls: ``scipy.linalg.solve_triangular`` / ``solve`` / ``numpy.linalg.inv``; non-finite operands
    as ``scipy``'s ``check_finite``."""
    kind, k = (code >> 32) & 0xFF, 0xFFFFFFFF - (code & 0xFFFFFFFF)
    if kind == NONFINITE:
        return ValueError("array must not contain infs or NaNs")
    if opname == "SolveTriangular":
        # (trtrs reports the 1-based index; SciPy prints info - 1)
        return np.linalg.LinAlgError(f"singular matrix: resolution failed at diagonal {k}")
    if opname == "MatrixInverse":
        return np.linalg.LinAlgError("Singular matrix")
    return np.linalg.LinAlgError("Matrix is singular.")


def _mat(a: DevArray, r0, r1, c0, c1) -> DevArray:
    """The sub-block [r0:r1, c0:c1] of a matrix view."""
    return a.view((r1 - r0, c1 - c0), a.strides, a.offset + r0 * a.strides[0] + c0 * a.strides[1])


def _t(a: DevArray) -> DevArray:
    """The transpose of a matrix view."""
    return a.view((a.shape[1], a.shape[0]), (a.strides[1], a.strides[0]))


def _column(a: DevArray) -> DevArray:
    """The only column of an n x 1 matrix view, as a vector."""
    return a.view(a.shape[:1], a.strides[:1])


class LinalgMixin:

    # ------------------------------------------------------------------ operands ------
    def _la_operands(self, node, args):
        ops, dt = self._float_operands(node, args)
        A = ops[0]
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError(f"{node.op}: expected a square matrix, got shape {tuple(A.shape)}")
        if len(ops) > 1:
            b = ops[1]
            if b.ndim not in (1, 2) or b.shape[0] != A.shape[0]:
                raise ValueError(f"{node.op}: shapes of a {tuple(A.shape)} and b {tuple(b.shape)} are "
                                 "incompatible")
        return ops, dt

    def _la_info(self):
        return _VP(self._bad_ptr())

    def _la_check_finite(self, a: DevArray, info):
        """``check_finite=True``: one pass over an operand."""
        if a.size == 0:
            return
        a2 = a if a.ndim == 2 else a.view((a.shape[0], 1), (a.strides[0], 0))
        self._launch("ahip_check_finite", (dtype_code(a.dtype), a2.shape[0], a2.shape[1], _VP(a2.ptr),
                                           a2.strides[0], a2.strides[1], info, self._stream()))

    def _la_rhs(self, b: DevArray):
        """(a fresh contiguous copy of b: the result, solved in place; its n x m matrix view)."""
        out = self.materialize(b)
        return out, (out if out.ndim == 2 else out.view((out.shape[0], 1), (1, 0)))

    # ------------------------------------------------------------------ products ------
    def _la_update(self, T: DevArray, Xk: DevArray, Xr: DevArray):
        """``Xr -= T @ Xk`` in place: ``ahip_gemv`` for one right-hand side, else ``ahip_gemm``."""
        (M, K), m = T.shape, Xk.shape[1]
        if M == 0 or K == 0 or m == 0:
            return
        # (the launchers, not _gemm / _gemv: in place, and never split-K, whose sums run in another order)
        if m == 1:
            y = _column(Xr)
            self._launch_gemv(-1.0, T, _column(Xk), 1.0, y, y)
        else:
            self._launch_gemm(-1.0, neutral_strides(T), neutral_strides(Xk), 1.0, Xr, Xr)

    # ------------------------------------------------------------------ block loops ---
    def _la_trsm(self, T: DevArray, X: DevArray, lower, unit, info):
        """Solve ``T X = X`` in place: ``T`` n x n triangular (any strides), ``X`` an n x m view."""
        n, m = T.shape[0], X.shape[1]
        if n == 0 or m == 0:
            return
        starts = list(range(0, n, NB))
        for k in (starts if lower else reversed(starts)):
            e = min(k + NB, n)
            Tk, Xk = _mat(T, k, e, k, e), _mat(X, k, e, 0, m)
            self._launch("ahip_trsm_diag", (dtype_code(T.dtype), int(lower), int(unit), e - k, m,
                                            _VP(Tk.ptr), T.strides[0], T.strides[1], _VP(Xk.ptr),
                                            X.strides[0], X.strides[1], k, info, self._stream()))
            if lower:
                self._la_update(_mat(T, e, n, k, e), Xk, _mat(X, e, n, 0, m))
            else:
                self._la_update(_mat(T, 0, k, k, e), Xk, _mat(X, 0, k, 0, m))

    def _la_getrf(self, LU: DevArray, info):
        """Right-looking blocked LU with partial pivoting of the workspace copy ``LU``, in place;
        returns the pivots (int32 device vector).  Four launches per panel."""
        n = LU.shape[0]
        piv = self.alloc((n,), "int32")
        code, (rs, cs) = dtype_code(LU.dtype), LU.strides
        for k in range(0, n, NB):
            e = min(k + NB, n)
            self._launch("ahip_getrf_panel", (code, n - k, e - k, _VP(_mat(LU, k, n, k, e).ptr), rs, cs,
                                              _VP(piv.ptr), k, info, self._stream()))
            if n > e - k:
                self._launch("ahip_laswp", (code, n, n - (e - k), _VP(LU.ptr), rs, cs, _VP(piv.ptr), k, e,
                                            k, e - k, self._stream()))
            if e < n:
                U12 = _mat(LU, k, e, e, n)
                self._launch("ahip_trsm_diag", (code, 1, 1, e - k, n - e, _VP(_mat(LU, k, e, k, e).ptr), rs,
                                                cs, _VP(U12.ptr), rs, cs, k, None, self._stream()))
                self._la_update(_mat(LU, e, n, k, e), U12, _mat(LU, e, n, e, n))
        return piv

    def _la_factor(self, A: DevArray, assume_a, lower, info):
        """(LU, pivots) of a private copy of ``A`` — completed from the triangle ``lower`` names
        unless ``assume_a`` is 'gen'."""
        n = A.shape[0]
        LU = self.alloc((n, n), A.dtype)
        self.copy_into(LU, A)
        if assume_a != "gen" and n > 1:
            self._launch("ahip_mirror_triangle", (dtype_code(A.dtype), int(lower), n, _VP(LU.ptr), n, 1,
                                                  self._stream()))
        return LU, self._la_getrf(LU, info)

    def _la_lu_solve(self, LU, piv, X):
        n, m = LU.shape[0], X.shape[1]
        if n == 0 or m == 0:
            return
        self._launch("ahip_laswp", (dtype_code(LU.dtype), n, m, _VP(X.ptr), X.strides[0], X.strides[1],
                                    _VP(piv.ptr), 0, n, m, 0, self._stream()))
        self._la_trsm(LU, X, True, True, None)
        self._la_trsm(LU, X, False, False, None)       # (a zero pivot was recorded by the factorisation)

    # ------------------------------------------------------------------ the Ops -------
    def _op_SolveTriangular(self, node, args):
        """reference: slinalg.py:301 SolveTriangular.perform (scipy.linalg.solve_triangular);
        ``trans`` = 1 is a stride swap plus flipping ``lower``."""
        (A, b), dt = self._la_operands(node, args)
        p = node.params
        info = self._la_info()
        if p["check_finite"]:
            self._la_check_finite(A, info)
            self._la_check_finite(b, info)
        lower = bool(p["lower"])
        if p["trans"]:
            A, lower = A.view(A.shape, (A.strides[1], A.strides[0])), not lower
        out, X = self._la_rhs(b)
        self._la_trsm(A, X, lower, p["unit_diagonal"], None if p["unit_diagonal"] else info)
        return [out]

    def _op_CholeskySolve(self, node, args):
        """reference: slinalg.py:158 CholeskySolve.perform (scipy.linalg.cho_solve, LAPACK potrs:
        two triangular solves, no singularity test)."""
        (Cf, b), dt = self._la_operands(node, args)
        p = node.params
        if p["check_finite"]:
            info = self._la_info()
            self._la_check_finite(Cf, info)
            self._la_check_finite(b, info)
        Ct = Cf.view(Cf.shape, (Cf.strides[1], Cf.strides[0]))
        out, X = self._la_rhs(b)
        if p["lower"]:          # A = L L^T
            self._la_trsm(Cf, X, True, False, None)
            self._la_trsm(Ct, X, False, False, None)
        else:                   # A = U^T U
            self._la_trsm(Ct, X, True, False, None)
            self._la_trsm(Cf, X, False, False, None)
        return [out]

    def _op_Solve(self, node, args):
        """reference: slinalg.py:388 Solve.perform (scipy.linalg.solve): LU of a copy, the
        interchanges on b, unit-lower and upper solves."""
        (A, b), dt = self._la_operands(node, args)
        p = node.params
        info = self._la_info()
        if p["check_finite"]:
            self._la_check_finite(A, info)
            self._la_check_finite(b, info)
        LU, piv = self._la_factor(A, p["assume_a"], p["lower"], info)
        out, X = self._la_rhs(b)
        self._la_lu_solve(LU, piv, X)
        return [out]

    def _op_MatrixInverse(self, node, args):
        """reference: nlinalg.py:124 MatrixInverse.perform (np.linalg.inv): ``Solve`` with B = I."""
        (A,), dt = self._la_operands(node, args)
        n = A.shape[0]
        LU, piv = self._la_factor(A, "gen", False, self._la_info())
        out = self.alloc((n, n), dt)
        self.fill_zero(out)
        if n:
            self.copy_into(out.view((n,), (n + 1,)), self._one(dt))
        self._la_lu_solve(LU, piv, out)
        return [out]

    def _op_Det(self, node, args):
        """reference: nlinalg.py:210 Det.perform (np.linalg.det): the sign of the interchanges times
        the diagonal of U; a singular matrix gives 0 (no info word), a 0 x 0 matrix 1."""
        (A,), dt = self._la_operands(node, args)
        n = A.shape[0]
        LU, piv = self._la_factor(A, "gen", False, None)
        out = self.alloc((), dt)
        self._launch("ahip_lu_det", (dtype_code(dt), n, _VP(LU.ptr), n, 1, _VP(piv.ptr), _VP(out.ptr),
                                     self._stream()))
        return [out]

    # ------------------------------------------------------------------ QR ------------
    def _qr_apply(self, V: DevArray, T: DevArray, Cm: DevArray, W: DevArray, W2: DevArray):
        """``Cm <- (I - V T V^T) Cm`` in place as three products (``W``, ``W2``: NB-row workspaces);
        pass the transposed view of ``T`` for the transposed block reflector."""
        nb, nc = V.shape[1], Cm.shape[1]
        if nb == 0 or nc == 0 or V.shape[0] == 0:
            return
        Wv, W2v = W.view((nb, nc), (nc, 1)), W2.view((nb, nc), (nc, 1))
        # (the launcher: in place, and never split-K, whose sums run in another order)
        self._launch_gemm(1.0, neutral_strides(_t(V)), neutral_strides(Cm), 0.0, Wv, Wv)
        self._launch_gemm(1.0, neutral_strides(T), neutral_strides(Wv), 0.0, W2v, W2v)
        self._launch_gemm(-1.0, neutral_strides(V), neutral_strides(W2v), 1.0, Cm, Cm)

    def _op_QR(self, node, args):
        """reference: nlinalg.py:441 QRFull.perform (np.linalg.qr(x, mode)).  Six launches per panel
        (panel, G, T, three products), three for a last panel that nothing follows."""
        (A,), dt = self._float_operands(node, args)
        mode = node.params["mode"]
        if mode not in QR_MODES:
            raise ValueError(f"{node.op}: mode {mode!r} (one of {', '.join(QR_MODES)})")
        if A.ndim != 2:
            raise ValueError(f"{node.op}: expected a matrix, got shape {tuple(A.shape)}")
        (M, N), code = A.shape, dtype_code(dt)
        K = min(M, N)
        H = self.alloc((N, M), dt)
        Aw = H.view((M, N), (1, M))
        self.copy_into(Aw, A)
        tau = self.alloc((K,), dt)
        want_q = mode in ("reduced", "complete")
        cols = M if mode == "complete" else K
        starts = list(range(0, K, NB))
        # the reflectors: all of them for Q, else the current panel's only
        Vall = self.alloc((K if want_q else min(NB, K), M), dt)
        Vall = Vall.view((M, Vall.shape[0]), (1, M))
        Ts = self.alloc((len(starts) if want_q else 1, NB, NB), dt)
        G = self.alloc((NB, NB), dt)
        wide = max(N, cols) if want_q else N
        W, W2 = self.alloc((NB, wide), dt), self.alloc((NB, wide), dt)
        blocks = []
        for p, k in enumerate(starts):
            e = min(k + NB, K)
            nb = e - k
            V = _mat(Vall, k, M, k, e) if want_q else _mat(Vall, k, M, 0, nb)
            T = Ts.view((nb, nb), (NB, 1), Ts.offset + (p * NB * NB if want_q else 0))
            tau_k = _VP(tau.view((nb,), (1,), tau.offset + k).ptr)
            self._launch("ahip_geqr2_panel", (code, M - k, nb, _VP(_mat(Aw, k, M, k, e).ptr), 1, M, tau_k,
                                              _VP(V.ptr), V.strides[0], V.strides[1], self._stream()))
            if e < N or want_q:
                Gv = G.view((nb, nb), (NB, 1))
                self._launch_gemm(1.0, neutral_strides(_t(V)), neutral_strides(V), 0.0, Gv, Gv)
                self._launch("ahip_larft", (code, nb, _VP(Gv.ptr), NB, 1, tau_k, _VP(T.ptr), NB, 1,
                                            self._stream()))
                self._qr_apply(V, _t(T), _mat(Aw, k, M, e, N), W, W2)
            blocks.append((k, V, T))
        if mode == "raw":
            return [H, tau]
        R = self.alloc((M if mode == "complete" else K, N), dt)
        if R.size:
            self._launch("ahip_qr_extract_r", (code, R.shape[0], N, _VP(Aw.ptr), 1, M, _VP(R.ptr), N, 1,
                                               self._stream()))
        if not want_q:
            return [R]
        Q = self.alloc((M, cols), dt)
        self.fill_zero(Q)
        if cols:
            self.copy_into(Q.view((cols,), (cols + 1,)), self._one(dt))
        for k, V, T in reversed(blocks):
            self._qr_apply(V, T, _mat(Q, k, M, k, cols), W, W2)
        return [Q, R]
