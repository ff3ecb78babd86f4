"""The pseudo-inverse of a PlanExecutor: ``MatrixPinv`` (reference: tensor/nlinalg.py:16,
``np.linalg.pinv(x, hermitian)``) on the kernels of csrc/svd.hip plus ``ahip_syev_apply``,
``ahip_scale_cols``, ``ahip_gemm`` and the blocked QR of exec_linalg.py.

The decomposition is a one-sided (Hestenes) Jacobi SVD of the orientation with ``rows >= cols`` (``m <
n`` runs on the transposed view and transposes the result: ``pinv(A^T) = pinv(A)^T``): rotations of
column pairs in round-robin order give ``W = X V`` with orthogonal columns of norms ``sigma``, and
``pinv(X) = (V d)(W d)^T`` with ``d = 1 / sigma`` where ``sigma > 1e-15 max(sigma)``, else 0.

Up to ``TILE`` = 64 columns the whole solve is ONE launch (``ahip_gesvj_tile``: matrix and rotations
resident in LDS).  An operand with more than 64 rows first goes through the reduced QR — ``pinv(Q R) =
pinv(R) Q^T`` for any ``R``, since ``Q`` has orthonormal columns — and the tile solver works on the
``k x k`` factor.  Nothing is read on the host: such a call records and replays.

Above 64 columns the columns are zero-padded to a multiple of 64 (a zero column never rotates) and
32-wide column blocks play the tournament of exec_eig.py: per step ``ahip_gesvj_gram`` (the 64 x 64 Gram
matrix of every pair, slab partials), ``ahip_gesvj_gram_tile`` (its rotation matrix ``J`` under the same
scaled threshold) and ``ahip_syev_apply`` on ``A`` and on ``V``, out of place between two workspaces.
After every sweep ``ahip_gesvj_done`` sums the tiles' rotation counts and the host reads ONE word: a
read that cannot be recorded, so such a plan runs eagerly (``HostReadInReplay``, like ``Eigvalsh`` above
64 rows).  The sweep that rotates nothing is the last.

``hermitian=True`` is ``np.linalg.pinv``'s other branch: ``eigh`` of the lower triangle
(``_eig_jacobi``), the same cutoff on ``|w|``, and ``(V d) V^T`` with ``d = 1 / w``.

Errors go through the node's info word: NumPy raises ``LinAlgError("SVD did not converge")`` for a NaN;
the device raises the same for every non-finite operand and for sweeps that run out (above 64 columns
the host that reads the done word raises that itself).

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_eig.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401
from .exec_eig import BLOCK, NSWEEP, TILE
from .exec_linalg import _mat, _t

SLAB = 256                    # AHIP_GESVJ_SLAB: rows of A behind one partial Gram matrix
STATUS_HEAD = 4               # AHIP_GESVJ_STATUS_HEAD
SVD_OPS = ("MatrixPinv",)


class SvdMixin:

    # ------------------------------------------------------------------ Jacobi --------
    def _svd_status(self, slots):
        status = self.alloc((STATUS_HEAD + slots,), "int64")
        self.fill_zero(status)
        self.svd_status = status            # (the last solve's record: sweep counts for tools/pinv_probe.py)
        return status

    def _svd_tile(self, X: DevArray, info):
        """(``W = X V``, ``V``) of a view of at most 64 rows and no more columns than rows: one launch."""
        (rows, cols), dt = X.shape, X.dtype
        W, V = self.alloc((rows, cols), dt), self.alloc((cols, cols), dt)
        status = self._svd_status(0)
        self._launch("ahip_gesvj_tile", (dtype_code(dt), 1, rows, cols, _VP(X.ptr), 0, X.strides[0],
                                         X.strides[1], _VP(W.ptr), 0, cols, 1, _VP(V.ptr), 0, cols, 1,
                                         None, 0, _VP(status.ptr), info, self._stream()))
        return W, V

    def _svd_tournament(self, X: DevArray, info):
        """(``W = X V``, ``V``) of a view of more than 64 columns and any row count: the sweep loop,
        one host read a sweep."""
        (rows, cols), dt = X.shape, X.dtype
        code = dtype_code(dt)
        k_pad = -(-cols // TILE) * TILE
        nb = k_pad // BLOCK
        pairs, slabs = nb // 2, -(-rows // SLAB)
        slots = (nb - 1) * pairs
        status = self._svd_status(slots)
        A0, A1 = self.alloc((rows, k_pad), dt), self.alloc((rows, k_pad), dt)
        self.fill_zero(A0)
        self.copy_into(_mat(A0, 0, rows, 0, cols), X)
        V0, V1 = self._eig_identity(k_pad, dt), self.alloc((k_pad, k_pad), dt)
        P, Jt = self.alloc((pairs, slabs, TILE, TILE), dt), self.alloc((pairs, TILE, TILE), dt)
        sweeps = 0
        while True:
            for step in range(nb - 1):
                self._launch("ahip_gesvj_gram", (code, nb, step, rows, _VP(A0.ptr), k_pad, 1, _VP(P.ptr),
                                                 self._stream()))
                self._launch("ahip_gesvj_gram_tile", (code, pairs, slabs, rows, _VP(P.ptr), _VP(Jt.ptr),
                                                      _VP(status.ptr), step * pairs, self._stream()))
                for S0, S1, n in ((A0, A1, rows), (V0, V1, k_pad)):
                    self._jacobi_apply(code, nb, step, n, S0, S1, k_pad, Jt)
                A0, A1, V0, V1 = A1, A0, V1, V0
            sweeps += 1
            self._launch("ahip_gesvj_done", (slots, _VP(status.ptr), info, self._stream()))
            if self.dry_run:
                break                       # (a dry run has no values: it shows the launches of one sweep)
            if self._jacobi_done(status):
                break
            if sweeps == NSWEEP:
                raise np.linalg.LinAlgError("SVD did not converge")
        return _mat(A0, 0, rows, 0, cols), _mat(V0, 0, cols, 0, cols)

    def _svd_weights(self, W, w, cols, dt):
        """``d`` of ``ahip_pinv_weights``: from the column norms of ``W``, or from the eigenvalues ``w``."""
        sigma, d = self.alloc((cols,), "float64"), self.alloc((cols,), dt)
        self.svd_sigma = sigma
        source = (0, cols, None, 0, 0, _VP(w.ptr)) if W is None else (W.shape[0], cols, _VP(W.ptr), *W.strides, None)
        self._launch("ahip_pinv_weights", (dtype_code(dt), *source, _VP(sigma.ptr), _VP(d.ptr), self._stream()))
        return d

    def _svd_scaled(self, M: DevArray, d: DevArray):
        """``M diag(d)`` as a fresh contiguous matrix."""
        rows, cols = M.shape
        out = self.alloc((rows, cols), M.dtype)
        self._launch("ahip_scale_cols", (dtype_code(M.dtype), rows, cols, _VP(M.ptr), M.strides[0], M.strides[1],
                                         None, _VP(d.ptr), None, _VP(out.ptr), cols, 1, self._stream()))
        return out

    # ------------------------------------------------------------------ the Op --------
    def _op_MatrixPinv(self, node, args):
        """reference: nlinalg.py:27 MatrixPinv.perform (np.linalg.pinv(x, hermitian).astype(x.dtype))."""
        (A,), dt = self._float_operands(node, args)
        if A.ndim != 2:
            raise ValueError(f"{node.op}: expected a matrix, got shape {tuple(A.shape)}")
        m, n = A.shape
        out = self.alloc((n, m), dt)
        if m == 0 or n == 0:
            return [out]
        info = self._la_info()
        if node.params["hermitian"]:
            if m != n:
                raise ValueError(f"{node.op}: hermitian=True expects a square matrix, got shape {tuple(A.shape)}")
            # np.linalg.eigh reads the lower triangle only: so does the check
            Cm = self.materialize(A)
            if n > 1:
                self._launch("ahip_mirror_triangle", (dtype_code(dt), 1, n, _VP(Cm.ptr), n, 1, self._stream()))
            self._la_check_finite(Cm, info)
            w, V = self._eig_jacobi(Cm, True, True, info)
            Vd = self._svd_scaled(V, self._svd_weights(None, w, n, dt))
            self._launch_gemm(1.0, neutral_strides(Vd), neutral_strides(_t(V)), 0.0, out, out)
            return [out]
        self._la_check_finite(A, info)
        X = A if m >= n else _t(A)
        rows, k = X.shape
        if k > TILE:
            W, V = self._svd_tournament(X, info)
            d = self._svd_weights(W, None, k, dt)
        else:
            Q = None
            if rows > TILE:
                Q, X = self._la_qr(X, "reduced")
            Wk, V = self._svd_tile(X, info)
            d = self._svd_weights(Wk, None, k, dt)
            W = Wk
            if Q is not None:               # W = Q (R V): the columns keep their norms
                W = self.alloc((rows, k), dt)
                self._launch_gemm(1.0, neutral_strides(Q), neutral_strides(Wk), 0.0, W, W)
        Vd, Wd = self._svd_scaled(V, d), self._svd_scaled(W, d)
        if m >= n:                          # (V d)(W d)^T, and its transpose for the transposed view
            self._launch_gemm(1.0, neutral_strides(Vd), neutral_strides(_t(Wd)), 0.0, out, out)
        else:
            self._launch_gemm(1.0, neutral_strides(Wd), neutral_strides(_t(Vd)), 0.0, out, out)
        return [out]
