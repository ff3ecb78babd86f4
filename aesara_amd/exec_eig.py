"""The symmetric eigenvalues of a PlanExecutor: ``Eigvalsh`` and ``EigvalshGrad`` (reference:
tensor/slinalg.py :446 / :493, ``scipy.linalg.eigvalsh`` / ``eigh``) on the kernels of csrc/eig.hip
plus ``ahip_trsm_diag``, ``ahip_gemm`` and the sort kernels.

The solver is two-sided Jacobi in round-robin order.  Up to ``TILE`` = 64 rows the whole solve is ONE
launch (``ahip_syev_tile``: matrix and rotations resident in LDS) and the call records and replays like
any other.  Above it the matrix is zero-padded to a multiple of 64 (an exact zero coupling is an exact
identity rotation: the padding never mixes in) and 32-wide blocks play the tournament: per step the
pairs are gathered into 64 x 64 tiles, the tile solver returns their rotation matrices and
``ahip_syev_apply`` multiplies them onto the columns, then onto the rows through the transposed view,
out of place between two workspaces — and onto ``V`` when eigenvectors are wanted.  A tile of the
tournament converges to ``eps / sqrt(nb - 1)`` of its own norm: every diagonal block is in ``nb - 1``
tiles of a sweep, so tiles that all pass that test give a matrix that passes ``off_F <= eps ||A||_F``.
Before every sweep ``ahip_syev_off`` measures that and the host reads ONE word: a read that cannot be
recorded, so such a plan runs eagerly (``HostReadInReplay``, like a do-while Scan).

The generalised problem factors ``B = L L^T`` with a blocked Cholesky (``ahip_potrf_diag`` on the
diagonal block, ``ahip_trsm_diag`` below it, ``ahip_gemm`` behind it: the loop of ``_la_getrf``) and
solves the standard problem of ``C = L^-1 A L^-T``.  ``lower`` only names the triangle that is read:
for the upper one the same loop runs on the transposed view.  The factorisation is internal: the
``Cholesky`` Op stays refused.

Errors go through the node's info word (kind ``EIG``: ``B`` not positive definite, no convergence of
the one-launch solver; non-finite operands as in exec_linalg.py); above 64 rows the host that reads
the done word raises the non-convergence itself.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_linalg.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401
from .exec_linalg import NB, _mat, _t

TILE = 64                     # AHIP_SYEV_TILE: rows of the one-launch solver
BLOCK = TILE // 2             # rows of a block of the tournament
NSWEEP = 30                   # AHIP_SYEV_NSWEEP
STATUS_WORDS = 4 + 2 * 256    # AHIP_SYEV_STATUS_WORDS
EIG_OPS = ("Eigvalsh", "EigvalshGrad")


class EigMixin:

    # ------------------------------------------------------------------ operands ------
    def _eig_operands(self, node, args):
        ops, dt = self._float_operands(node, args)
        A = ops[0]
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError(f"{node.op}: expected a square matrix, got shape {tuple(A.shape)}")
        if len(ops) > 1 and tuple(ops[1].shape) != tuple(A.shape):
            raise ValueError(f"{node.op}: shapes of a {tuple(A.shape)} and b {tuple(ops[1].shape)} are "
                             "incompatible")
        if len(ops) > 2 and tuple(ops[2].shape) != (A.shape[0],):
            raise ValueError(f"{node.op}: shapes of a {tuple(A.shape)} and gw {tuple(ops[2].shape)} are "
                             "incompatible")
        return ops, dt

    def _eig_identity(self, n, dt):
        out = self.alloc((n, n), dt)
        self.fill_zero(out)
        if n:
            self.copy_into(out.view((n,), (n + 1,)), self._one(dt))
        return out

    # ------------------------------------------------------------------ Cholesky of b -
    def _eig_potrf(self, L: DevArray, info):
        """``B = L L^T`` in place in the lower triangle of the view ``L``; three launches per block."""
        n, code, (rs, cs) = L.shape[0], dtype_code(L.dtype), L.strides
        for k in range(0, n, NB):
            e = min(k + NB, n)
            Lkk = _mat(L, k, e, k, e)
            self._launch("ahip_potrf_diag", (code, 1, e - k, _VP(Lkk.ptr), rs, cs, k, info, self._stream()))
            if e < n:
                # the panel below: P <- P L_kk^-T, solved as L_kk X = P^T on the transposed view
                P = _mat(L, e, n, k, e)
                self._launch("ahip_trsm_diag", (code, 1, 0, e - k, n - e, _VP(Lkk.ptr), rs, cs, _VP(P.ptr),
                                                cs, rs, k, None, self._stream()))
                B22 = _mat(L, e, n, e, n)
                self._launch_gemm(-1.0, neutral_strides(P), neutral_strides(_t(P)), 1.0, B22, B22)

    def _eig_reduce(self, A: DevArray, b, lower, info):
        """(the symmetric matrix whose eigenvalues are wanted, the triangle to read, ``L`` or None):
        ``a`` itself for the standard problem, else ``C = L^-1 A L^-T`` with ``B = L L^T``."""
        if b is None:
            return A, lower, None
        n, dt = A.shape[0], A.dtype
        L = self.materialize(b)
        if not lower:
            L = _t(L)             # the upper triangle of b is the lower one of this view
        self._eig_potrf(L, info)
        Cm = self.materialize(A)
        if n > 1:
            self._launch("ahip_mirror_triangle", (dtype_code(dt), int(lower), n, _VP(Cm.ptr), n, 1,
                                                  self._stream()))
        self._la_trsm(L, Cm, True, False, None)            # L^-1 A
        self._la_trsm(L, _t(Cm), True, False, None)        # (L^-1 A) L^-T, through the transposed view
        return Cm, True, L

    # ------------------------------------------------------------------ Jacobi --------
    def _jacobi_apply(self, code, nb, step, rows, src: DevArray, dst: DevArray, ld, Jt: DevArray, transposed=False):
        """``dst[:, p|q] = src[:, p|q] J`` for the pairs of a tournament step (``ahip_syev_apply``), on
        ``rows`` rows of two row-major workspaces of pitch ``ld``; ``transposed``: on their transposed
        views, which is ``dst[p|q, :] = J^T src[p|q, :]``."""
        rs, cs = (1, ld) if transposed else (ld, 1)
        self._launch("ahip_syev_apply", (code, nb, step, rows, _VP(src.ptr), rs, cs, _VP(Jt.ptr),
                                         _VP(dst.ptr), rs, cs, self._stream()))

    def _jacobi_done(self, status: DevArray):
        """The done word of a status record, read on the host: ONE word a sweep.  While a launch list
        is recorded the read raises HostReadInReplay: such a plan runs eagerly."""
        return int(self.host_array(status.view((1,), (1,)))[0]) != 0

    def _eig_jacobi(self, Cm: DevArray, lower, want_v, info):
        """(``w`` unsorted, ``V`` or None) of the symmetric ``Cm``, of which only the triangle ``lower``
        names is read: the diagonal of ``V^T Cm V`` and the accumulated rotations."""
        n, dt = Cm.shape[0], Cm.dtype
        code = dtype_code(dt)
        status = self.alloc((STATUS_WORDS,), "int64")
        self.fill_zero(status)
        self.eig_status = status            # (the last solve's record: sweep counts for tools/eig_probe.py)
        w = self.alloc((n,), dt)
        if n <= TILE:
            V = self.alloc((n, n), dt) if want_v else None
            self._launch("ahip_syev_tile", (code, int(lower), 1, n, _VP(Cm.ptr), 0, Cm.strides[0], Cm.strides[1],
                                            None, 0, 0, 0, _VP(V.ptr) if want_v else None, 0, n, 1,
                                            _VP(w.ptr), 0, 1.0, _VP(status.ptr), info, self._stream()))
            return w, V
        n_pad = -(-n // TILE) * TILE
        nb = n_pad // BLOCK
        pairs = nb // 2
        W0, W1 = self.alloc((n_pad, n_pad), dt), self.alloc((n_pad, n_pad), dt)
        self.fill_zero(W0)
        self.copy_into(_mat(W0, 0, n, 0, n), Cm)
        self._launch("ahip_mirror_triangle", (code, int(lower), n, _VP(W0.ptr), n_pad, 1, self._stream()))
        T, Jt = self.alloc((pairs, TILE, TILE), dt), self.alloc((pairs, TILE, TILE), dt)
        V0 = V1 = None
        if want_v:
            V0, V1 = self._eig_identity(n_pad, dt), self.alloc((n_pad, n_pad), dt)
        tt = TILE * TILE
        sweeps = 0
        while True:
            self._launch("ahip_syev_off", (code, n_pad, _VP(W0.ptr), n_pad, 1, _VP(status.ptr), info,
                                           self._stream()))
            # (a dry run has no values: it shows the launches of one sweep)
            done = sweeps >= 1 if self.dry_run else self._jacobi_done(status)
            if done:
                break
            if sweeps == NSWEEP:
                raise np.linalg.LinAlgError("Eigenvalues did not converge")
            for step in range(nb - 1):
                self._launch("ahip_syev_gather", (code, nb, step, _VP(W0.ptr), n_pad, 1, _VP(T.ptr),
                                                  self._stream()))
                self._launch("ahip_syev_tile", (code, 1, pairs, TILE, _VP(T.ptr), tt, TILE, 1, None, 0, 0, 0,
                                                _VP(Jt.ptr), tt, TILE, 1, None, 0, 1.0 / (nb - 1),
                                                _VP(status.ptr), None, self._stream()))
                # A <- A J into the other workspace, then A <- J^T A back
                self._jacobi_apply(code, nb, step, n_pad, W0, W1, n_pad, Jt)
                self._jacobi_apply(code, nb, step, n_pad, W1, W0, n_pad, Jt, transposed=True)
                if want_v:
                    self._jacobi_apply(code, nb, step, n_pad, V0, V1, n_pad, Jt)
                    V0, V1 = V1, V0
            sweeps += 1
        self._launch("ahip_syev_diag", (code, n, _VP(W0.ptr), n_pad, 1, _VP(w.ptr), self._stream()))
        return w, (_mat(V0, 0, n, 0, n) if want_v else None)

    def _eig_checked(self, ops, info):
        for a in ops:           # scipy.linalg.eigvalsh / eigh: check_finite=True
            self._la_check_finite(a, info)

    # ------------------------------------------------------------------ the Ops -------
    def _op_Eigvalsh(self, node, args):
        """reference: slinalg.py:476 Eigvalsh.perform (scipy.linalg.eigvalsh(a, b, lower)): ascending
        eigenvalues of ``a x = w b x``; ``b`` absent for the standard problem."""
        if node.params.get("batched"):
            return [self._eig_stack(node, args)]
        ops, dt = self._eig_operands(node, args)
        return [self._eigvalsh(ops, bool(node.params["lower"]))]

    def _eigvalsh(self, ops, lower):
        A, b = ops[0], (ops[1] if len(ops) > 1 else None)
        if A.shape[0] == 0:
            return self.alloc((0,), A.dtype)
        info = self._la_info()
        self._eig_checked(ops, info)
        Cm, lo, _ = self._eig_reduce(A, b, lower, info)
        w, _ = self._eig_jacobi(Cm, lo, False, info)
        return self._sort(None, [w, np.int64(0)], False)[0]

    def _eig_stack(self, node, args):
        """The standard problem on every matrix of a ``[T, n, n]`` stack (a ``batched`` node of
        scan_rewrite.batch_map_step): up to ``TILE`` rows ONE ``ahip_syev_tile`` launch with batch = T and one
        sort of the rows of the ``[T, n]`` result, the single-matrix route per matrix above."""
        A, dt = self._la_stack(node, args)
        T, n = A.shape[0], A.shape[1]
        lower = bool(node.params["lower"])
        if T == 0 or n == 0:
            return self.alloc((T, n), dt)
        if n > TILE:
            return self._la_each(A, self.alloc((T, n), dt), lambda M: self._eigvalsh([M], lower))
        info = self._la_info()
        # (check_finite over the stack as ONE matrix of T n rows: a stack whose leading dimensions do not
        # fold is copied first)
        Af = A if A.strides[0] == n * A.strides[1] else self.materialize(A)
        self._la_check_finite(Af.view((T * n, n), Af.strides[1:]), info)
        status = self.alloc((STATUS_WORDS,), "int64")
        self.fill_zero(status)
        self.eig_status = status
        w = self.alloc((T, n), dt)
        self._launch("ahip_syev_tile", (dtype_code(dt), int(lower), T, n, _VP(A.ptr), A.strides[0], A.strides[1],
                                        A.strides[2], None, 0, 0, 0, None, 0, 0, 0, _VP(w.ptr), n, 1.0,
                                        _VP(status.ptr), info, self._stream()))
        return self._sort(None, [w, np.int64(1)], False)[0]

    def _op_EigvalshGrad(self, node, args):
        """reference: slinalg.py:533 EigvalshGrad.perform: ``w, v = scipy.linalg.eigh(a, b, lower)``,
        ``gA = v diag(gw) v^T``, ``gB = -v diag(gw w) v^T``, each folded into the named triangle."""
        (A, b, gw), dt = self._eig_operands(node, args)
        n, code, lower = A.shape[0], dtype_code(dt), bool(node.params["lower"])
        outs = [self.alloc((n, n), dt), self.alloc((n, n), dt)]
        if n == 0:
            return outs
        info = self._la_info()
        self._eig_checked((A, b, gw), info)
        Cm, lo, L = self._eig_reduce(A, b, lower, info)
        wu, Y = self._eig_jacobi(Cm, lo, True, info)
        V = self.materialize(Y)
        self._la_trsm(_t(L), V, False, False, None)        # V <- L^-T Y: B-orthonormal columns
        w = self._sort(None, [wu, np.int64(0)], False)[0]
        order = self._sort(None, [wu, np.int64(0)], True)[0]
        gwc = self.contiguous(gw)

        def scaled(g, h):
            """the columns of V in ascending eigenvalue order, times g and h"""
            out = self.alloc((n, n), dt)
            self._launch("ahip_scale_cols", (code, n, n, _VP(V.ptr), n, 1, _VP(order.ptr),
                                             None if g is None else _VP(g.ptr), None if h is None else _VP(h.ptr),
                                             _VP(out.ptr), n, 1, self._stream()))
            return out
        Vs = neutral_strides(_t(scaled(None, None)))
        G = self.alloc((n, n), dt)
        for out, alpha, S in ((outs[0], 1.0, scaled(gwc, None)), (outs[1], -1.0, scaled(gwc, w))):
            self._launch_gemm(alpha, neutral_strides(S), Vs, 0.0, G, G)
            self._launch("ahip_sym_fold", (code, int(lower), n, _VP(G.ptr), n, 1, _VP(out.ptr), n, 1,
                                           self._stream()))
        return outs
