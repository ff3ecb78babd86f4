"""The matrix exponential of a PlanExecutor: ``Expm`` and ``ExpmGrad`` (reference: tensor/slinalg.py:595
/ :631, ``scipy.linalg.expm``) on the kernels of csrc/expm.hip plus ``ahip_gemm`` and the blocked LU of
exec_linalg.py.

Scaling and squaring after Higham (2005): ``||A||_1`` picks the Pade degree ``m`` from 3, 5, 7, 9, 13 and
the scaling ``s``; with ``B = 2^-s A`` the approximant is ``(V - U)^-1 (V + U)``, ``U`` odd and ``V`` even in
``B``, and the result is its ``2^s``-th power by ``s`` squarings.

Up to ``TILE_ROWS`` rows (64 in float32, 48 in float64) all of that is ONE launch (``ahip_expm_tile``: seven
matrices resident in LDS).  Nothing is read on the host: such a call records and replays.

Above, the products are ``ahip_gemm`` and the solve is ``_la_getrf`` + ``_la_lu_solve``.  ``ahip_expm_norm1``
leaves the norm, ``m`` and ``s`` in a status record and the host reads it ONCE — how many products to issue
depends on it: a read that cannot be recorded, so such a plan runs eagerly (``HostReadInReplay``, like
``Eigvalsh`` above 64 rows).  ``ahip_expm_combine`` forms the linear combinations of the powers; the scaling
is the coefficient of the first of them (``B = 2^-s A``, exact).  Folding ``2^-2ks`` into the coefficient of
``A^2k`` instead would leave float32 with subnormal coefficients from ``s = 13`` on.

``ExpmGrad(A, G)`` is the Frechet derivative of ``exp`` at ``A^T`` in direction ``G``: the top-right block of
``expm([[A^T, G], [0, A^T]])``, through the same dispatch on the ``2n x 2n`` matrix.  Unlike the reference's
``eig`` / ``inv(V)`` route it has no complex arithmetic and holds for a defective ``A``.

Nothing fails: the LU of ``V - U`` meets no zero pivot under the thresholds, so there is no info word, and a
non-finite operand gives a non-finite result like SciPy.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_svd.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401
from .exec_linalg import _mat, _t

TILE_ROWS = {"float32": 64, "float64": 48}      # AHIP_EXPM_TILE_F32 / _F64
STATUS_WORDS = 3                                # AHIP_EXPM_STATUS_WORDS: the bits of ||A||_1, m, s
EXPM_OPS = ("Expm", "ExpmGrad")
# b_0 .. b_m of the degree-m Pade numerator (Higham 2005, (2.3)), as the integers csrc/expm.hip holds
PADE = {3: (120, 60, 12, 1),
        5: (30240, 15120, 3360, 420, 30, 1),
        7: (17297280, 8648640, 1995840, 277200, 25200, 1512, 56, 1),
        9: (17643225600, 8821612800, 2075673600, 302702400, 30270240, 2162160, 110880, 3960, 90, 1),
        13: (64764752532480000, 32382376266240000, 7771770303897600, 1187353796428800, 129060195264000,
             10559470521600, 670442572800, 33522128640, 1323241920, 40840800, 960960, 16380, 182, 1)}


class ExpmMixin:

    def _expm_combine(self, out: DevArray, terms, d=0.0):
        """``out = sum c X + d I`` for up to four ``(c, X)`` of contiguous n x n matrices; ``out`` may be one."""
        flat = [v for c, X in terms for v in (_VP(X.ptr), float(c))]
        flat += [None, 0.0] * (4 - len(terms))
        self._launch("ahip_expm_combine", (dtype_code(out.dtype), out.shape[0], len(terms), *flat, float(d),
                                           _VP(out.ptr), self._stream()))

    def _expm_product(self, X: DevArray, Y: DevArray):
        out = self.alloc(X.shape, X.dtype)
        # (the launcher: never split-K, whose sums run in another order)
        self._launch_gemm(1.0, X, Y, 0.0, out, out)
        return out

    def _expm_blocked(self, A: DevArray):
        """``expm`` of a square view of more than ``TILE_ROWS`` rows: one host read, then products and one LU."""
        n, dt = A.shape[0], A.dtype
        status, colsum = self.alloc((STATUS_WORDS,), "int64"), self.alloc((n,), "float64")
        self.expm_status = status           # (the last call's record: norm, m, s for tools/expm_probe.py)
        self._launch("ahip_expm_norm1", (dtype_code(dt), n, _VP(A.ptr), A.strides[0], A.strides[1],
                                         _VP(colsum.ptr), _VP(status.ptr), self._stream()))
        # (a dry run has no values: it shows the launches of the highest degree and one squaring)
        m, s = (13, 1) if self.dry_run else (int(v) for v in self.host_array(status)[1:])
        B = self.materialize(A)
        if s:
            self._expm_combine(B, [(2.0 ** -s, B)])
        c = [b / PADE[m][0] for b in PADE[m]]
        A2 = self._expm_product(B, B)
        A4 = self._expm_product(A2, A2) if m >= 5 else None
        A6 = self._expm_product(A4, A2) if m >= 7 else None
        UV = []
        if m <= 9:
            powers = [A2, A4, A6, self._expm_product(A4, A4) if m == 9 else None][:m // 2]
            for odd in (1, 0):
                W = self.alloc((n, n), dt)
                self._expm_combine(W, [(c[2 * k + 2 + odd], P) for k, P in enumerate(powers)], c[odd])
                UV.append(self._expm_product(B, W) if odd else W)
        else:
            T = self.alloc((n, n), dt)
            for odd in (1, 0):
                self._expm_combine(T, [(c[12 + odd], A6), (c[10 + odd], A4), (c[8 + odd], A2)])
                W = self._expm_product(A6, T)
                self._expm_combine(W, [(1.0, W), (c[6 + odd], A6), (c[4 + odd], A4), (c[2 + odd], A2)], c[odd])
                UV.append(self._expm_product(B, W) if odd else W)
        U, V = UV
        L, X = self.alloc((n, n), dt), self.alloc((n, n), dt)
        self._expm_combine(L, [(1.0, V), (-1.0, U)])
        self._expm_combine(X, [(1.0, V), (1.0, U)])
        self._la_lu_solve(L, self._la_getrf(L, None), X)
        for _ in range(s):
            X = self._expm_product(X, X)
        return X

    def _expm(self, A: DevArray):
        """``expm`` of a non-empty square float32 / float64 view of any strides, as a fresh contiguous array."""
        n, dt = A.shape[0], A.dtype
        if n > TILE_ROWS[dt]:
            return self._expm_blocked(A)
        out = self.alloc((n, n), dt)
        self._launch("ahip_expm_tile", (dtype_code(dt), 1, n, _VP(A.ptr), 0, A.strides[0], A.strides[1],
                                        _VP(out.ptr), 0, n, 1, None, self._stream()))
        return out

    def _expm_square(self, node, A):
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            # (scipy.linalg.expm's wording)
            raise np.linalg.LinAlgError("Last 2 dimensions of the array must be square")

    # ------------------------------------------------------------------ the Ops -------
    def _op_Expm(self, node, args):
        """reference: slinalg.py:617 Expm.perform (scipy.linalg.expm(A))."""
        if node.params.get("batched"):
            return [self._expm_stack(node, args)]
        (A,), dt = self._float_operands(node, args)
        self._expm_square(node, A)
        if A.shape[0] == 0:
            return [self.alloc((0, 0), dt)]
        return [self._expm(A)]

    def _expm_stack(self, node, args):
        """``expm`` of every matrix of a ``[T, n, n]`` stack (a ``batched`` node of scan_rewrite.batch_map_step):
        ONE ``ahip_expm_tile`` launch with batch = T inside ``TILE_ROWS``, the single-matrix route per matrix
        above."""
        (A,), dt = self._float_operands(node, args)
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise np.linalg.LinAlgError("Last 2 dimensions of the array must be square")
        T, n = A.shape[0], A.shape[1]
        out = self.alloc((T, n, n), dt)
        if out.size == 0:
            return out
        if n > TILE_ROWS[dt]:
            return self._la_each(A, out, self._expm)
        self._launch("ahip_expm_tile", (dtype_code(dt), T, n, _VP(A.ptr), A.strides[0], A.strides[1], A.strides[2],
                                        _VP(out.ptr), n * n, n, 1, None, self._stream()))
        return out

    def _op_ExpmGrad(self, node, args):
        """reference: slinalg.py:654 ExpmGrad.perform; here the top-right block of
        ``expm([[A^T, G], [0, A^T]])``."""
        (A, G), dt = self._float_operands(node, args)
        self._expm_square(node, A)
        n = A.shape[0]
        if tuple(G.shape) != (n, n):
            raise ValueError(f"{node.op}: shapes of A {tuple(A.shape)} and the output gradient {tuple(G.shape)} "
                             "are incompatible")
        if n == 0:
            return [self.alloc((0, 0), dt)]
        if n == 1:
            # the derivative of the scalar exponential: exp(a) g, as a 1 x 1 product
            out = self.alloc((1, 1), dt)
            self._launch_gemm(1.0, neutral_strides(self._expm(A)), neutral_strides(G), 0.0, out, out)
            return [out]
        M = self.alloc((2 * n, 2 * n), dt)
        self.fill_zero(M)
        self.copy_into(_mat(M, 0, n, 0, n), _t(A))
        self.copy_into(_mat(M, n, 2 * n, n, 2 * n), _t(A))
        self.copy_into(_mat(M, 0, n, n, 2 * n), G)
        return [self.materialize(_mat(self._expm(M), 0, n, n, 2 * n))]
