"""The random-stream Ops of a PlanExecutor: ``MrgUniform``, ``MultinomialFromUniform`` and
``ChoiceFromUniform`` (reference: sandbox/rng_mrg.py mrg_uniform :373, sandbox/multinomial.py
MultinomialFromUniform :14 / ChoiceFromUniform :223) on the three kernels of csrc/rng.hip.

``size`` and ``n`` are operands: host integers, constant or not, read at run time.  The launch shape
of ``MrgUniform`` is a function of the number of streams, the number of samples and the switch
``AESARA_HIP_MRG_PARTS`` only, so a recorded launch list replays for the same shapes; the state goes
in and comes out as a device tensor and never visits the host.

MRG31k3p has an exact jump-ahead (:func:`mrg_jump_table`): a stream's run is cut into ``parts``
pieces that start from the state jumped ahead, which fills the device when there are fewer streams
than lanes and changes no bit of the result.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_pool.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401

M1 = 2147483647          # 2^31 - 1
M2 = 2147462579          # 2^31 - 21069
# one step as a matrix: (x11, x12, x13) <- A1 (x11, x12, x13) mod M1, likewise A2 / M2
A1 = ((0, 1 << 22, (1 << 7) + 1), (1, 0, 0), (0, 1, 0))
A2 = ((1 << 15, 0, (1 << 15) + 1), (1, 0, 0), (0, 1, 0))
_EYE = ((1, 0, 0), (0, 1, 0), (0, 0, 1))

# lanes that fill the device: 256 CUs x 16 wavefronts x 64 lanes (the rule of mrg_parts; measured,
# 8 wavefronts per CU were 23 % slower at 2^24 float32 samples)
FILL_LANES = 256 * 16 * 64


def mat_mul_mod(A, B, m):
    """3x3 product mod ``m`` in Python integers."""
    return tuple(tuple(sum(A[i][k] * B[k][j] for k in range(3)) % m for j in range(3)) for i in range(3))


def mat_pow_mod(A, k, m):
    """``A**k mod m`` by square-and-multiply, in Python integers (``k >= 0``)."""
    k = int(k)
    if k < 0:
        raise ValueError("negative power")
    R, S = _EYE, A
    while k:
        if k & 1:
            R = mat_mul_mod(R, S, m)
        S = mat_mul_mod(S, S, m)
        k >>= 1
    return R


def mrg_jump_table(parts, c):
    """int64 ``[parts, 18]``: row ``p`` is ``A1**(p*c) mod M1`` then ``A2**(p*c) mod M2``, row-major.

    The powers ``A**(c * 2**i)`` are Python integers; the rows are filled by doubling, rows
    ``[2**i, 2**(i+1))`` = rows ``[0, 2**i)`` times ``A**(c * 2**i)``, in ``uint64``: entries stay below
    2^31, a product below 2^62 and a sum of three below 2^64, so nothing wraps."""
    parts, c = int(parts), int(c)
    tab = np.zeros((parts, 2, 3, 3), dtype=np.uint64)
    tab[0, 0] = tab[0, 1] = np.asarray(_EYE, dtype=np.uint64)
    for h, (A, m) in enumerate(((A1, M1), (A2, M2))):
        S, n = mat_pow_mod(A, c, m), 1
        while n < parts:
            k = min(n, parts - n)
            B = np.asarray(S, dtype=np.uint64)
            # (X @ B)[i, j] = sum_k X[i, k] * B[k, j]
            prod = tab[:k, h, :, :, None] * B[None, None, :, :]
            tab[n:n + k, h] = prod.sum(axis=2, dtype=np.uint64) % np.uint64(m)
            S = mat_mul_mod(S, S, m)
            n += k
    return tab.reshape(parts, 18).astype(np.int64)


def mrg_parts(n_streams, n_elements, forced=0):
    """Pieces per stream: ``forced`` when positive (``AESARA_HIP_MRG_PARTS``), else the smallest
    count that puts about sixteen wavefronts on every CU, at most one piece per sample."""
    if forced > 0:
        return int(forced)
    j_max = -(-n_elements // n_streams)
    return max(1, min(-(-FILL_LANES // n_streams), j_max))


class RngMixin:

    def _mrg_table(self, parts, c):
        """The jump table on the device, one upload per (parts, c) of this executor (a replayed
        launch list keeps addressing it)."""
        cache = self.__dict__.setdefault("_mrg_tables", {})
        t = cache.get((parts, c))
        if t is None:
            if self._capturing:
                raise HostReadInReplay("jump table uploaded while recording a launch list")
            if len(cache) >= 64:
                cache.pop(next(iter(cache)))
            t = cache[(parts, c)] = self._from_numpy(mrg_jump_table(parts, c))
        return t

    def _op_MrgUniform(self, node, args):
        """reference: rng_mrg.py:401 mrg_uniform.perform / :539 c_code (checks :581-646)."""
        p = node.params
        ndim, dt = int(p["ndim"]), p["dtype"]
        size = self.host_array(args[1])
        if size.ndim != 1:
            raise ValueError("size must be vector")
        if size.shape[0] != ndim:
            raise ValueError("size must have length %i (not %i)" % (ndim, size.shape[0]))
        if size.dtype.kind not in "iu":
            raise TypeError(f"size must hold integers, got {size.dtype}")
        shape = tuple(int(s) for s in size)
        if any(s < 0 for s in shape):
            raise ValueError(f"negative dimensions are not allowed: size {shape}")
        n_elements = _prod(shape)
        if n_elements > M1:
            raise ValueError("rng_mrg does not support more than (2**31 -1) samples")
        rstate = self.to_device(args[0])
        if rstate.ndim != 2:
            raise ValueError("rstate must be matrix")
        if rstate.shape[1] != 6:
            raise ValueError("rstate must have 6 columns")
        if rstate.dtype != "int32":
            raise ValueError("rstate must be int32")
        n_streams = rstate.shape[0]
        sample = self.alloc(shape, dt)
        if p["inplace"]:
            if self._capturing:
                # building a replay entry evaluates the plan and then runs the recorded launches once
                # more: an in-place update of an argument would be applied twice -> eager calls only
                raise HostReadInReplay("in-place state update while recording a launch list")
            if not rstate.is_contiguous():
                raise ValueError("mrg_uniform{inplace}: the state buffer must be contiguous")
            new = rstate
        else:
            new = self.alloc(rstate.shape, "int32")
        if n_streams == 0:
            if n_elements:
                raise ValueError("rstate must have at least one stream")
            return [new, sample]
        src = rstate
        if n_elements == 0:
            # an empty sample: unchanged state, no generator launch
            if new is not rstate:
                self._copy_strided(new, rstate.strides, rstate)
            return [new, sample]
        parts = mrg_parts(n_streams, n_elements, int(knobs.get("MRG_PARTS")))
        if not src.is_contiguous() or (parts > 1 and new is rstate):
            # the pieces of a stream read its old state while the last one stores the new state
            src = self.alloc(rstate.shape, "int32")
            self._copy_strided(src, rstate.strides, rstate)
        table = None
        if parts > 1:
            c = -(-(-(-n_elements // n_streams)) // parts)
            table = self._mrg_table(parts, c)
        self._launch("ahip_mrg_uniform", (dtype_code(dt), _VP(src.ptr), _VP(new.ptr), n_streams,
                                          _VP(sample.ptr), n_elements, parts,
                                          _VP(table.ptr) if table is not None else _VP(), self._stream()))
        return [new, sample]

    def _multinomial_operands(self, node, args):
        """(pvals, unis, n) checked the way both C bodies check them (multinomial.py:84-99)."""
        pvals, unis = self.to_device(args[0]), self.to_device(args[1])
        n = self.host_int(args[2])
        if pvals.ndim != 2:
            raise TypeError("pvals ndim should be 2")
        if unis.ndim != 1:
            raise TypeError("unis ndim should be 2")        # (the reference's words)
        for what, a in (("pvals", pvals), ("unis", unis)):
            if a.dtype not in ("float32", "float64"):
                raise TypeError(f"{node.op}: {what} of dtype {a.dtype} (one of float32 / float64 only)")
        if n < 0:
            raise ValueError(f"{node.op}: n = {n} samples")
        return pvals, unis, n

    def _op_MultinomialFromUniform(self, node, args):
        """reference: multinomial.py:65 MultinomialFromUniform.c_code."""
        pvals, unis, n = self._multinomial_operands(node, args)
        if unis.shape[0] != pvals.shape[0] * n:
            raise ValueError("unis.shape[0] != pvals.shape[0] * n")
        odt = self.plan.vars[node.outputs[0]].dtype
        out = self.alloc(pvals.shape, odt)
        if out.size:
            self._launch("ahip_multinomial_from_uniform",
                         (dtype_code(pvals.dtype), dtype_code(unis.dtype), dtype_code(odt), _VP(pvals.ptr),
                          pvals.strides[0], pvals.strides[1], _VP(unis.ptr), unis.strides[0],
                          pvals.shape[0], pvals.shape[1], n, _VP(out.ptr), self._stream()))
        return [out]

    def _op_ChoiceFromUniform(self, node, args):
        """reference: multinomial.py:261 ChoiceFromUniform.c_code (replace = False)."""
        pvals, unis, n = self._multinomial_operands(node, args)
        nb_multi, nb_outcomes = pvals.shape
        if n > nb_outcomes:
            raise ValueError("Cannot sample without replacement n samples bigger than the size of "
                             "the distribution.")
        if unis.shape[0] != nb_multi * n:
            raise ValueError("unis.shape[0] != pvals.shape[0] * n")
        odt = self.plan.vars[node.outputs[0]].dtype
        out = self.alloc((nb_multi, n), odt)
        if out.size:
            # the private copy of pvals the lanes renormalise: stored outcome-major, so that for one
            # outcome a wavefront's rows are consecutive elements
            ws = self.alloc((nb_outcomes, nb_multi), pvals.dtype).view((nb_multi, nb_outcomes), (1, nb_multi))
            self._copy_strided(ws, pvals.strides, pvals)
            self._launch("ahip_choice_from_uniform",
                         (dtype_code(pvals.dtype), dtype_code(unis.dtype), dtype_code(odt), _VP(ws.ptr),
                          ws.strides[0], ws.strides[1], _VP(unis.ptr), unis.strides[0],
                          nb_multi, nb_outcomes, n, _VP(out.ptr), self._stream()))
        return [out]
