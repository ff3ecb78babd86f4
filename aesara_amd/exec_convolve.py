"""The 1-D convolution of a PlanExecutor: ``Convolve`` (reference: tensor/math.py:3005, perform :3062
``np.convolve(a, v, mode)``) on the kernel of csrc/convolve.hip.

With ``m = len(a) >= n = len(v)`` (NumPy swaps the operands first, so does this) the three modes are windows
``[lo, lo + len)`` of ``full[j] = sum_k v[k] a[j - k]``, ``j`` in ``[0, m + n - 1)``:

    full   (0, m + n - 1)
    valid  (n - 1, m - n + 1)
    same   ((n - 1) // 2, m)        (even ``n`` centres asymmetrically, like NumPy)

and one entry point, ``ahip_convolve``, takes the window.  The operands are read through their element
strides, so ``a[::-1]`` and ``v[::2]`` views are not copied.  The lowering has brought both to the dtype of
the result; integers wrap around like NumPy's.

The output, the number of tap splits and the split workspace (``ahip_convolve_ws_bytes``) follow from the
shapes alone and nothing is read on the host: a call records and replays.  An empty operand raises NumPy's
``ValueError`` on the host, from the shapes, in the call.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_expm.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401

TILE_OUT = 2048                 # AHIP_CONVOLVE_TILE_OUT: outputs a workgroup
TAP_CHUNK = 256                 # AHIP_CONVOLVE_TAP_CHUNK: taps staged in LDS at a time
MODES = ("full", "valid", "same")
DTYPES = ("float32", "float64", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64")


def window(mode, m, n):
    """``(lo, len)`` of the window of ``full`` that ``mode`` returns, for ``m >= n >= 1``."""
    if mode == "full":
        return 0, m + n - 1
    if mode == "valid":
        return n - 1, m - n + 1
    if mode == "same":
        return (n - 1) // 2, m
    raise ValueError("Invalid mode - must be full, valid or same")


class ConvolveMixin:

    def _op_Convolve(self, node, args):
        """reference: math.py:3062 Convolve.perform (np.convolve(a, v, mode=self.mode))."""
        a, v = (self.to_device(x) for x in args)
        dt = self.plan.vars[node.outputs[0]].dtype
        if dt not in DTYPES or a.dtype != dt or v.dtype != dt:
            raise TypeError(f"{node.op}: operands of dtypes {[a.dtype, v.dtype]} for a {dt} result (both in the "
                            f"dtype of the result, one of {', '.join(DTYPES)})")
        if a.ndim != 1 or v.ndim != 1:
            raise ValueError("inputs to `convolve` must be 1-dim.")
        if v.shape[0] > a.shape[0]:             # np.convolve: the longer operand first, then the checks
            a, v = v, a
        m, n = a.shape[0], v.shape[0]
        if m == 0:
            raise ValueError("a cannot be empty")
        if n == 0:
            raise ValueError("v cannot be empty")
        lo, length = window(node.params["mode"], m, n)
        out = self.alloc((length,), dt)
        need = int(lib.ahip_convolve_ws_bytes(dtype_code(dt), m, n, lo, length))
        ws = self.alloc((need,), "uint8") if need else None
        self._launch("ahip_convolve", (dtype_code(dt), _VP(a.ptr), m, a.strides[0], _VP(v.ptr), n, v.strides[0],
                                       lo, length, _VP(out.ptr), _VP(ws.ptr) if ws is not None else None, need,
                                       self._stream()))
        return [out]
