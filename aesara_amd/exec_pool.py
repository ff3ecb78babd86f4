"""The pooling Ops of a PlanExecutor: ``Pool``, ``MaxPoolGrad``, ``AvgPoolGrad``, ``MaxPoolGradGrad``
(reference: tensor/signal/pool.py Pool :283, MaxPoolGrad :1162, AveragePoolGrad :1490,
DownsampleFactorMaxGradGrad :1834) on the four kernels of csrc/pool.hip.

``ws`` / ``stride`` / ``pad`` are operands: host integer vectors, constant or not, read at run time.
The geometry (:func:`pool_geometry`) is a function of their values and the operand shapes only, so
a recorded launch list replays for the same shapes.  All four Ops use the windows of the reference's
C implementation (``Pool.c_code`` :840-848), the forward windows: in image coordinates window ``j``
of a dimension with extent ``X`` is ``[max(j*s - p, 0), min(j*s + w - p, X))``.

The image is read through its strides (its leading dimensions collapsed to at most three); the
other operands are contiguous, which is what the Ops that produce them hand over.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_conv.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401
from .lower_pool import MAX_NDIM, MODES


def _out_extent(v, w, s, ignore_border):
    """``Pool.out_shape`` (pool.py:445 compute_out) for one padded extent ``v``."""
    if ignore_border:
        return v // s if w == s else max((v - w) // s + 1, 0)
    return (v - 1) // s + 1 if s >= w else max(0, (v - 1 - w + s) // s) + 1


class PoolGeo:
    """Sizes of one pooling, checked the way the reference's ``make_node`` / ``c_code`` check them.
    ``lead`` / ``img`` / ``out``: leading, pooled-image and pooled-output extents; ``ws`` /
    ``stride`` / ``pad`` as tuples of ``ndim`` ints."""
    __slots__ = ("ndim", "mode", "ignore_border", "lead", "img", "out", "ws", "stride", "pad")

    @property
    def out_shape(self):
        return self.lead + self.out

    @property
    def x_shape(self):
        return self.lead + self.img

    def windows(self, k):
        """[(start, end)] of the windows of pooled dimension ``k``, in image coordinates."""
        w, s, p, X = self.ws[k], self.stride[k], self.pad[k], self.img[k]
        return [(max(j * s - p, 0), min(j * s + w - p, X)) for j in range(self.out[k])]

    def sizes(self, k):
        """Per window of dimension ``k`` its factor of the divisor: 1 (``max`` / ``sum``), the cells
        of the padded image it covers (``average_inc_pad``) or those of the image
        (``average_exc_pad``)."""
        if self.mode in ("max", "sum"):
            return [1] * self.out[k]
        if self.mode == "average_exc_pad":
            return [e - b for b, e in self.windows(k)]
        w, s, P = self.ws[k], self.stride[k], self.img[k] + 2 * self.pad[k]
        return [min(j * s + w, P) - j * s for j in range(self.out[k])]

    def geo_array(self, lead3):
        """The 18 values of the kernels' ``geo``: three pooled dimensions, the missing leading ones
        with extent 1 / window 1 / stride 1 / pad 0."""
        fill = MAX_NDIM - self.ndim
        vals = list(lead3)
        for seq, neutral in ((self.img, 1), (self.out, 1), (self.ws, 1), (self.stride, 1), (self.pad, 0)):
            vals += [neutral] * fill + list(seq)
        return _i64arr(vals)


def _int_vector(name, v, ndim):
    a = np.asarray(v)
    if a.ndim != 1 or a.shape[0] != ndim:
        raise ValueError(f"{name} must be a vector of size {ndim}, got shape {tuple(a.shape)}")
    if a.dtype.kind not in "iu":
        raise TypeError(f"{name} must hold integers, got {a.dtype}")
    return tuple(int(e) for e in a)


def pool_geometry(x_shape, ws, stride, pad, ndim, ignore_border, mode="max"):
    """Output shape, windows and divisors of a pooling of ``x_shape`` — the one place they are
    computed: all four Ops and the tests use it.  Raises what the reference raises (``c_code``
    :679-715, ``make_node`` :524-529) for vectors of the wrong length, non-positive windows or
    strides, negative or too large padding, padding without ``ignore_border`` and, without
    ``ignore_border``, an empty output."""
    ndim = int(ndim)
    if not 1 <= ndim <= MAX_NDIM:
        raise ValueError(f"pooling over {ndim} dimensions (1, 2 or 3 only)")
    if mode not in MODES:
        raise ValueError(f"pooling mode {mode!r}")
    x_shape = tuple(int(s) for s in x_shape)
    if len(x_shape) < ndim:
        raise TypeError(f"pooling over {ndim} dimensions of a {len(x_shape)}-d operand")
    g = PoolGeo()
    g.ndim, g.mode, g.ignore_border = ndim, mode, bool(ignore_border)
    g.ws, g.stride, g.pad = (_int_vector(n, v, ndim) for n, v in
                             (("ws", ws), ("stride", stride), ("pad", pad)))
    if min(g.ws) <= 0:
        raise ValueError(f"pooling window {g.ws} must be positive")
    if min(g.stride) <= 0:
        raise ValueError(f"pooling stride {g.stride} must be positive")
    if min(g.pad) < 0:
        raise ValueError(f"pooling padding {g.pad} must not be negative")
    if max(g.pad) != 0 and not g.ignore_border:
        raise ValueError("padding must be zero when ignore border is False")
    if any(p >= w for p, w in zip(g.pad, g.ws)):
        raise ValueError(f"padding must be smaller than strides: pad {g.pad}, ws {g.ws}")
    g.lead, g.img = x_shape[:len(x_shape) - ndim], x_shape[len(x_shape) - ndim:]
    g.out = tuple(_out_extent(X + 2 * p, w, s, g.ignore_border)
                  for X, w, s, p in zip(g.img, g.ws, g.stride, g.pad))
    if not g.ignore_border and (min(g.out) <= 0 or min(g.img) <= 0):
        raise ValueError(f"pooling of extents {g.img} without ignore_border needs a non-empty "
                         f"image (output extents {g.out})")          # pool.py:562 / :744 assert
    if any(X == 0 and o > 0 for X, o in zip(g.img, g.out)):
        # padding alone would fill a window (the reference reads past the end of the image there)
        raise ValueError(f"pooling of extents {g.img} with pad {g.pad}: a window holds padding only")
    return g


_MODE_CODE = {m: i for i, m in enumerate(MODES)}


class PoolMixin:

    def _pool_geo(self, node, x, args):
        """Geometry from the image and the last three operands (ws, stride, pad: host vectors)."""
        ws, stride, pad = (self.host_array(a) for a in args[-3:])
        p = node.params
        return pool_geometry(x.shape, ws, stride, pad, p["ndim"], p["ignore_border"], p["mode"])

    def _pool_image(self, g, x: DevArray):
        """(x or a copy of it, its three leading extents, its six element strides): the leading
        dimensions collapsed; a copy only if more than three remain."""
        nl = len(g.lead)
        sh, st = collapse_dims(list(x.shape[:nl]), [list(x.strides[:nl])]) if nl else ([1], [[0]])
        if len(sh) > MAX_NDIM:
            x = self._pool_contig(x)        # (not contiguous: a contiguous image collapses to one)
            sh, st = collapse_dims(list(x.shape[:nl]), [list(x.strides[:nl])])
        lead3 = [1] * (3 - len(sh)) + list(sh)
        strides = [0] * (3 - len(sh)) + list(st[0]) + [0] * (MAX_NDIM - g.ndim) + list(x.strides[nl:])
        return x, lead3, _i64arr(strides)

    def _pool_lead3(self, g):
        return [1, 1, _prod(g.lead)]

    def _pool_contig(self, a: DevArray) -> DevArray:
        if a.is_contiguous():
            return a
        out = self.alloc(a.shape, a.dtype)
        self._copy_strided(out, a.strides, a)
        return out

    def _pool_same_shape(self, node, what, a, want, g):
        if tuple(a.shape) != tuple(want):
            raise ValueError(f"{node.op}: an image of shape {g.x_shape} with ws {g.ws}, stride "
                             f"{g.stride} and pad {g.pad} goes with {what} of shape {tuple(want)}, but "
                             f"the given {what} has shape {tuple(a.shape)}")

    def _pool_streaming(self, x: DevArray, g):
        """The streaming policy (exec_elemwise.BIG_STREAM): an image of 96 MiB or more whose
        windows do not overlap is read once, with non-temporal loads."""
        return int(not (knobs.is_set("VECBYTES") or knobs.is_set("NT"))
                   and x.size * x.itemsize >= self.BIG_STREAM
                   and all(s >= w for s, w in zip(g.stride, g.ws)))

    def _op_Pool(self, node, args):
        """reference: pool.py:551 Pool.perform / :657 c_code."""
        (x,), dt = self._float_operands(node, args[:-3])
        g = self._pool_geo(node, x, args)
        out = self.alloc(g.out_shape, dt)
        if out.size == 0:
            return [out]
        x, lead3, xs = self._pool_image(g, x)
        self._launch("ahip_pool_fwd", (dtype_code(dt), _MODE_CODE[g.mode], self._pool_streaming(x, g),
                                       g.geo_array(lead3), _VP(x.ptr), xs, _VP(out.ptr), self._stream()))
        return [out]

    def _op_MaxPoolGrad(self, node, args):
        """reference: pool.py:1266 MaxPoolGrad.c_code."""
        (x, maxout, gz), dt = self._float_operands(node, args[:-3])
        g = self._pool_geo(node, x, args)
        self._pool_same_shape(node, "maxout", maxout, g.out_shape, g)
        self._pool_same_shape(node, "gz", gz, g.out_shape, g)
        out = self.alloc(g.x_shape, dt)
        if out.size == 0:
            return [out]
        x, lead3, xs = self._pool_image(g, x)
        maxout, gz = self._pool_contig(maxout), self._pool_contig(gz)
        self._launch("ahip_maxpool_grad", (dtype_code(dt), g.geo_array(lead3), _VP(x.ptr), xs,
                                           _VP(maxout.ptr), _VP(gz.ptr), _VP(out.ptr), self._stream()))
        return [out]

    def _op_AvgPoolGrad(self, node, args):
        """reference: pool.py:1603 AveragePoolGrad.c_code; x gives its shape only."""
        (x, gz), dt = self._float_operands(node, args[:-3])
        g = self._pool_geo(node, x, args)
        if g.mode == "max":
            raise ValueError(f"{node.op}: mode 'max' has no average gradient")
        if g.mode == "average_exc_pad" and max(g.pad) != 0:
            raise ValueError("padding must be zero for average_exc_pad")      # :1669-1674
        self._pool_same_shape(node, "gz", gz, g.out_shape, g)
        out = self.alloc(g.x_shape, dt)
        if out.size == 0:
            return [out]
        gz = self._pool_contig(gz)
        self._launch("ahip_avgpool_grad", (dtype_code(dt), _MODE_CODE[g.mode],
                                           g.geo_array(self._pool_lead3(g)), _VP(gz.ptr), _VP(out.ptr),
                                           self._stream()))
        return [out]

    def _op_MaxPoolGradGrad(self, node, args):
        """reference: pool.py:1954 DownsampleFactorMaxGradGrad.c_code."""
        (x, maxout, ggx), dt = self._float_operands(node, args[:-3])
        g = self._pool_geo(node, x, args)
        self._pool_same_shape(node, "maxout", maxout, g.out_shape, g)
        self._pool_same_shape(node, "ggx", ggx, g.x_shape, g)
        out = self.alloc(g.out_shape, dt)
        if out.size == 0:
            return [out]
        x, lead3, xs = self._pool_image(g, x)
        maxout, ggx = self._pool_contig(maxout), self._pool_contig(ggx)
        self._launch("ahip_maxpool_gradgrad", (dtype_code(dt), g.geo_array(lead3), _VP(x.ptr), xs,
                                               _VP(maxout.ptr), _VP(ggx.ptr), _VP(out.ptr),
                                               self._stream()))
        return [out]
