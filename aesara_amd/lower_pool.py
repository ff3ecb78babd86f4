"""Lowering of the pooling family of ``tensor/signal/pool.py``: ``Pool``, ``MaxPoolGrad``,
``AveragePoolGrad`` and ``DownsampleFactorMaxGradGrad`` map one to one onto the plan ops ``Pool`` /
``MaxPoolGrad`` / ``AvgPoolGrad`` / ``MaxPoolGradGrad`` (csrc/pool.hip; executor: exec_pool.py).
``ws`` / ``stride`` / ``pad`` stay graph inputs (host integer vectors at run time), so constant and
symbolic ones lower alike; the plan parameters are the Op's ``mode``, ``ignore_border`` and ``ndim``.

Registered by ``lower._register_handlers`` like lower_conv.py; every handler cites the reference Op
it restates.
"""

MODES = ("max", "sum", "average_inc_pad", "average_exc_pad")
MAX_NDIM = 3
# every refusal starts like the message of an Op without a handler ("<Op> has no HIP lowering"), then
# names the restriction: the part of tensor/signal/pool.py that stays out of scope is filed with it
FAMILY = "Pool has no HIP lowering"


def register(hip_lower, static_shape, UnsupportedOp):                       # noqa: N803
    from aesara.tensor.signal.pool import (AveragePoolGrad, DownsampleFactorMaxGradGrad, MaxPoolGrad,
                                           MaxPoolRop, Pool)

    def _pool(opname, op, node, ctx, n_data):
        name = type(op).__name__
        ndim = int(op.ndim)
        if not 1 <= ndim <= MAX_NDIM:
            raise UnsupportedOp(f"{FAMILY} for ndim = {ndim} ({name}: pooling over 1, 2 or 3 dimensions only)")
        if op.mode not in MODES:
            raise UnsupportedOp(f"{FAMILY} for mode {op.mode!r} ({name}: one of {', '.join(MODES)})")
        dts = [str(i.type.dtype) for i in node.inputs[:n_data]] + [str(node.outputs[0].type.dtype)]
        if any(d not in ("float32", "float64") or d != dts[0] for d in dts):
            raise UnsupportedOp(f"{FAMILY} for {name} over dtypes {dts} (one of float32 / float64 only)")
        if len(node.inputs) != n_data + 3:
            raise UnsupportedOp(f"{FAMILY} for {name} with {len(node.inputs)} inputs (the ws / stride / pad "
                                "operands are required)")
        ctx.emit(opname, node, {"mode": str(op.mode), "ignore_border": bool(op.ignore_border),
                                "ndim": ndim})

    @hip_lower.register(Pool)
    def _(op, node, ctx):
        # reference: pool.py:283 Pool(x, ws, stride, pad) (out_shape :326, perform :551, c_code
        # :657: windows :840-848, max :869-908, sum / averages :909-955)
        _pool("Pool", op, node, ctx, 1)

    @hip_lower.register(MaxPoolGrad)
    def _(op, node, ctx):
        # reference: pool.py:1162 MaxPoolGrad(x, maxout, gz, ws, stride, pad) (c_code :1266: the
        # forward windows :1413-1421, gx += gz where x == maxout :1467; perform :1197 shifts its
        # windows under padding, which is NOT followed)
        _pool("MaxPoolGrad", op, node, ctx, 3)

    @hip_lower.register(AveragePoolGrad)
    def _(op, node, ctx):
        # reference: pool.py:1490 AveragePoolGrad(x, gz, ws, stride, pad) (c_code :1603: windows and
        # their sizes :1751-1762, val = gz / size :1784-1791, gx += val :1813; perform :1528)
        _pool("AvgPoolGrad", op, node, ctx, 2)

    @hip_lower.register(DownsampleFactorMaxGradGrad)
    def _(op, node, ctx):
        # reference: pool.py:1834 DownsampleFactorMaxGradGrad(x, maxout, ggx, ws, stride, pad)
        # (c_code :1954: windows :2066-2074, ggz += ggx where x == maxout :2120; perform :1876)
        _pool("MaxPoolGradGrad", op, node, ctx, 3)

    @hip_lower.register(MaxPoolRop)
    def _(op, node, ctx):
        # reference: pool.py:2142 MaxPoolRop (the R-operator of a max pool)
        raise UnsupportedOp(f"{FAMILY} for MaxPoolRop (the R-operator of max pooling): Pool, MaxPoolGrad, "
                            "AveragePoolGrad and DownsampleFactorMaxGradGrad only")
