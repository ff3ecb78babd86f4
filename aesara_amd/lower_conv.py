"""Lowering of the 2-d convolution family of ``tensor/nnet/abstract_conv.py``: ``AbstractConv2d``,
``AbstractConv2d_gradWeights`` and ``AbstractConv2d_gradInputs`` map one to one onto the plan ops
``Conv2d`` / ``Conv2dGradW`` / ``Conv2dGradI`` (csrc/conv.hip + the MFMA GEMM; executor:
exec_conv.py).  The linker's rewrite query keeps the abstract Ops in the graph (linker.HIP_QUERY).

Registered by ``lower._register_handlers`` like lower_more.py; every handler cites the reference Op
it restates.
"""


def normalise_border_mode(border_mode):
    """``border_mode`` of a ``BaseAbstractConv`` (abstract_conv.py:2157-2203: ``"valid"`` / ``"full"``
    / ``"half"`` or a pair whose members are ints or pairs of ints) as the plan parameter: the
    symbols ``"half"`` / ``"full"`` (their padding depends on the dilated kernel size, a run-time
    value) or ``[[top, bottom], [left, right]]``."""
    if border_mode in ("half", "full"):
        return border_mode
    if border_mode == "valid":
        return [[0, 0], [0, 0]]
    if isinstance(border_mode, int):
        border_mode = (border_mode, border_mode)
    out = []
    for m in border_mode:
        out.append([int(m), int(m)] if isinstance(m, int) else [int(m[0]), int(m[1])])
    if len(out) != 2:
        raise ValueError(f"invalid border_mode {border_mode} which must be a tuple of length 2")
    return out


def resolve_pad(border_mode, dil_kshp):
    """The plan parameter and the dilated kernel size -> ``((top, bottom), (left, right))``, what
    ``border_mode_to_pad`` (abstract_conv.py:603) gives for the Op's ``border_mode``."""
    if border_mode == "full":
        return tuple((int(k) - 1,) * 2 for k in dil_kshp)
    if border_mode == "half":
        return tuple((int(k) // 2,) * 2 for k in dil_kshp)
    return tuple((int(a), int(b)) for a, b in border_mode)


def register(hip_lower, static_shape, UnsupportedOp):                       # noqa: N803
    from aesara.tensor.nnet.abstract_conv import (AbstractConv2d, AbstractConv2d_gradInputs,
                                                  AbstractConv2d_gradWeights, BaseAbstractConv)

    def _conv(opname, op, node, ctx):
        if op.convdim != 2:
            raise UnsupportedOp(f"{type(op).__name__}: convdim = {op.convdim} (2-d convolutions only)")
        if op.unshared:
            raise UnsupportedOp(f"{type(op).__name__} with unshared=True (shared kernels only)")
        dts = [str(i.type.dtype) for i in node.inputs[:2]] + [str(node.outputs[0].type.dtype)]
        if any(d not in ("float32", "float64") or d != dts[0] for d in dts):
            raise UnsupportedOp(f"{type(op).__name__} over dtypes {dts} (one of float32 / float64 only)")
        ctx.emit(opname, node, {
            "border_mode": normalise_border_mode(op.border_mode),
            "subsample": [int(s) for s in op.subsample],
            "filter_dilation": [int(d) for d in op.filter_dilation],
            "filter_flip": bool(op.filter_flip),
            "num_groups": int(op.num_groups)})

    @hip_lower.register(AbstractConv2d)
    def _(op, node, ctx):
        # reference: abstract_conv.py:2646 AbstractConv2d (perform :2501: zero-padded image,
        # convolve2d per channel pair, [::subsample]) -> im2col + one batched GEMM per group
        _conv("Conv2d", op, node, ctx)

    @hip_lower.register(AbstractConv2d_gradWeights)
    def _(op, node, ctx):
        # reference: abstract_conv.py:2990 AbstractConv2d_gradWeights (perform :2834); inputs
        # (img, topgrad, shape): ``shape`` = the kernel's (kh, kw), a host integer vector
        _conv("Conv2dGradW", op, node, ctx)

    @hip_lower.register(AbstractConv2d_gradInputs)
    def _(op, node, ctx):
        # reference: abstract_conv.py:3361 AbstractConv2d_gradInputs (perform :3191); inputs
        # (kern, topgrad, shape): ``shape`` = the image's (H, W), a host integer vector
        _conv("Conv2dGradI", op, node, ctx)

    @hip_lower.register(BaseAbstractConv)
    def _(op, node, ctx):
        # the 3-d Ops (AbstractConv3d and its gradients)
        raise UnsupportedOp(f"{type(op).__name__}: convdim = {op.convdim} (2-d convolutions only)")
