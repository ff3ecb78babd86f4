"""Lowering of the MRG31k3p random streams of ``aesara/sandbox``: ``rng_mrg.mrg_uniform``,
``multinomial.MultinomialFromUniform`` and ``multinomial.ChoiceFromUniform`` map one to one onto the
plan ops ``MrgUniform`` / ``MultinomialFromUniform`` / ``ChoiceFromUniform`` (csrc/rng.hip; executor:
exec_rng.py).  Everything else ``MRG_RandomStream`` offers (``uniform(low, high)``, ``binomial``,
``normal``, ``truncated_normal``, ``multinomial``, ``choice``) is a graph over these three made of Ops
that already have kernels.

The generator state is an ordinary ``int32 [n_streams, 6]`` tensor that goes in and comes out;
``size`` and ``n`` stay graph inputs (host integers at run time), so constant and symbolic ones lower
alike.  ``aesara.tensor.random`` (NumPy ``Generator`` objects as graph values) stays out of scope.

Registered by ``lower._register_handlers`` like lower_pool.py; every handler cites the reference Op
it restates.
"""

SAMPLE_DTYPES = ("float32", "float64")
# refusals start like the message of an Op without a handler ("<Op> has no HIP lowering"), then name
# the restriction
UNIFORM = "mrg_uniform has no HIP lowering"
CHOICE = "ChoiceFromUniform has no HIP lowering"
MULTINOMIAL = "MultinomialFromUniform has no HIP lowering"


def register(hip_lower, static_shape, UnsupportedOp):                       # noqa: N803
    from aesara.sandbox.multinomial import ChoiceFromUniform, MultinomialFromUniform
    from aesara.sandbox.rng_mrg import mrg_uniform

    @hip_lower.register(mrg_uniform)
    def _(op, node, ctx):
        # reference: rng_mrg.py:373 mrg_uniform(rstate, size) -> (new rstate, sample) (perform :401,
        # C body :452-537, checks :581-646); float16 has no compiled path there either (:543)
        dt = str(op.output_type.dtype)
        if dt not in SAMPLE_DTYPES:
            raise UnsupportedOp(f"{UNIFORM} for {dt} samples (one of float32 / float64 only)")
        ctx.emit("MrgUniform", node, {"inplace": bool(op.inplace), "ndim": int(op.output_type.ndim),
                                      "dtype": dt})

    def _pvals_unis(family, op, node):
        dts = [str(i.type.dtype) for i in node.inputs[:2]]
        if any(d not in SAMPLE_DTYPES for d in dts):
            raise UnsupportedOp(f"{family} for pvals / unis of dtypes {dts} (float32 / float64 only)")
        if len(node.inputs) != 3:
            raise UnsupportedOp(f"{family} with {len(node.inputs)} inputs (pvals, unis, n)")

    # (registered before its subclass; singledispatch picks the most specific class either way)
    @hip_lower.register(MultinomialFromUniform)
    def _(op, node, ctx):
        # reference: multinomial.py:14 MultinomialFromUniform(pvals, unis, n) (C body :84-161; the
        # Python perform :166 raises IndexError where the C body writes a row of zeros: C is followed)
        _pvals_unis(MULTINOMIAL, op, node)
        ctx.emit("MultinomialFromUniform", node, {"odtype": str(op.odtype)})

    @hip_lower.register(ChoiceFromUniform)
    def _(op, node, ctx):
        # reference: multinomial.py:223 ChoiceFromUniform(pvals, unis, n) (C body :279-388)
        if op.replace:
            raise UnsupportedOp(f"{CHOICE} for replace=True (sampling without replacement only)")
        _pvals_unis(CHOICE, op, node)
        ctx.emit("ChoiceFromUniform", node, {"odtype": str(op.odtype)})
