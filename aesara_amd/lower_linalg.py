"""Lowering of the dense solves of ``tensor/slinalg.py`` and ``tensor/nlinalg.py``: ``SolveTriangular``,
``CholeskySolve``, ``Solve``, ``MatrixInverse`` and ``Det`` map one to one onto plan ops of the same
names (csrc/linalg.hip; executor: exec_linalg.py).  The plan parameters are the Op's props, with
``trans`` reduced to 0 / 1 (2 and 'C' are 1 for real operands).

Their gradients are graphs over the same Ops plus ``Dot``, ``tril`` / ``triu``, ``outer`` and Elemwise
(``SolveBase.L_op`` slinalg.py:244, ``SolveTriangular.L_op`` :312, ``MatrixInverse.grad``
nlinalg.py:129, ``Det.grad`` :219), so nothing else is needed for ``aesara.grad`` through them.

``QRFull`` (``nlinalg.qr``, nlinalg.py:403) lowers to the plan op ``QR`` with its ``mode``: two outputs
(``Q, R`` for 'reduced' / 'complete', ``h, tau`` for 'raw') or one ('r').  The Op has no ``grad``, so
neither has the lowering (csrc/qr.hip; executor: exec_linalg.py).

``Cholesky`` and the other decompositions (``Eigh``, ``Eig``, ``SVD``, ``MatrixPinv``, ``Lstsq``,
``Eigvalsh``, ``Expm``, the Lyapunov solvers, ``TensorInv`` / ``TensorSolve``) have no handler: they
are refused by name like every Op without one.

Registered by ``lower._register_handlers`` like lower_pool.py; every handler cites the reference Op
it restates.
"""
from .plan import Node

FLOATS = ("float32", "float64")
ASSUME_A = ("gen", "sym", "her", "pos")
QR_MODES = ("reduced", "complete", "r", "raw")
_TRANS = {0: 0, 1: 1, 2: 1, "N": 0, "T": 1, "C": 1}


def family(name):
    """Every refusal starts like the message of an Op without a handler ("<Op> has no HIP
    lowering"), then names the restriction (``FAMILY`` of lower_pool.py)."""
    return f"{name} has no HIP lowering"


def register(hip_lower, static_shape, UnsupportedOp):                       # noqa: N803
    from aesara.tensor.nlinalg import Det, MatrixInverse, QRFull
    from aesara.tensor.slinalg import CholeskySolve, Solve, SolveTriangular

    from .lower_more import _B

    def _emit(opname, node, ctx, params):
        name = type(node.op).__name__
        odt = str(node.outputs[0].type.dtype)
        dts = [str(i.type.dtype) for i in node.inputs]
        if odt not in FLOATS or any(d not in FLOATS for d in dts):
            raise UnsupportedOp(f"{family(name)} for operands of dtypes {dts} giving {odt} (complex, "
                                "float16 and integer operands stay out: float32 / float64 only)")
        b = _B(ctx, static_shape, UnsupportedOp)
        # a float32 / float64 pair: both go to the dtype make_node declared (SolveBase.make_node
        # slinalg.py:228 asks scipy.linalg.solve on 1 x 1 operands), through the cast Elemwise
        ins = [b.cast(ctx.vid(i), odt) for i in node.inputs]
        outs = [ctx.new(o) for o in node.outputs]
        ctx.plan.nodes.append(Node(opname, ins, outs, params))

    @hip_lower.register(SolveTriangular)
    def _(op, node, ctx):
        # reference: slinalg.py:280 SolveTriangular (perform :301 scipy.linalg.solve_triangular(A, b,
        # lower, trans, unit_diagonal, check_finite); props :283)
        if op.trans not in _TRANS:
            raise UnsupportedOp(f"{family('SolveTriangular')} for trans = {op.trans!r} (one of 0, 1, 2, "
                                "'N', 'T', 'C')")
        _emit("SolveTriangular", node, ctx, {"lower": bool(op.lower), "trans": _TRANS[op.trans],
                                             "unit_diagonal": bool(op.unit_diagonal),
                                             "check_finite": bool(op.check_finite)})

    @hip_lower.register(CholeskySolve)
    def _(op, node, ctx):
        # reference: slinalg.py:130 CholeskySolve (perform :158 scipy.linalg.cho_solve((C, lower), b,
        # check_finite))
        _emit("CholeskySolve", node, ctx, {"lower": bool(op.lower), "check_finite": bool(op.check_finite)})

    @hip_lower.register(Solve)
    def _(op, node, ctx):
        # reference: slinalg.py:365 Solve (perform :388 scipy.linalg.solve(a, b, lower, check_finite,
        # assume_a); props :370)
        if op.assume_a not in ASSUME_A:
            raise UnsupportedOp(f"{family('Solve')} for assume_a = {op.assume_a!r} (one of "
                                f"{', '.join(ASSUME_A)})")
        _emit("Solve", node, ctx, {"assume_a": str(op.assume_a), "lower": bool(op.lower),
                                   "check_finite": bool(op.check_finite)})

    @hip_lower.register(MatrixInverse)
    def _(op, node, ctx):
        # reference: nlinalg.py:100 MatrixInverse (perform :124 np.linalg.inv(x).astype(x.dtype))
        _emit("MatrixInverse", node, ctx, {})

    @hip_lower.register(Det)
    def _(op, node, ctx):
        # reference: nlinalg.py:196 Det (perform :210 np.linalg.det(x) in x's dtype)
        _emit("Det", node, ctx, {})

    @hip_lower.register(QRFull)
    def _(op, node, ctx):
        # reference: nlinalg.py:403 QRFull (perform :441 np.linalg.qr(x, mode); make_node :418 declares
        # float outputs of the operand's item size, so an integer operand is refused by _emit)
        if op.mode not in QR_MODES:
            raise UnsupportedOp(f"{family('QRFull')} for mode = {op.mode!r} (one of "
                                f"{', '.join(QR_MODES)})")
        _emit("QR", node, ctx, {"mode": str(op.mode)})
