"""Scalar programs as C++ expressions: one node (``scalar_node_expr``), a whole body
(``emit_scalar_body``), what of it is loop invariant or feeds only a sum, reduction
combiners and identities, casts and literals."""
from __future__ import annotations

import numpy as np

from .. import knobs
from .prelude import RTYPE

_FLOAT_FN = {
    "sqrt": "sqrt", "exp": "exp", "exp2": "exp2", "expm1": "expm1", "log": "log",
    "log2": "log2", "log10": "log10", "log1p": "log1p", "sin": "sin", "cos": "cos",
    "tan": "tan", "arcsin": "asin", "arccos": "acos", "arctan": "atan", "sinh": "sinh",
    "cosh": "cosh", "tanh": "tanh", "arcsinh": "asinh", "arccosh": "acosh", "arctanh": "atanh",
    "ceil": "ceil", "floor": "floor", "trunc": "trunc", "round_half_to_even": "rint",
    "erf": "erf", "erfc": "erfc",
    # scalar/math.py: Gamma :283 (tgamma), GammaLn :317 (lgamma), Erfcx :108, Erfinv :173,
    # Erfcinv :219, J0 :978 / J1 :947 (libm j0 / j1), I0 :1064 / I1 :1038 (scipy.special.i0 / i1)
    "gamma": "gamma_", "gammaln": "lgamma", "erfcx": "erfcx", "erfinv": "erfinv",
    "erfcinv": "erfcinv", "j0": "j0", "j1": "j1", "i0": "bessel_i0_", "i1": "bessel_i1_",
}

_IDENT = {  # reduction identities
    "add": lambda dt: "0", "mul": lambda dt: "1", "or": lambda dt: "0", "xor": lambda dt: "0",
    "mul_without_zeros": lambda dt: "0",      # MulWithoutZeros.identity (tensor/math.py:2720)
    "and": lambda dt: "true" if dt == "bool" else "(%s)~(%s)0" % (RTYPE[dt], RTYPE[dt]),
}


def is_float(dt):
    return dt in ("float32", "float64")


def _is_uint(dt):
    return dt.startswith("uint")


def _lit(value, dt):
    """C literal for a scalar constant of dtype ``dt``."""
    if dt == "bool":
        return "true" if value else "false"
    if is_float(dt):
        v = float(value)
        if np.isnan(v):
            return "(%s)NAN" % RTYPE[dt]
        if np.isinf(v):
            return "(%s)(%sINFINITY)" % (RTYPE[dt], "-" if v < 0 else "")
        r = repr(float(np.float32(v))) if dt == "float32" else repr(v)
        if "e" not in r and "." not in r:
            r += ".0"
        return r + ("f" if dt == "float32" else "")
    v = int(value)
    if dt == "int64":
        return "(%dLL)" % v if v > -(2 ** 63) else "(-9223372036854775807LL - 1)"
    if dt == "uint64":
        return "(%dULL)" % v
    return "((%s)%d)" % (RTYPE[dt], v)


def cast(expr, src_dt, dst_dt):
    if src_dt == dst_dt:
        return expr
    if dst_dt == "bool":
        return "((%s) != 0)" % expr
    return "((%s)(%s))" % (RTYPE[dst_dt], expr)


def fname(base, dt):
    if base.endswith("_"):          # an overloaded wrapper of the preamble (float and double forms)
        return base
    return base + ("f" if dt == "float32" else "")


def scalar_node_expr(op, ins, in_dts, dt):
    """C++ expression for one scalar node.  ``ins``: C expressions of the inputs (already in
    their own dtypes ``in_dts``); result must have register type ``RTYPE[dt]``."""
    T = RTYPE[dt]
    c = [cast(e, d, dt) for e, d in zip(ins, in_dts)]  # inputs cast to the output dtype
    if op in ("add", "mul"):
        if dt == "bool":
            return "(" + (" || " if op == "add" else " && ").join(c) + ")"
        return "(" + (" + " if op == "add" else " * ").join(c) + ")"
    if op == "sub":
        return "(%s)(%s - %s)" % (T, c[0], c[1]) if dt != "bool" else "(%s != %s)" % (c[0], c[1])
    if op == "neg":
        return "(%s)(-%s)" % (T, c[0])
    if op == "true_div":
        return "(%s / %s)" % (c[0], c[1])
    if op == "int_div":
        if is_float(dt):
            return "%s(%s / %s)" % (fname("floor", dt), c[0], c[1])
        return "%s<%s>(%s, %s)" % ("udiv_floor" if _is_uint(dt) or dt == "bool" else "idiv_floor",
                                   T, c[0], c[1])
    if op == "mod":
        if is_float(dt):
            return "fmod_py(%s, %s)" % (c[0], c[1])
        return "%s<%s>(%s, %s)" % ("umod" if _is_uint(dt) or dt == "bool" else "imod_py", T,
                                   c[0], c[1])
    if op == "pow":
        if is_float(dt):
            return "%s(%s, %s)" % (fname("pow", dt), c[0], c[1])
        return "%s<%s>(%s, %s)" % ("upow" if _is_uint(dt) or dt == "bool" else "ipow", T, c[0], c[1])
    if op in ("maximum", "minimum"):
        if is_float(dt):
            f = "fmax_nan" if op == "maximum" else "fmin_nan"
        else:
            f = "imax" if op == "maximum" else "imin"
        e = c[0]
        for x in c[1:]:
            e = "%s<%s>(%s, %s)" % (f, T, e, x)
        return e
    if op in ("lt", "gt", "le", "ge", "eq", "neq"):
        sym = {"lt": "<", "gt": ">", "le": "<=", "ge": ">=", "eq": "==", "neq": "!="}[op]
        ct = np.result_type(*[np.dtype(d) for d in in_dts]).name
        if ct not in RTYPE:
            ct = "float64"
        a, b = (cast(e, d, ct) for e, d in zip(ins, in_dts))
        return cast("(%s %s %s)" % (a, sym, b), "bool", dt)
    if op in ("and", "or", "xor"):
        if dt == "bool":
            sym = {"and": "&&", "or": "||", "xor": "!="}[op]
        else:
            sym = {"and": "&", "or": "|", "xor": "^"}[op]
        return "(%s)(" % T + (" %s " % sym).join(c) + ")"
    if op == "invert":
        return "(!%s)" % c[0] if dt == "bool" else "(%s)(~%s)" % (T, c[0])
    if op == "abs":
        if is_float(dt):
            return "%s(%s)" % (fname("fabs", dt), c[0])
        if _is_uint(dt) or dt == "bool":
            return c[0]
        return "(%s)(%s < 0 ? -%s : %s)" % (T, c[0], c[0], c[0])
    if op == "sgn":
        if _is_uint(dt) or dt == "bool":
            return "(%s)(%s != 0)" % (T, c[0])
        if is_float(dt):
            # Sgn.c_code scalar/basic.py:2620: NaN stays NaN (np.sign does the same)
            return "(%s)(%s > 0 ? 1 : (%s < 0 ? -1 : (%s != %s ? NAN : 0)))" % (T, c[0], c[0], c[0], c[0])
        return "(%s)((%s > 0) - (%s < 0))" % (T, c[0], c[0])
    if op == "sqr":
        return "(%s)(%s * %s)" % (T, c[0], c[0]) if dt != "bool" else c[0]
    if op in _FLOAT_FN and is_float(dt):
        return "%s(%s)" % (fname(_FLOAT_FN[op], dt), c[0])
    if op in ("ceil", "floor", "trunc", "round_half_to_even", "round_half_away_from_zero") \
            and not is_float(dt):
        return c[0]
    if op == "round_half_away_from_zero":
        return "round_away(%s)" % c[0]
    if op == "reciprocal":
        return "((%s)1 / %s)" % (T, c[0])
    if op == "sigmoid":
        return "sigmoid_(%s)" % c[0]
    if op == "softplus":
        return "softplus_(%s)" % c[0]
    if op == "log1mexp":
        return "log1mexp_(%s)" % c[0]
    if op == "softsign" and is_float(dt):
        return "(%s / ((%s)1 + %s(%s)))" % (c[0], T, fname("fabs", dt), c[0])
    if op == "ultra_fast_sigmoid" and is_float(dt):
        # UltraFastScalarSigmoid.c_code tensor/nnet/sigm.py:54 (a piecewise tanh approximation): x and z
        # are variables of the OUTPUT type, the arithmetic between them is double (its constants are)
        return ("({ %(T)s ux_ = (%(T)s)(0.5 * (double)%(x)s); const double ua_ = ux_ >= (%(T)s)0 ? (double)ux_ "
                ": (double)(%(T)s)(-ux_); double uz_ = ua_ < 1.7 ? (1.5 * ua_ / (1 + ua_)) : (ua_ < 3 ? "
                "(0.935409070603099 + 0.0458812946797165 * (ua_ - 1.7)) : 0.99505475368673); "
                "const %(T)s uzt_ = (%(T)s)(ux_ >= (%(T)s)0 ? uz_ : -uz_); (%(T)s)(0.5 * ((double)uzt_ + 1.)); })"
                % {"T": T, "x": c[0]})
    if op == "xlogx" and is_float(dt):          # XlogX.c_code tensor/xlogx.py:27
        return "(%s == (%s)0 ? (%s)0 : %s * %s(%s))" % (c[0], T, T, c[0], fname("log", dt), c[0])
    if op == "xlogy0" and is_float(dt):         # XlogY0.c_code tensor/xlogx.py:58
        return "(%s == (%s)0 ? (%s)0 : %s * %s(%s))" % (c[0], T, T, c[0], fname("log", dt), c[1])
    if op in ("gammainc", "gammaincc") and is_float(dt):
        return "(%s)%s((double)%s, (double)%s)" % (T, "gamma_p_" if op == "gammainc" else "gamma_q_", c[0], c[1])
    if op == "chi2sf" and is_float(dt):          # Chi2SF.c_code: 1 - GammaP(k / 2, x / 2), inputs (x, k)
        return "(%s)gamma_q_((double)%s * 0.5, (double)%s * 0.5)" % (T, c[1], c[0])
    if op in ("gammau", "gammal") and is_float(dt):
        return "(%s)%s((double)%s, (double)%s)" % (T, "gamma_upper_" if op == "gammau" else "gamma_lower_",
                                                    c[0], c[1])
    if op == "psi" and is_float(dt):
        return "(%s)psi_as103((double)%s)" % (T, c[0])
    if op == "tri_gamma" and is_float(dt):
        return "(%s)trigamma_as121((double)%s)" % (T, c[0])
    if op == "deg2rad":
        return "(%s * (%s)0.017453292519943295)" % (c[0], T)
    if op == "rad2deg":
        return "(%s * (%s)57.29577951308232)" % (c[0], T)
    if op == "arctan2":
        return "%s(%s, %s)" % (fname("atan2", dt), c[0], c[1])
    if op in ("identity", "cast"):
        return c[0]
    if op == "second":
        return c[1]
    if op == "switch":
        return "((%s) ? %s : %s)" % (cast(ins[0], in_dts[0], "bool"), c[1], c[2])
    if op == "clip":
        return "(%s < %s ? %s : (%s > %s ? %s : %s))" % (c[0], c[1], c[1], c[0], c[2], c[2], c[0])
    if op == "isnan":
        return cast("(%s != %s)" % (ins[0], ins[0]) if is_float(in_dts[0]) else "false", "bool", dt)
    if op == "isinf":
        if is_float(in_dts[0]):
            return cast("(%s(%s) == INFINITY)" % (fname("fabs", in_dts[0]), ins[0]), "bool", dt)
        return cast("false", "bool", dt)
    raise NotImplementedError(f"HIP codegen: scalar op {op!r} for dtype {dt}")


def invariant_nodes(scalar, inv_inputs):
    """Indices of scalar nodes that depend only on loop-invariant operands (scalar inputs with
    all-zero strides, constants, other invariant nodes)."""
    inv = set()

    def is_inv(r):
        return r[0] == "c" or (r[0] == "i" and inv_inputs[r[1]]) or (r[0] == "t" and r[1] in inv)

    for k, n in enumerate(scalar["nodes"]):
        if all(is_inv(r) for r in n["in"]) and n["op"] != "second":
            inv.add(k)
    return inv


# ops through which a perturbation of <= 1.5 ulp stays a perturbation of a few ulp (continuous, no
# jumps, no integer results): what a quotient may pass through on its way to a float sum for the
# reciprocal form of a division to be admissible (``sum_only_nodes``)
_CONTINUOUS = {"add", "sub", "mul", "neg", "exp", "exp2", "expm1", "log", "log2", "log10", "log1p",
               "sqr", "sqrt", "sin", "cos", "tanh", "sinh", "cosh", "arctan", "sigmoid", "softplus",
               "true_div", "reciprocal", "identity", "abs", "erf", "erfc"}


def sum_only_nodes(scalar, red, stored_refs):
    """Scalar nodes whose value reaches memory ONLY as a term of the kernel's own floating-point
    SUM (through continuous functions, never through an element-wise output, a comparison, a
    rounding op or an integer cast).  Such a kernel's result already depends on the order of
    summation at the 1e-16 level, so a quotient in that set may be formed as x * (1/c) (<= 1.5 ulp
    from the IEEE quotient); every other division stays the correctly rounded one."""
    if red is None or red.get("op") != "add" or not is_float(red.get("acc", "")):
        return set()
    nodes, outs = scalar["nodes"], [list(o) for o in scalar["out"]]
    stored_t = {outs[r][1] for r in stored_refs if outs[r][0] == "t"}
    sink = outs[red["ref"]]
    other_out_t = {o[1] for j, o in enumerate(outs) if o[0] == "t" and j != red["ref"]} | stored_t
    ok = {}
    for k in range(len(nodes) - 1, -1, -1):
        good = k not in other_out_t and is_float(nodes[k]["dtype"])
        if good:
            for m in range(k + 1, len(nodes)):
                if any(r[0] == "t" and r[1] == k for r in nodes[m]["in"]):
                    if nodes[m]["op"] not in _CONTINUOUS or not ok.get(m, False):
                        good = False
                        break
        if good and not any(any(r[0] == "t" and r[1] == k for r in nodes[m]["in"])
                            for m in range(k + 1, len(nodes))) and sink != ["t", k]:
            good = False             # feeds nothing: leave it alone
        ok[k] = good
    return {k for k, g in ok.items() if g}


def _is_pow2(v):
    try:
        m, _e = np.frexp(float(v))
        return abs(m) == 0.5 and np.isfinite(float(v))
    except (TypeError, ValueError):
        return False


def emit_scalar_body(scalar, in_exprs, in_dts, indent="      ", suffix="", hoisted=None,
                     only=None, exp_tbl=None, sum_only=()):
    """Lines computing the temporaries of a plan scalar expression; returns (lines, out_exprs,
    out_dtypes).  ``hoisted``: {node index: (name, recip_name | None)} of temporaries already
    computed before the loop (loop-invariant sub-expressions); ``only``: restrict emission to
    that set of nodes (used to emit the invariant prologue itself); ``exp_tbl``: name of the
    wave's 2^(j/64) table in LDS — float64 ``exp`` nodes then go through ``exp_tbl64``."""
    lines = []
    tdt = [n["dtype"] for n in scalar["nodes"]]
    hoisted = hoisted or {}

    def ref(r):
        if r[0] == "i":
            return in_exprs[r[1]], in_dts[r[1]]
        if r[0] == "t":
            if r[1] in hoisted:
                return hoisted[r[1]][0], tdt[r[1]]
            return "t%d%s" % (r[1], suffix), tdt[r[1]]
        return _lit(r[1], r[2]), r[2]

    uses = {}
    for n in scalar["nodes"]:
        for r in n["in"]:
            if r[0] == "t":
                uses[r[1]] = uses.get(r[1], 0) + 1
    for k, n in enumerate(scalar["nodes"]):
        if k in hoisted or (only is not None and k not in only):
            continue
        refs = [ref(r) for r in n["in"]]
        dt = n["dtype"]
        div = n["in"][1] if n["op"] == "true_div" else None
        if (div is not None and is_float(dt) and div[0] == "t" and div[1] in hoisted
                and hoisted[div[1]][1] and refs[1][1] == dt):
            # divisor is loop invariant: correctly-rounded division from its hoisted
            # reciprocal (q = x*r; q += r*fma(-q, c, x)) instead of the full v_div_* sequence
            # (AESARA_HIP_FASTDIV=1, tolerance mode: the rounded product x * r alone, <= 1.5 ulp)
            e = None
            num = n["in"][0]
            # AESARA_HIP_FASTDIV: 0 never / 1 always / 2 (default) only for a quotient that reaches
            # memory solely as a term of this kernel's float sum (``sum_only_nodes``)
            fd = knobs.get("FASTDIV")
            fast = fd == 1 or (fd == 2 and k in sum_only)
            if num[0] == "t" and num[1] not in hoisted \
                    and uses.get(num[1], 0) == 1 and list(num) not in [list(o) for o in scalar["out"]]:
                # (K * y) / c with K = +-2^k a literal: scaling by a power of two is exact, so the
                # quotient is y * (K * r) — K * r is loop invariant (the compiler hoists it), the
                # scaling multiply of every element goes away (config 2: -0.5 * sqr(x - mu))
                m = scalar["nodes"][num[1]]
                if m["op"] == "mul" and len(m["in"]) == 2 and m["dtype"] == dt:
                    for ci in (0, 1):
                        c_, y_ = m["in"][ci], m["in"][1 - ci]
                        if c_[0] == "c" and _is_pow2(c_[1]) and ref(y_)[1] == dt \
                                and (fast or 2.0 ** -8 <= abs(float(c_[1])) <= 2.0 ** 8):
                            e = "%s(%s, %s, %s, %s)" % (
                                "fdiv_rcp_s" if fast else "fdiv_inv_s", ref(y_)[0],
                                _lit(c_[1], dt), refs[1][0], hoisted[div[1]][1])
                            break
            if e is None:
                e = "%s(%s, %s, %s)" % ("fdiv_rcp" if fast else "fdiv_inv",
                                        cast(refs[0][0], refs[0][1], dt), refs[1][0], hoisted[div[1]][1])
        elif exp_tbl and n["op"] == "exp" and dt == "float64":
            e = "exp_tbl64(%s, %s)" % (cast(refs[0][0], refs[0][1], dt), exp_tbl)
        else:
            e = scalar_node_expr(n["op"], [x[0] for x in refs], [x[1] for x in refs], dt)
        lines.append("%sconst %s t%d%s = %s;" % (indent, RTYPE[dt], k, suffix, e))
    outs = [ref(r) for r in scalar["out"]]
    return lines, [o[0] for o in outs], [o[1] for o in outs]


def red_combine(op, acc_dt, a, b):
    T = RTYPE[acc_dt]
    # bool: NO short-circuit operators — `b` is often a cross-lane shuffle that every lane must
    # execute (a lane that skipped it would hand its partner an undefined value)
    if op == "add":
        return "(bool)((int)%s | (int)%s)" % (a, b) if acc_dt == "bool" else "(%s)(%s + %s)" % (T, a, b)
    if op == "mul":
        return "(bool)((int)%s & (int)%s)" % (a, b) if acc_dt == "bool" else "(%s)(%s * %s)" % (T, a, b)
    if op == "mul_without_zeros":
        return "mwz_<%s>(%s, %s)" % (T, a, b)
    if op == "maximum":
        return "%s<%s>(%s, %s)" % ("fmax_nan" if is_float(acc_dt) else "imax", T, a, b)
    if op == "minimum":
        return "%s<%s>(%s, %s)" % ("fmin_nan" if is_float(acc_dt) else "imin", T, a, b)
    sym = {"and": "&", "or": "|", "xor": "^"}[op]
    if acc_dt == "bool":
        return "(bool)((int)%s %s (int)%s)" % (a, sym, b)
    return "(%s)(%s %s %s)" % (T, a, sym, b)


def red_identity(op, acc_dt):
    if op in _IDENT:
        return _IDENT[op](acc_dt)
    info_max = op == "minimum"
    if is_float(acc_dt):
        return "(%s)(%sINFINITY)" % (RTYPE[acc_dt], "" if info_max else "-")
    if acc_dt == "bool":
        return "true" if info_max else "false"
    ii = np.iinfo(acc_dt)
    return _lit(ii.max if info_max else ii.min, acc_dt)


def store_val(expr, src_dt, dst_dt):
    v = cast(expr, src_dt, dst_dt)
    if dst_dt == "bool":
        v = "(unsigned char)(%s)" % v
    return v


IDENTITY_SCALAR = {"n_in": 1, "nodes": [], "out": [["i", 0]]}
