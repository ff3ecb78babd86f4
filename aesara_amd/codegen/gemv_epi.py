"""Fused GEMV chain + Elemwise epilogue (``gv_`` kernels)."""
from __future__ import annotations

from .prelude import CTYPE, PRELUDE, RTYPE
from .scalar import cast, emit_scalar_body, store_val
from .spec import Spec

AHIP_MAXDOTS = 8
AHIP_GV_MAXOPS = 16

GV_STRUCT = r"""
#define AHIP_MAXDOTS %d
#define AHIP_GV_MAXOPS %d
struct GvArgs {
  i64 M;
  const void* A[AHIP_MAXDOTS]; i64 a_rs[AHIP_MAXDOTS]; i64 a_cs[AHIP_MAXDOTS]; i64 K[AHIP_MAXDOTS];
  const void* x[AHIP_MAXDOTS]; i64 incx[AHIP_MAXDOTS];
  void* ptr[AHIP_GV_MAXOPS]; i64 stride[AHIP_GV_MAXOPS];
  int ndots; int nops;
  const void* xin[AHIP_MAXDOTS][4]; void* xout[AHIP_MAXDOTS];
};
""" % (AHIP_MAXDOTS, AHIP_GV_MAXOPS)


class GemvEpiSpec(Spec):
    """y[m] = f(dot_0[m], ..., dot_{D-1}[m], operands[m]) with dot_d[m] = A_d[m, :] . x_d.

    Replaces chains of ``Gemv`` nodes (tensor/blas.py:231; ``beta*y + alpha*A.x`` with y another
    Gemv) and the ``Elemwise`` that consumes them — e.g. one GRU gate
    ``sigmoid(W.T x + U.T h) * h`` of BASELINE config 4 — by a single HBM/L2-bound kernel: each
    wavefront owns output rows, streams the D matrix rows with 16-byte loads, reduces with
    cross-lane shuffles and evaluates the scalar epilogue in registers.

    dtype     : float32 | float64 (all matrices / vectors of the dots)
    dot_vec   : per dot, True when rows can be read with 16-byte vectors
    scalar    : plan scalar expression; its first D inputs are the dot results
    in_dtypes : dtypes of the non-dot epilogue operands; out_dtypes/out_refs as in KernelSpec
    """

    def __init__(self, dtype, dot_vec, scalar, in_dtypes, out_dtypes, out_refs, block=256,
                 rpw=1, kvs=None, xprogs=None, nt=False):
        # nt: the matrix rows are read with non-temporal 16-byte loads (a matrix of half the
        # memory-side cache or more is read once as far as the caches go, exec_elemwise.BIG_STREAM)
        self.nt = bool(nt)
        # xprogs: per dot None or {"scalar", "cls": ["v" | "s", ...], "out_ref", "store"}: the
        # dot's vector is an Elemwise of <= 4 vectors / scalars, evaluated while it is loaded
        # (and stored by the first wavefront when something else reads it).  Needs kvs.
        self.xprogs = list(xprogs) if xprogs and any(xprogs) else None
        assert not self.xprogs or kvs
        self.rpw = rpw  # rows per wavefront iteration (4 for short rows, 1 for long rows)
        # kvs: per dot, 16-byte vectors per lane (K = 64 * VEC * kv) when every row length is
        # such a multiple and small: the kernel is then specialised on the lengths and issues
        # ALL row loads of ALL dots before the first FMA (one memory round trip per wavefront
        # instead of one per loop iteration per dot — short kernels are latency-, not
        # bandwidth-bound: BASELINE config 4 step kernels 4.5 -> see DESIGN §3.3)
        self.kvs = list(kvs) if kvs else None
        self.dtype = dtype
        self.dot_vec = list(dot_vec)
        self.scalar = scalar
        self.in_dtypes = list(in_dtypes)
        self.out_dtypes = list(out_dtypes)
        self.out_refs = list(out_refs)
        self.block = block
        assert 1 <= len(self.dot_vec) <= AHIP_MAXDOTS
        assert len(self.in_dtypes) + len(self.out_dtypes) <= AHIP_GV_MAXOPS

    def source_fields(self):
        return ["gv4", self.dtype, self.dot_vec, self.scalar, self.in_dtypes,
                self.out_dtypes, self.out_refs, self.block, self.rpw, self.kvs,
                self.xprogs] + (["nt"] if self.nt else [])

    def generate(self):
        return generate_gemv_epilogue(self)


def generate_gemv_epilogue(spec: GemvEpiSpec):
    T = RTYPE[spec.dtype]
    V = 4 if spec.dtype == "float32" else 2
    D = len(spec.dot_vec)
    R = spec.rpw
    nin, nout = len(spec.in_dtypes), len(spec.out_dtypes)
    name = "gv_" + spec.digest()
    waves = spec.block // 64
    L = [PRELUDE, GV_STRUCT]
    LD = "nt_load(%s)" if spec.nt else "*%s"          # how a 16-byte piece of a matrix row is read
    L.append('extern "C" __global__ __launch_bounds__(%d) void %s(GvArgs a) {' % (spec.block, name))
    L.append("  const int lane = threadIdx.x & 63;")
    L.append("  const i64 nwaves = (i64)gridDim.x * %d;" % waves)
    # each wavefront owns R consecutive output rows per iteration: for short rows (K*itemsize of
    # a few KB) this keeps R independent 16-byte loads in flight per lane instead of one
    L.append("  for (i64 m0 = ((i64)blockIdx.x * %d + (threadIdx.x >> 6)) * %d; m0 < a.M; "
             "m0 += nwaves * %d) {" % (waves, R, R))
    if spec.kvs:
        # ---- fixed lengths: loads of every dot first, then FMAs, then interleaved reductions
        for d in range(D):
            L.append("    const %s* __restrict__ xv%d = (const %s*)a.x[%d];" % (T, d, T, d))
            for r in range(R):
                L.append("    const %s* __restrict__ row%d_%d = (const %s*)a.A[%d] + "
                         "((m0 + %d < a.M) ? (m0 + %d) : (a.M - 1)) * a.a_rs[%d];"
                         % (T, d, r, T, d, r, r, d))
        for d in range(D):
            xp = spec.xprogs[d] if spec.xprogs else None
            for j in range(spec.kvs[d]):
                for r in range(R):
                    L.append("    const Pack<%s, %d> a%d_%d_%d = %s;" % (T, V, d, r, j, LD % (
                        "(const Pack<%s, %d>*)(row%d_%d + (%d + lane) * %d)" % (T, V, d, r, j * 64, V))))
                if xp is None:
                    L.append("    const Pack<%s, %d> x%d_%d = *(const Pack<%s, %d>*)(xv%d + (%d + lane) * %d);"
                             % (T, V, d, j, T, V, d, j * 64, V))
                else:
                    for q, c in enumerate(xp["cls"]):
                        if c == "v":
                            L.append("    const Pack<%s, %d> xi%d_%d_%d = *(const Pack<%s, %d>*)"
                                     "((const %s*)a.xin[%d][%d] + (%d + lane) * %d);"
                                     % (T, V, d, q, j, T, V, T, d, q, j * 64, V))
                        elif j == 0:
                            L.append("    const %s xs%d_%d = *(const %s*)a.xin[%d][%d];" % (T, d, q, T, d, q))
        # vector prologues: x_d evaluated from its operands, stored once if something reads it
        for d in range(D):
            xp = spec.xprogs[d] if spec.xprogs else None
            if xp is None:
                continue
            for j in range(spec.kvs[d]):
                L.append("    Pack<%s, %d> x%d_%d;" % (T, V, d, j))
                for e in range(V):
                    ins_ = ["xi%d_%d_%d.v[%d]" % (d, q, j, e) if c == "v" else "xs%d_%d" % (d, q)
                            for q, c in enumerate(xp["cls"])]
                    lines, oe, od = emit_scalar_body(xp["scalar"], ins_, [spec.dtype] * len(ins_),
                                                     indent="    ", suffix="_xp%d_%d_%d" % (d, j, e))
                    L.extend(lines)
                    L.append("    x%d_%d.v[%d] = %s;" % (d, j, e, cast(oe[xp["out_ref"]],
                                                                         od[xp["out_ref"]], spec.dtype)))
                if xp["store"]:
                    L.append("    if (m0 == 0) *(Pack<%s, %d>*)((%s*)a.xout[%d] + (%d + lane) * %d) = x%d_%d;"
                             % (T, V, T, d, j * 64, V, d, j))
        for d in range(D):
            for r in range(R):
                terms = ["a%d_%d_%d.v[%d] * x%d_%d.v[%d]" % (d, r, j, e, d, j, e)
                         for j in range(spec.kvs[d]) for e in range(V)]
                # two interleaved accumulation chains per dot (as the generic loop does)
                L.append("    %s d%d_%d = (%s) + (%s);" % (T, d, r, " + ".join(terms[0::2]),
                                                          " + ".join(terms[1::2]) if terms[1::2] else "0"))
        L.append("    for (int s = 32; s > 0; s >>= 1) {")
        for d in range(D):
            for r in range(R):
                L.append("      d%d_%d += shfl_xor_<%s>(d%d_%d, s);" % (d, r, T, d, r))
        L.append("    }")
    for d in (range(D) if not spec.kvs else []):
        for r in range(R):
            L.append("    %s d%d_%d = 0;" % (T, d, r))
        L.append("    {")
        L.append("      const %s* __restrict__ xv = (const %s*)a.x[%d];" % (T, T, d))
        L.append("      const i64 K = a.K[%d];" % d)
        for r in range(R):
            # rows past M are clamped to the last row (their results are never stored)
            L.append("      const %s* __restrict__ row%d = (const %s*)a.A[%d] + "
                     "((m0 + %d < a.M) ? (m0 + %d) : (a.M - 1)) * a.a_rs[%d];" % (T, r, T, d, r, r, d))
        if spec.dot_vec[d]:
            L.append("      const i64 nv = K / %d;" % V)
            if R == 1:
                L.append("      %s e0 = 0, e1 = 0;" % T)
                L.append("      i64 v = lane;")
                L.append("      for (; v + 64 < nv; v += 128) {")
                L.append("        const Pack<%s, %d> a0 = %s;" % (T, V, LD % ("(const Pack<%s, %d>*)(row0 + v * %d)" % (T, V, V))))
                L.append("        const Pack<%s, %d> a1 = %s;" % (T, V, LD % ("(const Pack<%s, %d>*)(row0 + (v + 64) * %d)" % (T, V, V))))
                L.append("        const Pack<%s, %d> x0 = *(const Pack<%s, %d>*)(xv + v * %d);" % (T, V, T, V, V))
                L.append("        const Pack<%s, %d> x1 = *(const Pack<%s, %d>*)(xv + (v + 64) * %d);" % (T, V, T, V, V))
                for e in range(V):
                    L.append("        e0 += a0.v[%d] * x0.v[%d]; e1 += a1.v[%d] * x1.v[%d];" % (e, e, e, e))
                L.append("      }")
                L.append("      for (; v < nv; v += 64) {")
                L.append("        const Pack<%s, %d> a0 = %s;" % (T, V, LD % ("(const Pack<%s, %d>*)(row0 + v * %d)" % (T, V, V))))
                L.append("        const Pack<%s, %d> x0 = *(const Pack<%s, %d>*)(xv + v * %d);" % (T, V, T, V, V))
                for e in range(V):
                    L.append("        e0 += a0.v[%d] * x0.v[%d];" % (e, e))
                L.append("      }")
                L.append("      d%d_0 = e0 + e1;" % d)
            else:
                L.append("      for (i64 v = lane; v < nv; v += 64) {")
                L.append("        const Pack<%s, %d> x0 = *(const Pack<%s, %d>*)(xv + v * %d);" % (T, V, T, V, V))
                for r in range(R):
                    L.append("        const Pack<%s, %d> a%d = %s;" % (T, V, r, LD % (
                        "(const Pack<%s, %d>*)(row%d + v * %d)" % (T, V, r, V))))
                for r in range(R):
                    for e in range(V):
                        L.append("        d%d_%d += a%d.v[%d] * x0.v[%d];" % (d, r, r, e, e))
                L.append("      }")
        else:
            L.append("      const i64 cs = a.a_cs[%d], ix = a.incx[%d];" % (d, d))
            L.append("      for (i64 k = lane; k < K; k += 64) {")
            L.append("        const %s xk = xv[k * ix];" % T)
            for r in range(R):
                L.append("        d%d_%d += row%d[k * cs] * xk;" % (d, r, r))
            L.append("      }")
        for r in range(R):
            L.append("      for (int s = 32; s > 0; s >>= 1) d%d_%d += shfl_xor_<%s>(d%d_%d, s);"
                     % (d, r, T, d, r))
        L.append("    }")
    for r in range(R):
        L.append("    if (m0 + %d < a.M) {" % r)
        L.append("      const i64 m = m0 + %d;" % r)
        ins = ["d%d_%d" % (d, r) for d in range(D)]
        in_dts = [spec.dtype] * D
        for k in range(nin):
            ct = CTYPE[spec.in_dtypes[k]]
            L.append("      const %s x%d = ((const %s*)a.ptr[%d])[m * a.stride[%d]];" % (ct, k, ct, k, k))
            ins.append("(x%d != 0)" % k if spec.in_dtypes[k] == "bool" else "x%d" % k)
            in_dts.append(spec.in_dtypes[k])
        lines, outs, odts = emit_scalar_body(spec.scalar, ins, in_dts, indent="      ")
        L.extend(lines)
        L.append("      if (lane == 0) {")
        for k, ri in enumerate(spec.out_refs):
            val = store_val(outs[ri], odts[ri], spec.out_dtypes[k])
            L.append("        ((%s*)a.ptr[%d])[m * a.stride[%d]] = %s;" %
                     (CTYPE[spec.out_dtypes[k]], nin + k, nin + k, val))
        L.append("      }")
        L.append("    }")
    L.append("  }")
    L.append("}")
    return "\n".join(L) + "\n", (name,)
