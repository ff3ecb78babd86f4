"""HIP source generator for the fused broadcast Elemwise / CAReduce kernels (K1, K2, K3).

Plays the role of the reference's per-Op C generators — ``Elemwise._c_all``
(tensor/elemwise.py:835), ``elemwise_cgen.make_loop`` / ``make_reordered_loop`` (:228/:305),
``CAReduce._c_all`` (:1522) and ``Composite.c_code_template`` (scalar/basic.py:4250) — but emits
one gfx950 kernel per fused group instead of a CPU loop nest:

* one lane handles ``VEC`` consecutive elements of the innermost (collapsed) dimension with
  16-byte global loads; outer dimensions are index arithmetic over at most ``AHIP_MAXD``
  collapsed dims; a grid-stride loop covers the rest (HBM-bound streaming shape);
* broadcast operands (stride 0 on the inner dim) are loaded once per lane, not per element;
* a CAReduce consumer is fused into the same kernel: per-lane accumulation in the reference's
  accumulator dtype (``CAReduce._acc_dtype`` :1371), wavefront reduction with cross-lane
  shuffles, one partial per workgroup, and a deterministic fixed-order finalize.

The scalar bodies restate the ``c_code`` of the reference ScalarOps (scalar/basic.py,
scalar/math.py) for the supported dtypes (bool, (u)int8-64, float32/64).
"""
from __future__ import annotations

from .. import knobs
from .._lib import AHIP_MAXD, AHIP_MAXOPS
from .finalize import reduce_all_finalize
from .prelude import CTYPE, PRELUDE, RTYPE
from .scalar import (cast, emit_scalar_body, invariant_nodes, is_float, red_combine, red_identity,
                     store_val, sum_only_nodes)
from .spec import Spec


class KernelSpec(Spec):
    """Everything that determines the generated source of one fused kernel.

    scalar      : plan scalar expression (dict)
    in_dtypes   : dtypes of the Elemwise inputs
    out_dtypes  : dtypes of the materialised Elemwise outputs (may be empty for pure reduce)
    out_refs    : indices into scalar["out"] that are stored
    inner       : per-operand (inputs then stored outputs) inner-dim class: 'c' unit stride,
                  'b' broadcast (stride 0), 's' arbitrary stride (forces vec == 1)
    nd          : number of collapsed dims (elemwise / reduce_all) or nk + nr (reduce_axis)
    vec, block  : elements per lane along the inner dim; threads per workgroup
    idx64       : use 64-bit index arithmetic
    reduce      : None | dict(kind='all'|'row'|'col', op=, acc=, out=, ref=<scalar out index>,
                  nk=, nr=)
    """

    def __init__(self, scalar, in_dtypes, out_dtypes, out_refs, inner, nd, vec, block=256,
                 idx64=False, reduce=None, unroll=1, nt=False, invariant=None, tile_dim=None,
                 early=None, blocked=None, trace=None, fast_exp=None, hjobs=False):
        self.scalar = scalar
        # horizontal fusion: the kernel takes an ArgsH block — several independent jobs of this
        # one specialisation in one grid (flat full reductions only)
        self.hjobs = bool(hjobs)
        flat_all = (reduce is not None and reduce.get("kind") == "all" and tile_dim is None
                    and nd == 1 and vec > 1)
        # flat full reductions: the first group of loads is issued before the invariant prologue
        # (its dependent scalar loads and the reciprocal would otherwise delay them ~0.3 us)
        self.early = bool(knobs.get("EARLY") if early is None else early) and flat_all
        # one contiguous chunk of the stream per workgroup instead of a grid-stride walk
        self.blocked = int(knobs.get("RED_BLOCKED") if blocked is None else blocked) if flat_all else 0
        # plain flat Elemwise streams (no reduction): the same walks, off unless measured better
        if reduce is None and tile_dim is None and nd == 1 and vec > 1:
            # (plain Elemwise streams keep the grid-stride walk: the blocked walks lose there,
            # profiles/r04_cfg1b_stream_walks.txt — the STREAM_BLOCKED switch is gone)
            self.blocked = int(0 if blocked is None else blocked)
        if self.hjobs:
            assert flat_all and len(in_dtypes) + len(out_dtypes) <= 6, "hjobs: flat full reductions only"
            self.blocked = 1                    # a contiguous chunk per workgroup inside its job
        # per-workgroup s_memrealtime stamps into the reduce workspace (tools/ew_trace.py)
        self.trace = bool(knobs.get("EW_TRACE") if trace is None else trace) and \
            reduce is not None and reduce.get("kind") == "all" and tile_dim is None
        # float64 exp through the LDS table (exp_tbl64); only where the scalar program has one
        self.fast_exp = bool(knobs.get("FASTEXP") if fast_exp is None else fast_exp) and \
            tile_dim is None and any(n["op"] == "exp" and n["dtype"] == "float64"
                                     for n in scalar["nodes"])
        self.in_dtypes = list(in_dtypes)
        self.out_dtypes = list(out_dtypes)
        self.out_refs = list(out_refs)
        self.inner = list(inner)
        self.nd = nd
        self.vec = vec
        self.block = block
        self.idx64 = idx64
        self.reduce = reduce
        self.unroll = unroll   # independent vectors in flight per lane (flat 1-d shape only)
        self.nt = nt           # non-temporal (streaming) loads for read-once operands
        # per-input flag: operand is a true scalar (all strides zero) -> loop invariant
        self.invariant = list(invariant) if invariant else [False] * len(self.in_dtypes)
        # tiled form (generate_tiled): dim whose 64-element runs are staged through LDS for the
        # operands of class 't' (unit stride along tile_dim instead of along the last dim)
        self.tile_dim = tile_dim
        assert len(self.inner) == len(self.in_dtypes) + len(self.out_dtypes)
        assert 1 <= nd <= AHIP_MAXD and len(self.inner) <= AHIP_MAXOPS

    def source_fields(self):
        return [self.scalar, self.in_dtypes, self.out_dtypes, self.out_refs,
                self.inner, self.nd, self.vec, self.block, self.idx64, self.reduce,
                self.unroll, self.nt, self.invariant, "v10", self._variant()] + \
            ([["tile2", self.tile_dim]] if self.tile_dim is not None else [])

    def _variant(self):
        return "r4%d%d%d%d%d%s%s" % (self.early, self.blocked, self.trace, self.fast_exp, 0,
                                     "H" if self.hjobs else "", "D%d" % knobs.get("FASTDIV"))

    def generate(self):
        return generate(self)


def _offset_code(spec, nops, nd_lo, nd_hi, var, idx_t, inner_vecs=None):
    """Index decomposition of `var` over dims [nd_lo, nd_hi) (outermost first), accumulating
    per-operand offsets into off<k>.  If inner_vecs, the innermost dim is counted in vectors
    and its index is left in `inner` (not multiplied into the offsets)."""
    L = []
    dims = list(range(nd_lo, nd_hi))
    L.append("      %s rem = %s;" % (idx_t, var))
    for pos, d in enumerate(reversed(dims)):
        last = pos == len(dims) - 1
        is_inner = (d == nd_hi - 1) and inner_vecs
        ext = inner_vecs if is_inner else "(%s)a.shape[%d]" % (idx_t, d)
        if last:
            L.append("      { const %s r = rem;" % idx_t)
        else:
            L.append("      { const %s q = rem / %s; const %s r = rem - q * %s; rem = q;" %
                     (idx_t, ext, idx_t, ext))
        if is_inner:
            L.append("        inner = r;")
        else:
            for k in range(nops):
                L.append("        off%d += (i64)r * a.stride[%d][%d];" % (k, k, d))
        L.append("      }")
    return L


def _kernel_prologue(spec, name, L, mid=None, pre=None):
    """Kernel head shared by generate / generate_tiled: operand pointers, accumulator, and the
    loop-invariant part (scalar operands, sub-expressions of them, reciprocals of invariant
    divisors).  ``pre(L)`` / ``mid(L)`` may emit code right after the operand pointers (index
    arithmetic on kernel arguments) and after the small loads of the head (the early first loads
    of a flat reduction).  Returns (hoisted, inv_in) for emit_scalar_body."""
    nin, nout = len(spec.in_dtypes), len(spec.out_dtypes)
    nops, V, red = nin + nout, spec.vec, spec.reduce
    L.append(PRELUDE)
    hj = spec.hjobs
    if hj:
        # horizontally fused form: find this workgroup's job, then build the single-job view `a`
        # the rest of the kernel is written against (flat operands: shape[0] = n, no strides)
        L.append('extern "C" __global__ __launch_bounds__(%d) void %s(ArgsH h) {' % (spec.block, name))
        L.append("  unsigned job_ = 0;")
        L.append("  for (int j = 1; j < h.njobs; ++j) if (blockIdx.x >= h.wg0[j]) job_ = j;")
        L.append("  const unsigned lb_ = blockIdx.x - h.wg0[job_], gj_ = h.wg0[job_ + 1] - h.wg0[job_];")
        L.append("  const unsigned slot0_ = h.wg0[job_];")
        L.append("  struct { i64 n; i64 shape[1]; void* ptr[AHIP_HOPS]; void* ws; void* out; i64 aux1; } a;")
        L.append("  a.n = h.n[job_]; a.shape[0] = a.n; a.ws = h.ws; a.out = h.out[job_]; a.aux1 = h.aux1;")
        L.append("  for (int k = 0; k < %d; ++k) a.ptr[k] = h.ptr[job_][k];" % nops)
    else:
        L.append('extern "C" __global__ __launch_bounds__(%d) void %s(Args a) {' % (spec.block, name))
    for k in range(nin):
        L.append("  const %s* __restrict__ p%d = (const %s*)a.ptr[%d];" %
                 (CTYPE[spec.in_dtypes[k]], k, CTYPE[spec.in_dtypes[k]], k))
    for k in range(nout):
        L.append("  %s* __restrict__ p%d = (%s*)a.ptr[%d];" %
                 (CTYPE[spec.out_dtypes[k]], nin + k, CTYPE[spec.out_dtypes[k]], nin + k))
    if any(c == "s" for c in spec.inner):
        assert V == 1
        for k in range(nops):
            if spec.inner[k] == "s":
                L.append("  const i64 is%d = a.stride[%d][%d];" % (k, k, spec.nd - 1))

    if spec.trace:
        # stamps are kept in registers until the launch epoch is known: even and odd epochs write
        # to two halves of the trace area, so the stamps of two CONSECUTIVE launches survive
        # (end of one launch -> first wavefront of the next, on one clock)
        L.append("  unsigned long long tr_s_[8] = {0, 0, 0, 0, 0, 0, 0, 0};")
        L.append("  if (threadIdx.x == 0) { tr_s_[0] = __builtin_readcyclecounter(); tr_s_[1] = wall_clock64(); "
                 "unsigned hw_; asm volatile(\"s_getreg_b32 %0, hwreg(HW_REG_HW_ID)\" : \"=s\"(hw_)); "
                 "unsigned xcc_; asm volatile(\"s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)\" : \"=s\"(xcc_)); "
                 "tr_s_[7] = ((unsigned long long)xcc_ << 32) | hw_; }")
    # every load the head of the kernel depends on is ISSUED before anything waits: the small
    # ones first (exp-table entry, scalar operands, launch epoch: they come back from the
    # memory-side cache), then — ``mid`` — the first group of a flat reduction's stream, so the
    # invariant arithmetic below runs while the stream's first bytes are in flight
    if pre is not None:
        pre(L)
    fast_exp = spec.fast_exp
    if fast_exp:
        L.append("  const double etv_ = AHIP_EXP2_64[threadIdx.x & 63];")
    hoisted = {}
    inv_in = {}
    if any(spec.invariant):
        for k in range(nin):
            if spec.invariant[k]:
                e = "xinv%d" % k
                L.append("  const %s %s = p%d[0];" % (CTYPE[spec.in_dtypes[k]], e, k))
                inv_in[k] = "(%s != 0)" % e if spec.in_dtypes[k] == "bool" else e
    if red is not None and red["kind"] == "all":
        # launch epoch of the finalize (read early: its latency hides under the streaming loop);
        # a fused launch keeps one epoch word per job (a job's collector advances it when all of
        # THAT job's workgroups have published, i.e. have read it)
        L.append("  unsigned* const epochp = (unsigned*)((char*)a.ws + a.aux1 + 2048 + %s);" %
                 ("256 + 4 * job_" if hj else "64"))
        L.append("  const unsigned ep0 = __hip_atomic_load(epochp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);")
    if mid is not None:
        mid(L)
    if fast_exp:
        # one copy of the 2^(j/64) table per wavefront: lane j writes entry j of its wave's copy
        # and the wave reads only that copy, so there is no workgroup barrier (LDS operations of
        # one wave complete in order; the asm keeps the compiler from moving reads above it)
        L.append("  __shared__ double exptbl_[%d];" % spec.block)
        L.append("  exptbl_[threadIdx.x] = etv_;")
        L.append("  asm volatile(\"s_waitcnt lgkmcnt(0)\" ::: \"memory\");")
        L.append("  const double* const etbl_ = exptbl_ + (threadIdx.x & ~63u);")
    if red is not None:
        acc_t = RTYPE[red["acc"]]
        L.append("  %s acc = %s;" % (acc_t, red_identity(red["op"], red["acc"])))

    # loop-invariant prologue: sub-expressions that depend only on scalar operands are computed
    # once per thread, and reciprocals of invariant divisors are hoisted
    if any(spec.invariant):
        inv_nodes = invariant_nodes(spec.scalar, spec.invariant)
        if inv_nodes:
            ins0 = [inv_in.get(k, "0") for k in range(nin)]
            lines, _, _ = emit_scalar_body(spec.scalar, ins0, spec.in_dtypes, indent="  ",
                                           suffix="_inv", only=inv_nodes)
            L.extend(lines)
            divisors = {n["in"][1][1] for n in spec.scalar["nodes"]
                        if n["op"] == "true_div" and n["in"][1][0] == "t"}
            for k in sorted(inv_nodes):
                dt = spec.scalar["nodes"][k]["dtype"]
                rname = None
                if k in divisors and is_float(dt):
                    rname = "r%d_inv, ok%d_inv" % (k, k)
                    L.append("  const %s r%d_inv = (%s)1 / t%d_inv;" % (RTYPE[dt], k, RTYPE[dt], k))
                    L.append("  const bool ok%d_inv = recip_ok(t%d_inv, r%d_inv);" % (k, k, k))
                hoisted[k] = ("t%d_inv" % k, rname)
    return hoisted, inv_in


def generate_tiled(spec: KernelSpec):
    """K3t — Elemwise (optionally + full reduction) with TRANSPOSED operands.

    The reference walks such operands with its strided loop nest (`elemwise_cgen.py:228-305`
    make_loop with per-operand strides); a lane-per-element GPU loop would fetch one element per
    cache line from them.  Here the last dim and `tile_dim` are cut into T x T tiles: operands of
    class 't' (unit stride along tile_dim) are read with the lanes running along tile_dim — full
    lines — into a padded LDS tile, then the scalar body runs with the lanes along the last dim,
    taking those operands from LDS (conflict-free thanks to the odd row pitch) and every other
    operand / output directly (coalesced for class 'c', broadcast for 'b').  One workgroup of 256
    threads per tile; remaining dims are decomposed from the tile index."""
    nin, nout = len(spec.in_dtypes), len(spec.out_dtypes)
    nops, nd, red = nin + nout, spec.nd, spec.reduce
    td, T = spec.tile_dim
    assert spec.vec == 1 and spec.block == 256 and T in (32, 64) and 0 <= td < nd - 1
    assert red is None or red["kind"] == "all"
    LP = 256 // T          # tile lines covered per pass
    P = T // LP            # passes
    name = "ewt_" + spec.digest()
    L = []
    hoisted, inv_in = _kernel_prologue(spec, name, L)
    tk = [k for k in range(nin) if spec.inner[k] == "t" and k not in inv_in]
    assert tk and all(spec.inner[k] != "t" for k in range(nin, nops))
    for k in tk:
        L.append("  __shared__ %s tile%d[%d][%d];" % (CTYPE[spec.in_dtypes[k]], k, T, T + 1))
    outer = [d for d in range(nd - 1) if d != td]
    L.append("  const i64 R = a.shape[%d], C = a.shape[%d];" % (td, nd - 1))
    L.append("  const i64 tr = (R + %d) / %d, tc = (C + %d) / %d;" % (T - 1, T, T - 1, T))
    L.append("  const i64 ntiles = tr * tc%s;" % "".join(" * a.shape[%d]" % d for d in outer))
    L.append("  const int ta = threadIdx.x %% %d, tb = threadIdx.x / %d;" % (T, T))
    L.append("  for (i64 tix = blockIdx.x; tix < ntiles; tix += gridDim.x) {")
    L.append("    i64 rem = tix;")
    L.append("    const i64 jc = rem % tc; rem /= tc;")
    L.append("    const i64 jr = rem % tr; rem /= tr;")
    live = [k for k in range(nops) if k not in inv_in]
    L.append("    i64 " + ", ".join("off%d = 0" % k for k in live) + ";")
    for d in reversed(outer):
        L.append("    { const i64 q = rem / a.shape[%d]; const i64 r = rem - q * a.shape[%d]; rem = q;"
                 % (d, d))
        for k in live:
            L.append("      off%d += r * a.stride[%d][%d];" % (k, k, d))
        L.append("    }")
    L.append("    const i64 r0 = jr * %d, c0 = jc * %d;" % (T, T))
    # every load of the tile is issued up front with clamped (always valid) coordinates — no
    # branches between them, so P x (operands) requests per lane are in flight at once; only the
    # compute / store / accumulate is guarded at ragged edges.
    direct = [k for k in range(nin) if k not in inv_in and k not in tk]

    def addr(k, r, c):
        inner = {"c": " + %s" % c, "b": "", "s": " + %s * a.stride[%d][%d]" % (c, k, nd - 1)}[
            spec.inner[k]]
        return "off%d + %s * a.stride[%d][%d]%s" % (k, r, k, td, inner)

    L.append("    const i64 rl = (r0 + ta < R) ? r0 + ta : R - 1;   // phase 1: lanes along tile_dim")
    L.append("    const i64 cq = (c0 + ta < C) ? c0 + ta : C - 1;   // phase 2: lanes along the last dim")
    for k in tk + direct:
        L.append("    %s v%d[%d];" % (CTYPE[spec.in_dtypes[k]], k, P))
    L.append("#pragma unroll")
    L.append("    for (int j = 0; j < %d; ++j) {" % P)
    L.append("      const i64 cl = (c0 + tb + j * %d < C) ? c0 + tb + j * %d : C - 1;" % (LP, LP))
    for k in tk:
        L.append("      v%d[j] = p%d[off%d + rl + cl * a.stride[%d][%d]];" % (k, k, k, k, nd - 1))
    L.append("    }")
    if direct:
        L.append("#pragma unroll")
        L.append("    for (int j = 0; j < %d; ++j) {" % P)
        L.append("      const i64 rq = (r0 + tb + j * %d < R) ? r0 + tb + j * %d : R - 1;" % (LP, LP))
        for k in direct:
            L.append("      v%d[j] = p%d[%s];" % (k, k, addr(k, "rq", "cq")))
        L.append("    }")
    L.append("#pragma unroll")
    L.append("    for (int j = 0; j < %d; ++j) {" % P)
    for k in tk:
        L.append("      tile%d[tb + j * %d][ta] = v%d[j];" % (k, LP, k))
    L.append("    }")
    L.append("    __syncthreads();")
    L.append("#pragma unroll")
    L.append("    for (int j = 0; j < %d; ++j) {" % P)
    L.append("      const int rr = tb + j * %d;" % LP)
    L.append("      const i64 r = r0 + rr, c = c0 + ta;")
    L.append("      if (r < R && c < C) {")
    ins = []
    for k in range(nin):
        if k in inv_in:
            ins.append(inv_in[k])
            continue
        ct = CTYPE[spec.in_dtypes[k]]
        if k in tk:
            L.append("        const %s x%d = tile%d[ta][rr];" % (ct, k, k))
        else:
            L.append("        const %s x%d = v%d[j];" % (ct, k, k))
        ins.append("(x%d != 0)" % k if spec.in_dtypes[k] == "bool" else "x%d" % k)
    lines, outs, odts = emit_scalar_body(spec.scalar, ins, spec.in_dtypes, indent="        ",
                                         suffix="_t", hoisted=hoisted)
    L.extend(lines)
    for k, ri in enumerate(spec.out_refs):
        val = store_val(outs[ri], odts[ri], spec.out_dtypes[k])
        L.append("        p%d[%s] = %s;" % (nin + k, addr(nin + k, "r", "c"), val))
    if red is not None:
        val = cast(outs[red["ref"]], odts[red["ref"]], red["acc"])
        L.append("        acc = %s;" % red_combine(red["op"], red["acc"], "acc", val))
    L.append("      }")
    L.append("    }")
    L.append("    __syncthreads();")
    L.append("  }")
    if red is not None:
        reduce_all_finalize(spec, red, L)
    L.append("}")
    return "\n".join(L) + "\n", (name,)


def _loads(spec, elem_off_exprs, sfx="", decl=True):
    """Loads of one item (``vec`` elements per lane) of every operand that is not loop invariant."""
    V = spec.vec
    B = []
    for k in range(len(spec.in_dtypes)):
        ct = CTYPE[spec.in_dtypes[k]]
        if spec.invariant[k]:
            continue
        if spec.inner[k] == "c" and V > 1:
            ptr = "(const Pack<%s, %d>*)(p%d + %s)" % (ct, V, k, elem_off_exprs[k])
            head = "const Pack<%s, %d> " % (ct, V) if decl else ""
            B.append("      %sx%d%s = %s;" % (head, k, sfx, "nt_load(%s)" % ptr if int(spec.nt) & 1 else "*" + ptr))
        else:
            B.append("      %sx%d%s = p%d[%s];" % ("const %s " % ct if decl else "", k, sfx, k,
                                                 elem_off_exprs[k]))
    return B


def _compute(spec, head, elem_off_exprs, sfx="", accs=None):
    """The scalar body of one item, its stores and its accumulation.  ``head``: what
    ``_kernel_prologue`` returned."""
    hoisted, inv_in = head
    V, nin, nout, red = spec.vec, len(spec.in_dtypes), len(spec.out_dtypes), spec.reduce
    sum_only = sum_only_nodes(spec.scalar, red, spec.out_refs)
    B = []
    accs = accs or ["acc"] * V
    for k in range(nout):
        if V > 1:
            B.append("      Pack<%s, %d> y%d%s;" % (CTYPE[spec.out_dtypes[k]], V, k, sfx))
    for v in range(V):
        ins = []
        for k in range(nin):
            if k in inv_in:
                ins.append(inv_in[k])
                continue
            e = "x%d%s.v[%d]" % (k, sfx, v) if spec.inner[k] == "c" and V > 1 else "x%d%s" % (k, sfx)
            if spec.in_dtypes[k] == "bool":
                e = "(%s != 0)" % e
            ins.append(e)
        lines, outs, odts = emit_scalar_body(spec.scalar, ins, spec.in_dtypes,
                                             suffix="_%d%s" % (v, sfx), hoisted=hoisted,
                                             exp_tbl="etbl_" if spec.fast_exp else None,
                                             sum_only=sum_only)
        B.extend(lines)
        for k, ri in enumerate(spec.out_refs):
            val = store_val(outs[ri], odts[ri], spec.out_dtypes[k])
            if V > 1:
                B.append("      y%d%s.v[%d] = %s;" % (k, sfx, v, val))
            else:
                B.append("      p%d[%s] = %s;" % (nin + k, elem_off_exprs[nin + k], val))
        if red is not None:
            val = cast(outs[red["ref"]], odts[red["ref"]], red["acc"])
            B.append("      %s = %s;" % (accs[v], red_combine(red["op"], red["acc"], accs[v], val)))
    if V > 1:
        for k in range(nout):
            dst = "(Pack<%s, %d>*)(p%d + %s)" % (CTYPE[spec.out_dtypes[k]], V, nin + k, elem_off_exprs[nin + k])
            B.append(("      nt_store(%s, y%d%s);" if int(spec.nt) & 2 else "      *%s = y%d%s;") % (dst, k, sfx))
    return B


def generate(spec: KernelSpec):
    """Return (source, kernel_names) for a spec (one kernel per spec)."""
    if spec.tile_dim is not None:
        return generate_tiled(spec)
    red = spec.reduce
    if red is None or red["kind"] == "all":
        return _generate_stream(spec)
    return (_generate_row_reduce if red["kind"] == "row" else _generate_col_reduce)(spec)


def _generate_stream(spec: KernelSpec):
    """K1 / K3 — Elemwise over the items of a flat or n-d space (vectors of V elements of the
    innermost dim), optionally with a full reduction of one of its values (in-kernel finalize)."""
    nin, nops = len(spec.in_dtypes), len(spec.in_dtypes) + len(spec.out_dtypes)
    V, U, nd, red = spec.vec, spec.unroll, spec.nd, spec.reduce
    idx_t = "i64" if spec.idx64 else "int"
    name = "ew_" + spec.digest()
    L = []
    flat_u = nd == 1 and U > 1
    early = spec.early and flat_u

    def index_setup(L_):
        # the walk over the items (vectors of V elements): grid-stride, or (blocked) one
        # contiguous chunk per workgroup, a whole number of vectors per thread
        L_.append("  const %s inner_vecs = (%s)(a.shape[%d] / %d);" % (idx_t, idx_t, nd - 1, V))
        if spec.blocked:
            L_.append("  const %s items_all = (%s)(a.n / %d);" % (idx_t, idx_t, V))
            grd = "gj_" if spec.hjobs else "gridDim.x"
            L_.append("  const %s chunk_ = ((items_all + (%s)%s - 1) / (%s)%s + %d) / %d * %d;" %
                      (idx_t, idx_t, grd, idx_t, grd, spec.block - 1, spec.block, spec.block))
            if spec.blocked == 2:
                # workgroup b runs on XCD b % 8 (observed dispatch order, a speed hint only): give
                # every XCD one contiguous eighth of the stream, so an XCD's L2 / TLB sees 1/8 of
                # the pages instead of all of them
                L_.append("  const unsigned vb_ = (gridDim.x % 8u == 0u) ? (blockIdx.x % 8u) * (gridDim.x / 8u) + "
                          "blockIdx.x / 8u : blockIdx.x;")
            else:
                L_.append("  const unsigned vb_ = %s;" % ("lb_" if spec.hjobs else "blockIdx.x"))
            L_.append("  const %s beg_ = (%s)vb_ * chunk_;" % (idx_t, idx_t))
            L_.append("  const %s items = beg_ + chunk_ < items_all ? beg_ + chunk_ : items_all;" % idx_t)
            L_.append("  const %s step = %d;" % (idx_t, spec.block))
            L_.append("  %s item = beg_ + threadIdx.x;" % idx_t)
        else:
            L_.append("  const %s items = (%s)(a.n / %d);" % (idx_t, idx_t, V))
            L_.append("  const %s step = (%s)gridDim.x * %d;" % (idx_t, idx_t, spec.block))
            L_.append("  %s item = (%s)blockIdx.x * %d + threadIdx.x;" % (idx_t, idx_t, spec.block))

    flat = [{"c": "(i64)%%s * %d" % V, "b": "0", "s": "(i64)%%s * is%d" % k}[spec.inner[k]]
            for k in range(nops)]

    def flat_offsets(it):
        return [f % it if "%s" in f else f for f in flat]

    def early_loads(L_):
        # the first group of U vectors per lane, issued straight after the kernel arguments: the
        # invariant prologue below (dependent scalar loads of mu / sigma, a full-precision
        # reciprocal, the exp table) then runs while they are in flight
        for u in range(U):
            for k in range(nin):
                if spec.invariant[k]:
                    continue
                ct = CTYPE[spec.in_dtypes[k]]
                L_.append("  %s x%d_e%d;" % ("Pack<%s, %d>" % (ct, V) if spec.inner[k] == "c" and V > 1
                                              else ct, k, u))
        # issued unconditionally, at clamped positions (no branch: the compiler then knows how
        # many loads are outstanding and waits for the exp table / scalars only); an empty
        # operand is re-pointed at the workspace by the launcher, so position 0 is always readable
        L_.append("  const bool first_ = item + %d * step < items;" % (U - 1))
        L_.append("  const %s last_ = items > 0 ? items - 1 : 0;" % idx_t)
        for u in range(U):
            L_.append("  const %s ie%d_ = item + %d * step < last_ ? item + %d * step : last_;" %
                      (idx_t, u, u, u))
            L_.extend(_loads(spec, flat_offsets("ie%d_" % u), "_e%d" % u, decl=False))

    head = _kernel_prologue(spec, name, L, mid=early_loads if early else None,
                            pre=index_setup if early else None)
    tstamp = (lambda k: L.append("  if (threadIdx.x == 0) tr_s_[%d] = wall_clock64();" % k)) \
        if spec.trace else (lambda k: None)
    if not early:
        index_setup(L)
    if flat_u:
        # flat streaming shape: U independent vectors in flight per lane, loads first
        if early:
            L.append("  if (first_) {")
            for u in range(U):
                L.extend(_compute(spec, head, flat_offsets("(item + %d * step)" % u), "_e%d" % u))
            L.append("    item += %d * step;" % U)
            L.append("  }")
            tstamp(2)
        L.append("  for (; item + %d * step < items; item += %d * step) {" % (U - 1, U))
        for u in range(U):
            L.extend(_loads(spec, flat_offsets("(item + %d * step)" % u), "_u%d" % u))
        for u in range(U):
            L.extend(_compute(spec, head, flat_offsets("(item + %d * step)" % u), "_u%d" % u))
        L.append("  }")
    L.append("  for (; item < items; item += step) {")
    L.append("      i64 " + ", ".join("off%d = 0" % k for k in range(nops)) + ";")
    L.append("      %s inner = 0;" % idx_t)
    L.extend(_offset_code(spec, nops, 0, nd, "item", idx_t, inner_vecs="inner_vecs"))
    eo = [{"c": "off%d + (i64)inner * %d" % (k, V), "b": "off%d" % k,
           "s": "off%d + (i64)inner * is%d" % (k, k)}[spec.inner[k]] for k in range(nops)]
    L.extend(_loads(spec, eo))
    L.extend(_compute(spec, head, eo))
    L.append("  }")
    tstamp(3)
    if red is not None:
        reduce_all_finalize(spec, red, L)
    L.append("}")
    return "\n".join(L) + "\n", (name,)


# K2 axis reductions.  Dims are [kept (nk) | reduced (nr)]; `lanes` threads cooperate:
#   row: the unit stride is in the reduced group.  `lanes` (<= 64, power of two) adjacent
#        lanes share one output, each taking vectors of V elements of the flattened
#        reduced index; gridDim.y slices long reductions (partials + fold pass).
#   col: the unit stride is in the kept group.  A workgroup is TX x TY threads: TX =
#        `lanes` along the kept index (V adjacent outputs per thread), TY rows of the
#        reduced index walked concurrently; folded with shuffles, then across the waves
#        through LDS, in a fixed order.
def _generate_row_reduce(spec: KernelSpec):
    nops = len(spec.in_dtypes) + len(spec.out_dtypes)
    V, U, red = spec.vec, spec.unroll, spec.reduce
    idx_t = "i64" if spec.idx64 else "int"
    name = "ew_" + spec.digest()
    L = []
    head = _kernel_prologue(spec, name, L)
    nk, nr = red["nk"], red["nr"]
    G = red.get("lanes", 64)
    acc_t = RTYPE[red["acc"]]
    vec_cls = {"c": " + (i64)inner * %d" % V, "b": "", "s": ""}
    assert G <= 64 and 64 % G == 0
    L.append("  const int gl = threadIdx.x %% %d;" % G)
    # a workgroup walks the outputs with a grid stride (the launcher caps the grid at a
    # few workgroups per CU): millions of short rows as one output per thread group would
    # be bound by the rate at which wavefronts are DISPATCHED (max over 4 194 304 rows of
    # 8: 32 768 workgroups of one 16-byte load per thread, 32 us = 0.52 of the HBM peak)
    if red.get("short"):
        # every output's reduced run is at most one vector per lane (rows of 8 ... 256
        # elements): the inner loop below runs at most once, so the compiler may keep the
        # loads of several outputs in flight
        L.append("#pragma unroll 4")
    L.append("  for (i64 ob = (i64)blockIdx.x * %d; ob < a.n; ob += (i64)gridDim.x * %d) {" %
             (spec.block // G, spec.block // G))
    L.append("  const i64 o = ob + threadIdx.x / %d;" % G)
    L.append("  const bool valid = o < a.n;")
    L.append("  acc = %s;" % red_identity(red["op"], red["acc"]))
    L.append("  i64 " + ", ".join("base%d = 0" % k for k in range(nops)) + ";")
    L.append("  if (valid) {")
    L.append("      i64 " + ", ".join("off%d = 0" % k for k in range(nops)) + ";")
    L.extend(_offset_code(spec, nops, 0, nk, "o", idx_t))
    L.append("      " + " ".join("base%d = off%d;" % (k, k) for k in range(nops)))
    L.append("  }")
    L.append("  const %s inner_vecs = (%s)(a.shape[%d] / %d);" % (idx_t, idx_t, nk + nr - 1, V))
    L.append("  const i64 nredv = a.aux0 / %d;" % V)
    L.append("  const i64 per = (nredv + a.aux1 - 1) / a.aux1;")
    L.append("  const i64 rbeg = (i64)blockIdx.y * per;")
    L.append("  const i64 rend = !valid ? 0 : ((rbeg + per < nredv) ? rbeg + per : nredv);")
    # consecutive iterations are independent: unrolling keeps several loads in flight
    if red.get("short"):
        L.append("  if (rbeg + gl < rend) { const i64 r0 = rbeg + gl;")
    else:
        L.append("#pragma unroll %d" % (U if U > 1 else 8))
        L.append("  for (i64 r0 = rbeg + gl; r0 < rend; r0 += %d) {" % G)
    L.append("      i64 " + ", ".join("off%d = base%d" % (k, k) for k in range(nops)) + ";")
    L.append("      %s inner = 0;" % idx_t)
    if V > 1:
        L.extend(_offset_code(spec, nops, nk, nk + nr, "(%s)r0" % idx_t, idx_t,
                              inner_vecs="inner_vecs"))
        eo = ["off%d%s" % (k, vec_cls[spec.inner[k]]) for k in range(nops)]
    else:
        L.extend(_offset_code(spec, nops, nk, nk + nr, "(%s)r0" % idx_t, idx_t))
        eo = ["off%d" % k for k in range(nops)]
    L.extend(_loads(spec, eo))
    L.extend(_compute(spec, head, eo))
    L.append("  }")
    L.append("  for (int m = %d; m > 0; m >>= 1) acc = %s;" %
             (G // 2, red_combine(red["op"], red["acc"], "acc", "shfl_xor_<%s>(acc, m)" % acc_t)))
    L.append("  if (valid && gl == 0) {")
    L.append("    if (a.aux1 == 1) ((%s*)a.out)[o] = %s;" %
             (CTYPE[red["out"]], store_val("acc", red["acc"], red["out"])))
    L.append("    else ((%s*)a.out)[(i64)blockIdx.y * a.n + o] = acc;" % CTYPE[red["acc"]])
    L.append("  }")
    L.append("  }")      # (grid-stride walk over the outputs)
    L.append("}")
    return "\n".join(L) + "\n", (name,)


def _generate_col_reduce(spec: KernelSpec):
    nops = len(spec.in_dtypes) + len(spec.out_dtypes)
    V, U, red = spec.vec, spec.unroll, spec.reduce
    idx_t = "i64" if spec.idx64 else "int"
    name = "ew_" + spec.digest()
    L = []
    head = _kernel_prologue(spec, name, L)
    nk, nr = red["nk"], red["nr"]
    TX = red.get("lanes", spec.block)
    acc_t = RTYPE[red["acc"]]
    comb = lambda a_, b_: red_combine(red["op"], red["acc"], a_, b_)  # noqa: E731
    vec_cls = {"c": " + (i64)inner * %d" % V, "b": "", "s": ""}
    assert (TX <= 64 and 64 % TX == 0 or TX % 64 == 0) and spec.block % TX == 0
    TY = spec.block // TX
    # rows of the LDS fold: the waves (TX <= 64: a wave holds 64 / TX reduced rows, folded
    # by shuffles first) or the TY thread rows (TX > 64: every wave is part of one row)
    nw = spec.block // 64 if TX <= 64 else TY
    accs = ["acc"] + ["acc_%d" % v for v in range(1, V)]
    for nm in accs[1:]:
        L.append("  %s %s = %s;" % (acc_t, nm, red_identity(red["op"], red["acc"])))
    L.append("  const int tx = threadIdx.x %% %d, ty = threadIdx.x / %d;" % (TX, TX))
    L.append("  const i64 nkeptv = a.n / %d;" % V)
    L.append("  const i64 ov = (i64)blockIdx.x * %d + tx;" % TX)
    L.append("  const bool valid = ov < nkeptv;")
    L.append("  i64 " + ", ".join("base%d = 0" % k for k in range(nops)) + ";")
    L.append("  if (valid) {")
    L.append("      i64 " + ", ".join("off%d = 0" % k for k in range(nops)) + ";")
    if V > 1:
        L.append("      const %s inner_vecs = (%s)(a.shape[%d] / %d);" % (idx_t, idx_t, nk - 1, V))
        L.append("      %s inner = 0;" % idx_t)
        L.extend(_offset_code(spec, nops, 0, nk, "(%s)ov" % idx_t, idx_t,
                              inner_vecs="inner_vecs"))
        L.append("      " + " ".join("base%d = off%d%s;" % (k, k, vec_cls[spec.inner[k]])
                                     for k in range(nops)))
    else:
        L.extend(_offset_code(spec, nops, 0, nk, "(%s)ov" % idx_t, idx_t))
        L.append("      " + " ".join("base%d = off%d;" % (k, k) for k in range(nops)))
    L.append("  }")
    L.append("  const i64 nred = a.aux0;")
    L.append("  const i64 per = (nred + a.aux1 - 1) / a.aux1;")
    L.append("  const i64 rbeg = (i64)blockIdx.y * per;")
    L.append("  const i64 rend = !valid ? 0 : ((rbeg + per < nred) ? rbeg + per : nred);")
    L.append("#pragma unroll %d" % (U if U > 1 else 8))
    L.append("  for (i64 r0 = rbeg + ty; r0 < rend; r0 += %d) {" % TY)
    L.append("      i64 " + ", ".join("off%d = base%d" % (k, k) for k in range(nops)) + ";")
    L.extend(_offset_code(spec, nops, nk, nk + nr, "(%s)r0" % idx_t, idx_t))
    eo = ["off%d" % k for k in range(nops)]
    L.extend(_loads(spec, eo))
    L.extend(_compute(spec, head, eo, accs=accs))
    L.append("  }")
    # fold over ty: lanes of a wave that share tx (xor masks >= TX), then the waves in order
    sm_t = acc_t if acc_t != "bool" else "unsigned char"
    if TX < 64:
        for nm in accs:
            L.append("  for (int m = 32; m >= %d; m >>= 1) %s = %s;" %
                     (TX, nm, comb(nm, "shfl_xor_<%s>(%s, m)" % (acc_t, nm))))
    if nw > 1:
        L.append("  __shared__ %s sm[%d][%d];" % (sm_t, nw, TX * V))
        if TX <= 64:
            L.append("  if ((threadIdx.x & 63) < %d) {" % TX)
            row = "threadIdx.x >> 6"
        else:
            L.append("  {")
            row = "ty"
        for v, nm in enumerate(accs):
            L.append("    sm[%s][tx * %d + %d] = %s;" % (row, V, v, nm))
        L.append("  }")
        L.append("  __syncthreads();")
    L.append("  if (valid && threadIdx.x < %d) {" % TX)
    for v, nm in enumerate(accs):
        if nw > 1:
            L.append("    %s r%d = sm[0][tx * %d + %d];" % (acc_t, v, V, v))
            L.append("    for (int w = 1; w < %d; ++w) r%d = %s;" %
                     (nw, v, comb("r%d" % v, "(%s)sm[w][tx * %d + %d]" % (acc_t, V, v))))
        else:
            L.append("    %s r%d = %s;" % (acc_t, v, nm))
        L.append("    if (a.aux1 == 1) ((%s*)a.out)[ov * %d + %d] = %s;" %
                 (CTYPE[red["out"]], V, v, store_val("r%d" % v, red["acc"], red["out"])))
        L.append("    else ((%s*)a.out)[(i64)blockIdx.y * a.n + ov * %d + %d] = r%d;" %
                 (CTYPE[red["acc"]], V, v, v))
    L.append("  }")
    L.append("}")
    return "\n".join(L) + "\n", (name,)
