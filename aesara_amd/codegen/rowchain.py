"""Row chains: last-axis reductions and the Elemwise steps between them in one pass, with the row
in a wavefront's registers (``rc_`` kernels) or one workgroup per long row (``rcl_``)."""
from __future__ import annotations

from .prelude import CTYPE, PRELUDE, RTYPE
from .scalar import cast, emit_scalar_body, fname, red_combine, red_identity, store_val
from .spec import Spec

RC_MAXOPS = 16

RC_MAXLEAD = 4

RC_STRUCT = r"""
#define RC_MAXOPS %d
#define RC_MAXLEAD %d
struct RcArgs { i64 N; i64 K; i64 lshape[RC_MAXLEAD]; void* ptr[RC_MAXOPS]; i64 ls[RC_MAXOPS][RC_MAXLEAD]; };
""" % (RC_MAXOPS, RC_MAXLEAD)


class RowChainSpec(Spec):
    """Rows of an [N, K] space (K = the last, contiguous axis) processed by sub-wave groups of
    ``L`` lanes (L a power of two <= 64, 64 / L rows per wavefront); a lane keeps ``nch`` packs
    of ``V`` consecutive elements of every full operand in registers, so each operand is read
    from HBM exactly once and every intermediate between the reductions stays in registers.

    Replaces the separate passes the reference makes for such chains — e.g. Softmax.c_code
    (tensor/special.py:372-415: max pass, exp+sum pass, scale pass over the output) or the
    CAReduce / DimShuffle / Elemwise node sequence a hand-written normalisation lowers to
    (tensor/elemwise.py:1495, :222, :725).

    ext      : [(dtype, cls)] external operands; cls "f" full [N, K], "r" per-row [N, 1],
               "c" per-column [1, K], "s" scalar
    members  : the chain in execution order; each {"scalar", "ins", "reduce", "stores"} with
               ins[i] = ["e", k] | ["f", member, scalar-out index] | ["r", member];
               reduce = None | {"op", "acc", "out", "ref", "slot"}; stores = [[out index, dtype,
               slot]] (slots index RcArgs.ptr after the external operands)
    long_rows: rows that do not fit a wavefront's registers, one workgroup per row
               (generate_rowchain_long); selects the generator and the cache entry, not the digest
    """

    def __init__(self, ext, members, L, V, nch, lnd=1, block=256, nt=False, long_rows=False):
        self.long_rows = bool(long_rows)
        self.ext = [list(e) for e in ext]
        self.members, self.L, self.V, self.nch, self.block = members, L, V, nch, block
        self.lnd = lnd          # jointly-collapsed leading dims (row index -> coordinates)
        self.nt = bool(nt)      # streaming (non-temporal) loads of the full operands: read-once rows
        assert L in (1, 2, 4, 8, 16, 32, 64) and block % 64 == 0 and 1 <= lnd <= RC_MAXLEAD

    def source_fields(self):
        return ["rc2" + ("n" if self.nt else ""), self.ext, self.members, self.L, self.V, self.nch,
                self.lnd, self.block]

    def key(self):
        # the two forms of one chain share their digest (the kernel names differ: rc_ / rcl_)
        return ("long-" if self.long_rows else "") + self.digest()

    def generate(self):
        return (generate_rowchain_long if self.long_rows else generate_rowchain)(self)


def generate_rowchain(spec: RowChainSpec):
    L_, V, NCH = spec.L, spec.V, spec.nch
    rpw = 64 // L_
    waves = spec.block // 64
    name = "rc_" + spec.digest()
    S = [PRELUDE, RC_STRUCT]
    S.append('extern "C" __global__ __launch_bounds__(%d) void %s(RcArgs a) {' % (spec.block, name))
    S.append("  const int lane = threadIdx.x & 63;")
    S.append("  const int sub = lane & %d;" % (L_ - 1))
    S.append("  const int grp = lane >> %d;" % (L_.bit_length() - 1))
    S.append("  const i64 nwaves = (i64)gridDim.x * %d;" % waves)
    for c in range(NCH):
        S.append("  const i64 col%d = ((i64)%d + sub) * %d;" % (c, c * L_, V))
        S.append("  const bool ok%d = col%d < a.K;" % (c, c))
    for k, (dt, cls) in enumerate(spec.ext):
        ct = CTYPE[dt]
        if cls == "s":
            S.append("  const %s sc%d = *(const %s*)a.ptr[%d];" % (ct, k, ct, k))
        elif cls == "c":
            for c in range(NCH):
                S.append("  Pack<%s, %d> co%d_%d = {}; if (ok%d) co%d_%d = *(const Pack<%s, %d>*)"
                         "((const %s*)a.ptr[%d] + col%d);" % (ct, V, k, c, c, k, c, ct, V, ct, k, c))
    S.append("  for (i64 rb = ((i64)blockIdx.x * %d + (threadIdx.x >> 6)) * %d; rb < a.N; "
             "rb += nwaves * %d) {" % (waves, rpw, rpw))
    S.append("    const i64 row = rb + grp;")
    S.append("    const bool rv = row < a.N;")
    S.append("    const i64 rr = rv ? row : a.N - 1;")
    # row index -> coordinates over the collapsed leading dims (one div/mod per extra dim)
    rem = "rr"
    for d in range(spec.lnd - 1, 0, -1):
        S.append("    const i64 q%d = %s / a.lshape[%d];" % (d, rem, d))
        S.append("    const i64 lc%d = %s - q%d * a.lshape[%d];" % (d, rem, d, d))
        rem = "q%d" % d
    S.append("    const i64 lc0 = %s;" % rem)

    def row_off(k):
        return " + ".join("lc%d * a.ls[%d][%d]" % (d, k, d) for d in range(spec.lnd))
    for k, (dt, cls) in enumerate(spec.ext):
        ct = CTYPE[dt]
        if cls == "f":
            S.append("    const %s* __restrict__ xp%d = (const %s*)a.ptr[%d] + %s;"
                     % (ct, k, ct, k, row_off(k)))
            for c in range(NCH):
                S.append("    Pack<%s, %d> x%d_%d = {}; if (ok%d) x%d_%d = %s((const Pack<%s, %d>*)"
                         "(xp%d + col%d));" % (ct, V, k, c, c, k, c, "nt_load" if spec.nt else "*", ct, V, k, c))
        elif cls == "r":
            S.append("    const %s ro%d = ((const %s*)a.ptr[%d])[%s];" % (ct, k, ct, k, row_off(k)))

    def ext_expr(k, c, j):
        dt, cls = spec.ext[k]
        e = {"f": "x%d_%d.v[%d]" % (k, c, j), "r": "ro%d" % k, "c": "co%d_%d.v[%d]" % (k, c, j),
             "s": "sc%d" % k}[cls]
        return ("(%s != 0)" % e if dt == "bool" else e), dt

    outs = []      # per member: {(c, j): ([expr], [dtype])}
    rdt = {}       # member -> dtype of its row result
    for mi, m in enumerate(spec.members):
        red = m.get("reduce")
        if red:
            S.append("    %s acc%d = %s;" % (RTYPE[red["acc"]], mi, red_identity(red["op"], red["acc"])))
        mouts = {}

        def inputs_at(c, j):
            in_exprs, in_dts = [], []
            for r in m["ins"]:
                if r[0] == "e":
                    e, d = ext_expr(r[1], c, j)
                elif r[0] == "f":
                    es, ds = outs[r[1]][(c, j)]
                    e, d = es[r[2]], ds[r[2]]
                else:
                    e, d = "r%d" % r[1], rdt[r[1]]
                in_exprs.append(e)
                in_dts.append(d)
            return in_exprs, in_dts

        if m.get("rowlike"):
            # every input is per-row or scalar: one evaluation per row ([..., 1]-shaped values)
            in_exprs, in_dts = inputs_at(0, 0)
            lines, oe, od = emit_scalar_body(m["scalar"], in_exprs, in_dts, indent="    ",
                                             suffix="_m%d_r" % mi)
            S.extend(lines)
            for c in range(NCH):
                for j in range(V):
                    mouts[(c, j)] = (oe, od)
            outs.append(mouts)
            for oref, odt, slot in m.get("stores", []):
                S.append("    if (rv && sub == 0) ((%s*)a.ptr[%d])[%s] = %s;"
                         % (CTYPE[odt], slot, row_off(slot), store_val(oe[oref], od[oref], odt)))
            continue
        for c in range(NCH):
            for j in range(V):
                in_exprs, in_dts = inputs_at(c, j)
                lines, oe, od = emit_scalar_body(m["scalar"], in_exprs, in_dts, indent="    ",
                                                 suffix="_m%d_%d_%d" % (mi, c, j))
                S.extend(lines)
                mouts[(c, j)] = (oe, od)
                if red:
                    v = cast(oe[red["ref"]], od[red["ref"]], red["acc"])
                    S.append("    if (ok%d) acc%d = %s;" % (c, mi, red_combine(red["op"], red["acc"],
                                                                               "acc%d" % mi, v)))
        outs.append(mouts)
        if red:
            at_ = RTYPE[red["acc"]]
            msk = L_ // 2
            while msk >= 1:
                S.append("    acc%d = %s;" % (mi, red_combine(
                    red["op"], red["acc"], "acc%d" % mi, "shfl_xor_<%s>(acc%d, %d)" % (at_, mi, msk))))
                msk //= 2
            S.append("    const %s r%d = %s;" % (RTYPE[red["out"]], mi,
                                                  cast("acc%d" % mi, red["acc"], red["out"])))
            rdt[mi] = red["out"]
            if red.get("slot") is not None:
                S.append("    if (rv && sub == 0) ((%s*)a.ptr[%d])[%s] = %s;"
                         % (CTYPE[red["out"]], red["slot"], row_off(red["slot"]),
                            store_val("r%d" % mi, red["out"], red["out"])))
        for oref, odt, slot in m.get("stores", []):
            ct = CTYPE[odt]
            for c in range(NCH):
                S.append("    if (rv && ok%d) {" % c)
                S.append("      Pack<%s, %d> y;" % (ct, V))
                for j in range(V):
                    oe, od = mouts[(c, j)]
                    S.append("      y.v[%d] = %s;" % (j, store_val(oe[oref], od[oref], odt)))
                S.append("      *(Pack<%s, %d>*)((%s*)a.ptr[%d] + %s + col%d) = y;"
                         % (ct, V, ct, slot, row_off(slot), c))
                S.append("    }")
    S.append("  }")
    S.append("}")
    return "\n".join(S) + "\n", (name,)


def generate_rowchain_long(spec: RowChainSpec):
    """Row chains whose rows do not fit a wavefront's registers (K of tens of thousands: a
    vocabulary-sized softmax): ONE WORKGROUP PER ROW.  Every reduction of the chain is a stage
    that sweeps the row in 16-byte packs (block reduce through LDS, result broadcast to all
    threads); Elemwise members between the reductions are RE-EVALUATED in each later stage that
    needs them instead of being kept (exp(x - max) is computed in the sum stage and again in the
    scale stage).  The first sweep streams the row from HBM, the later sweeps re-read it from the
    L2 / memory-side cache (a row is a few hundred KB), so HBM traffic stays ~1 read + the stores.
    Same spec / argument block as generate_rowchain (spec.L and spec.nch are ignored)."""
    V = spec.V
    T_BLOCK = spec.block
    nw = T_BLOCK // 64
    members = spec.members
    name = "rcl_" + spec.digest()
    S = [PRELUDE, RC_STRUCT]
    S.append('extern "C" __global__ __launch_bounds__(%d) void %s(RcArgs a) {' % (T_BLOCK, name))
    S.append("  __shared__ double red_sm[%d];" % nw)
    S.append("  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;")
    for k, (dt, cls) in enumerate(spec.ext):
        if cls == "s":
            S.append("  const %s sc%d = *(const %s*)a.ptr[%d];" % (CTYPE[dt], k, CTYPE[dt], k))
    S.append("  for (i64 row = blockIdx.x; row < a.N; row += gridDim.x) {")
    rem = "row"
    for d in range(spec.lnd - 1, 0, -1):
        S.append("    const i64 q%d = %s / a.lshape[%d];" % (d, rem, d))
        S.append("    const i64 lc%d = %s - q%d * a.lshape[%d];" % (d, rem, d, d))
        rem = "q%d" % d
    S.append("    const i64 lc0 = %s;" % rem)

    def row_off(k):
        return " + ".join("lc%d * a.ls[%d][%d]" % (d, k, d) for d in range(spec.lnd))

    for k, (dt, cls) in enumerate(spec.ext):
        ct = CTYPE[dt]
        if cls == "f":
            S.append("    const %s* __restrict__ xp%d = (const %s*)a.ptr[%d] + %s;" % (ct, k, ct, k, row_off(k)))
        elif cls == "c":
            S.append("    const %s* __restrict__ xp%d = (const %s*)a.ptr[%d];" % (ct, k, ct, k))
        elif cls == "r":
            S.append("    const %s ro%d = ((const %s*)a.ptr[%d])[%s];" % (ct, k, ct, k, row_off(k)))

    rowlike = [bool(m.get("rowlike")) for m in members]
    rdt = {}

    def closure(targets):
        """per-element members needed (in order) to evaluate `targets`"""
        need = set()

        def visit(mi):
            if mi in need or rowlike[mi]:
                return
            need.add(mi)
            for r in members[mi]["ins"]:
                if r[0] == "f":
                    visit(r[1])
        for t in targets:
            visit(t)
        return sorted(need)

    row_vals = {}     # rowlike member -> (out exprs, out dtypes), evaluated once per row

    def emit_rowlike_ready(upto_reduce_done):
        """evaluate row-like members whose inputs are all available now"""
        for mi, m in enumerate(members):
            if not rowlike[mi] or mi in row_vals:
                continue
            ok = all((r[0] == "e") or (r[0] == "r" and r[1] in rdt)
                     or (r[0] == "f" and r[1] in row_vals) for r in m["ins"])
            if not ok:
                continue
            ins, dts = [], []
            for r in m["ins"]:
                if r[0] == "e":
                    dt, cls = spec.ext[r[1]]
                    e = "ro%d" % r[1] if cls == "r" else "sc%d" % r[1]
                    ins.append("(%s != 0)" % e if dt == "bool" else e)
                    dts.append(dt)
                elif r[0] == "r":
                    ins.append("r%d" % r[1])
                    dts.append(rdt[r[1]])
                else:
                    es, ds = row_vals[r[1]]
                    ins.append(es[r[2]])
                    dts.append(ds[r[2]])
            lines, oe, od = emit_scalar_body(m["scalar"], ins, dts, indent="    ", suffix="_m%d_r" % mi)
            S.extend(lines)
            row_vals[mi] = (oe, od)
            for oref, odt, slot in m.get("stores", []):
                S.append("    if (threadIdx.x == 0) ((%s*)a.ptr[%d])[%s] = %s;"
                         % (CTYPE[odt], slot, row_off(slot), store_val(oe[oref], od[oref], odt)))

    def emit_sweep(stage_id, needed, body_tail):
        """one pass over the row: loads, per-element evaluation of `needed`, then body_tail(outs)"""
        used_ext = sorted({r[1] for mi in needed for r in members[mi]["ins"] if r[0] == "e"
                           and spec.ext[r[1]][1] in "fc"})
        S.append("    for (i64 c0 = (i64)threadIdx.x * %d; c0 < a.K; c0 += %d) {" % (V, T_BLOCK * V))
        for k in used_ext:
            ct = CTYPE[spec.ext[k][0]]
            S.append("      const Pack<%s, %d> x%d = *(const Pack<%s, %d>*)(xp%d + c0);" % (ct, V, k, ct, V, k))
        for j in range(V):
            outs = {}
            for mi in needed:
                m = members[mi]
                ins, dts = [], []
                for r in m["ins"]:
                    if r[0] == "e":
                        dt, cls = spec.ext[r[1]]
                        e = {"f": "x%d.v[%d]" % (r[1], j), "c": "x%d.v[%d]" % (r[1], j),
                             "r": "ro%d" % r[1], "s": "sc%d" % r[1]}[cls]
                        ins.append("(%s != 0)" % e if dt == "bool" else e)
                        dts.append(dt)
                    elif r[0] == "r":
                        ins.append("r%d" % r[1])
                        dts.append(rdt[r[1]])
                    elif rowlike[r[1]]:
                        es, ds = row_vals[r[1]]
                        ins.append(es[r[2]])
                        dts.append(ds[r[2]])
                    else:
                        es, ds = outs[r[1]]
                        ins.append(es[r[2]])
                        dts.append(ds[r[2]])
                lines, oe, od = emit_scalar_body(m["scalar"], ins, dts, indent="      ",
                                                 suffix="_s%d_m%d_%d" % (stage_id, mi, j))
                S.extend(lines)
                outs[mi] = (oe, od)
            body_tail(j, outs)
        S.append("    }")

    def online_pair(mi):
        """max over a full operand immediately followed by sum(exp(x - max)) over the same
        operand (the head of every softmax / log-softmax): both come out of ONE sweep with the
        running-maximum rescaling  s <- s * exp(m_old - m_new) + sum exp(x - m_new)."""
        a_ = members[mi]
        if not (a_.get("reduce") and a_["reduce"]["op"] == "maximum" and not a_["scalar"]["nodes"]
                and a_["ins"] and a_["ins"][0][0] == "e" and spec.ext[a_["ins"][0][1]][1] == "f"
                and a_["scalar"]["out"][a_["reduce"]["ref"]] == ["i", 0]
                and spec.ext[a_["ins"][0][1]][0] in ("float32", "float64")):
            return None
        for bj in range(mi + 1, len(members)):
            b_ = members[bj]
            if rowlike[bj]:
                continue
            if not b_.get("reduce"):
                return None
            nodes = b_["scalar"]["nodes"]
            if (b_["reduce"]["op"] == "add" and len(nodes) == 2 and nodes[0]["op"] == "sub"
                    and nodes[1]["op"] == "exp" and nodes[1]["in"] == [["t", 0]]
                    and b_["scalar"]["out"][b_["reduce"]["ref"]] == ["t", 1]
                    and len(b_["ins"]) == 2 and b_["ins"][nodes[0]["in"][0][1]] == a_["ins"][0]
                    and b_["ins"][nodes[0]["in"][1][1]] == ["r", mi]
                    and nodes[0]["in"][0][0] == "i" and nodes[0]["in"][1][0] == "i"
                    and nodes[0]["dtype"] == nodes[1]["dtype"] == spec.ext[a_["ins"][0][1]][0]
                    and b_["reduce"]["acc"] in ("float32", "float64")):
                return bj
            return None
        return None

    stage = 0
    fused_done = set()
    for mi, m in enumerate(members):
        red = m.get("reduce")
        if not red or rowlike[mi] or mi in fused_done:
            continue
        emit_rowlike_ready(True)
        bj = online_pair(mi)
        if bj is not None:
            k = m["ins"][0][1]
            xt = CTYPE[spec.ext[k][0]]
            bt = RTYPE[members[bj]["reduce"]["acc"]]
            fexp = fname("exp", spec.ext[k][0])
            S.append("    %s om = (%s)(-INFINITY); %s os = 0;" % (xt, xt, bt))
            S.append("    for (i64 c0 = (i64)threadIdx.x * %d; c0 < a.K; c0 += %d) {" % (V, T_BLOCK * V))
            S.append("      const Pack<%s, %d> xv = *(const Pack<%s, %d>*)(xp%d + c0);" % (xt, V, xt, V, k))
            S.append("      %s cm = xv.v[0];" % xt)
            for j in range(1, V):
                S.append("      cm = fmax_nan<%s>(cm, xv.v[%d]);" % (xt, j))
            S.append("      const %s nm = fmax_nan<%s>(om, cm);" % (xt, xt))
            S.append("      if (!(nm == om)) { os = os * (%s)exp((double)om - (double)nm); om = nm; }" % bt)
            for j in range(V):
                S.append("      os += (%s)%s(xv.v[%d] - om);" % (bt, fexp, j))
            S.append("    }")
            # block combine: global max, then rescaled sums in wave / lane order
            S.append("    %s gm = om;" % xt)
            S.append("    for (int s_ = 32; s_ > 0; s_ >>= 1) gm = fmax_nan<%s>(gm, shfl_xor_<%s>(gm, s_));" % (xt, xt))
            S.append("    __syncthreads();")
            S.append("    if (lane == 0) ((%s*)red_sm)[wave] = gm;" % xt)
            S.append("    __syncthreads();")
            S.append("    gm = ((%s*)red_sm)[0];" % xt)
            S.append("    for (int w_ = 1; w_ < %d; ++w_) gm = fmax_nan<%s>(gm, ((%s*)red_sm)[w_]);" % (nw, xt, xt))
            S.append("    %s gs = (om == gm || os == 0) ? os : os * (%s)exp((double)om - (double)gm);" % (bt, bt))
            S.append("    for (int s_ = 32; s_ > 0; s_ >>= 1) gs += shfl_xor_<%s>(gs, s_);" % bt)
            S.append("    __syncthreads();")
            S.append("    if (lane == 0) ((%s*)red_sm)[wave] = gs;" % bt)
            S.append("    __syncthreads();")
            S.append("    gs = ((%s*)red_sm)[0];" % bt)
            S.append("    for (int w_ = 1; w_ < %d; ++w_) gs += ((%s*)red_sm)[w_];" % (nw, bt))
            for idx, val, accd in ((mi, "gm", red["acc"]), (bj, "gs", members[bj]["reduce"]["acc"])):
                rr = members[idx]["reduce"]
                S.append("    const %s r%d = %s;" % (RTYPE[rr["out"]], idx, cast(val, accd, rr["out"])))
                rdt[idx] = rr["out"]
                if rr.get("slot") is not None:
                    S.append("    if (threadIdx.x == 0) ((%s*)a.ptr[%d])[%s] = %s;"
                             % (CTYPE[rr["out"]], rr["slot"], row_off(rr["slot"]),
                                store_val("r%d" % idx, rr["out"], rr["out"])))
            fused_done.add(bj)
            stage += 1
            continue
        acc_t = RTYPE[red["acc"]]
        S.append("    %s acc%d = %s;" % (acc_t, mi, red_identity(red["op"], red["acc"])))

        def tail(j, outs, mi=mi, red=red):
            oe, od = outs[mi]
            v = cast(oe[red["ref"]], od[red["ref"]], red["acc"])
            S.append("      acc%d = %s;" % (mi, red_combine(red["op"], red["acc"], "acc%d" % mi, v)))
        emit_sweep(stage, closure([mi]), tail)
        stage += 1
        # block reduce, result to every thread (fixed order: deterministic)
        S.append("    for (int s_ = 32; s_ > 0; s_ >>= 1) acc%d = %s;"
                 % (mi, red_combine(red["op"], red["acc"], "acc%d" % mi,
                                    "shfl_xor_<%s>(acc%d, s_)" % (acc_t, mi))))
        S.append("    __syncthreads();")
        S.append("    if (lane == 0) ((%s*)red_sm)[wave] = acc%d;" % (acc_t, mi))
        S.append("    __syncthreads();")
        S.append("    %s tot%d = ((%s*)red_sm)[0];" % (acc_t, mi, acc_t))
        S.append("    for (int w_ = 1; w_ < %d; ++w_) tot%d = %s;"
                 % (nw, mi, red_combine(red["op"], red["acc"], "tot%d" % mi, "((%s*)red_sm)[w_]" % acc_t)))
        S.append("    const %s r%d = %s;" % (RTYPE[red["out"]], mi, cast("tot%d" % mi, red["acc"], red["out"])))
        rdt[mi] = red["out"]
        if red.get("slot") is not None:
            S.append("    if (threadIdx.x == 0) ((%s*)a.ptr[%d])[%s] = %s;"
                     % (CTYPE[red["out"]], red["slot"], row_off(red["slot"]),
                        store_val("r%d" % mi, red["out"], red["out"])))
    emit_rowlike_ready(True)
    # final sweep: members with full-size stores
    storing = [mi for mi, m in enumerate(members) if m.get("stores") and not rowlike[mi]]
    if storing:
        packs = {}
        for mi in storing:
            for oref, odt, slot in members[mi]["stores"]:
                packs[(mi, oref, slot)] = odt

        def tail(j, outs):
            for (mi, oref, slot), odt in packs.items():
                oe, od = outs[mi]
                if j == 0:
                    S.append("      Pack<%s, %d> y%d;" % (CTYPE[odt], V, slot))
                S.append("      y%d.v[%d] = %s;" % (slot, j, store_val(oe[oref], od[oref], odt)))
                if j == V - 1:
                    S.append("      *(Pack<%s, %d>*)((%s*)a.ptr[%d] + %s + c0) = y%d;"
                             % (CTYPE[odt], V, CTYPE[odt], slot, row_off(slot), slot))
        emit_sweep(stage, closure(storing), tail)
    S.append("    __syncthreads();")
    S.append("  }")
    S.append("}")
    return "\n".join(S) + "\n", (name,)
