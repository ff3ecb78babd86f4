"""Plan-level fusion performed by the HIP linker before execution.

The reference's rewriter already fuses Elemwise chains into ``Composite`` ops
(tensor/rewriting/elemwise.py:523 local_elemwise_fusion_op) but (a) never fuses an Elemwise into
the CAReduce that consumes it for a non-C target (``local_careduce_fusion`` :942 is C-only and
single-input) and (b) leaves tiny broadcast producers (``square(sigma)`` in BASELINE config 2)
as separate nodes.  On a GPU every extra node is a kernel boundary (≈1.5–2 µs, MI355X guide
"boundary" row) and, for Elemwise→Sum, a full HBM round trip of the intermediate — so the linker
fuses them here, where it is legal: it sees adjacent nodes, client lists and output status.

Produces a list of :class:`Step`:

* ``kind == "elemwise"`` — one generated kernel: ``scalar`` over ``inputs`` -> ``outputs``
* ``kind == "reduce"``   — Elemwise producer (possibly identity) + CAReduce in one kernel
* ``kind == "rowdot"``   — D = A . x (a Gemv stripped of its alpha/beta epilogue)
* ``kind == "gemv_epi"`` — chain of row dots + the Elemwise that consumes them, one kernel
* ``kind == "node"``     — any other plan node, executed by its handler

``Gemv(y, alpha, A, x, beta)`` (tensor/blas.py:231) is split into ``D = rowdot(A, x)`` and the
elementwise ``beta*y + alpha*D`` so that the ordinary Elemwise fusion merges Gemv chains
(``y`` itself a Gemv) and neighbouring Composites around the dot products; whatever elementwise
step finally consumes the dots becomes one ``gemv_epi`` kernel (one GRU gate of BASELINE
config 4 = 1 launch instead of 5).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

from ._lib import AHIP_MAXOPS
from .plan import Node, Plan

MAX_FUSED_OPERANDS = AHIP_MAXOPS - 2


@dataclass
class Step:
    kind: str
    inputs: List[int]
    outputs: List[int]
    scalar: Optional[dict] = None
    out_refs: List[int] = field(default_factory=list)  # scalar["out"] index per stored output
    reduce: Optional[Dict[str, Any]] = None            # scalar_op, axis, acc_dtype, out, ref
    node: Optional[Node] = None
    alive: bool = True
    dots: List[List[int]] = field(default_factory=list)  # gemv_epi: [A var, x var] per dot;
    #                               the scalar's first len(dots) inputs are the dot results
    extra: Dict[str, Any] = field(default_factory=dict)  # rowpass: reds, col_ref, ws vars
    post: List["Step"] = field(default_factory=list)     # rowpass: fold steps run after it
    fallback: List["Step"] = field(default_factory=list)  # rowpass: the unfused original steps


def _inline_constants(step: Step, plan: Plan):
    """Fold size-1 plan constants into the scalar expression as literals."""
    keep, remap = [], {}

    def foldable(vid):
        return plan.const_scalar(vid) is not None
    # a step whose operands are ALL size-1 constants keeps the one of the highest rank as a real
    # operand: the step's shape (and the axes of a fused reduction) come from its operands
    anchor = None
    if step.inputs and all(foldable(v) for v in step.inputs):
        anchor = max(step.inputs, key=lambda v: len(plan.vars[v].shape))
        if not plan.vars[anchor].shape:
            anchor = None
    for pos, vid in enumerate(step.inputs):
        if vid != anchor and foldable(vid):
            remap[pos] = ["c", plan.const_scalar(vid), plan.vars[vid].dtype]
        else:
            if vid in keep:
                remap[pos] = ["i", keep.index(vid)]
            else:
                keep.append(vid)
                remap[pos] = ["i", len(keep) - 1]
    step.scalar = _remap_inputs(step.scalar, remap, len(keep))
    step.inputs = keep


def _remap_inputs(scalar, remap, n_in, t_shift=0):
    def rr(r):
        if r[0] == "i":
            return list(remap[r[1]])
        if r[0] == "t":
            return ["t", r[1] + t_shift]
        return list(r)

    return {"n_in": n_in,
            "nodes": [{"op": n["op"], "dtype": n["dtype"], "in": [rr(r) for r in n["in"]]}
                      for n in scalar["nodes"]],
            "out": [rr(r) for r in scalar["out"]]}


def _merge_producer(cons: Step, prod: Step, vid: int):
    """Inline single-output elemwise ``prod`` (producing ``vid``) into ``cons``."""
    new_inputs = []

    def slot(v):
        if v not in new_inputs:
            new_inputs.append(v)
        return new_inputs.index(v)

    # producer nodes first
    p_remap = {pos: ["i", slot(v)] for pos, v in enumerate(prod.inputs)}
    ps = _remap_inputs(prod.scalar, p_remap, 0)
    p_out = ps["out"][prod.out_refs[prod.outputs.index(vid)]]
    shift = len(ps["nodes"])
    c_remap = {}
    for pos, v in enumerate(cons.inputs):
        c_remap[pos] = list(p_out) if v == vid else ["i", slot(v)]
    cs = _remap_inputs(cons.scalar, c_remap, 0, t_shift=shift)
    cons.scalar = {"n_in": len(new_inputs), "nodes": ps["nodes"] + cs["nodes"], "out": cs["out"]}
    cons.inputs = new_inputs


def build_steps(plan: Plan, fuse: bool = True) -> List[Step]:
    clients = plan.clients()
    out_set = set(plan.outputs)
    steps: List[Step] = []
    producer: Dict[int, Step] = {}

    for ni, node in enumerate(plan.nodes):
        gemv_split = fuse and node.op == "Gemv" and _gemv_splittable(plan, node)
        if node.op == "Elemwise" or gemv_split:
            if gemv_split:
                st = _split_gemv(plan, node, steps, producer)
            else:
                sc = copy.deepcopy(node.params["scalar"])
                st = Step("elemwise", list(node.inputs), list(node.outputs), sc,
                          out_refs=list(range(len(node.outputs))))
            _inline_constants(st, plan)
            if fuse:
                changed = True
                while changed:
                    changed = False
                    for vid in list(st.inputs):
                        p = producer.get(vid)
                        if (p is None or not p.alive or p.kind != "elemwise"
                                or len(p.outputs) != 1 or vid in out_set):
                            continue
                        if any(c[0] != ni for c in clients[vid]):
                            continue
                        n_ops = len(set(st.inputs + p.inputs) - {vid}) + len(st.outputs)
                        if n_ops > MAX_FUSED_OPERANDS:
                            continue
                        _merge_producer(st, p, vid)
                        p.alive = False
                        changed = True
                        break
            steps.append(st)
            for o in st.outputs:
                producer[o] = st
        elif node.op == "CAReduce":
            vid = node.inputs[0]
            red = {"scalar_op": node.params["scalar_op"], "axis": node.params["axis"],
                   "acc_dtype": node.params["acc_dtype"], "out": node.outputs[0], "ref": None}
            p = producer.get(vid) if fuse else None
            if p is not None and p.alive and p.kind == "elemwise" and \
                    len(p.inputs) + len(p.outputs) + 1 <= MAX_FUSED_OPERANDS:
                others = [c for c in clients[vid] if c[0] != ni]
                k = p.outputs.index(vid)
                red["ref"] = p.out_refs[k]
                p.kind = "reduce"
                p.reduce = red
                if not others and vid not in out_set:
                    # intermediate never leaves the kernel
                    del p.outputs[k]
                    del p.out_refs[k]
                producer[node.outputs[0]] = p
                # the fused step now also defines the reduce output; keep its position
                continue
            st = Step("reduce", [vid], [], {"n_in": 1, "nodes": [], "out": [["i", 0]]},
                      out_refs=[], reduce=dict(red, ref=0))
            steps.append(st)
            producer[node.outputs[0]] = st
        else:
            st = Step("node", list(node.inputs), list(node.outputs), node=node)
            steps.append(st)
            for o in node.outputs:
                producer[o] = st
    steps = [s for s in steps if s.alive]
    if fuse:
        steps = _drop_dead(plan, _fuse_dots(plan, steps))
        steps = _fuse_rowpass(plan, steps)
        steps = _fuse_rowchain(plan, steps)
        steps = _fuse_gemm_epi(plan, steps)
        steps = _fuse_xprologue(plan, steps)
    return steps


_PURE_NODES = {"AllocEmpty", "Alloc", "DimShuffle", "Shape_i", "Shape", "ViewOp", "SpecifyShape",
               "Subtensor", "Reshape", "ScalarFromTensor", "TensorFromScalar", "MakeVector",
               "BroadcastTo", "DeepCopyOp", "RFFT", "IRFFT", "Conv2d", "Conv2dGradW",
               "Conv2dGradI", "Pool", "MaxPoolGrad", "AvgPoolGrad", "MaxPoolGradGrad",
               # (MrgUniform is not listed: with ``inplace`` it writes its state operand)
               "MultinomialFromUniform", "ChoiceFromUniform"}


def _drop_dead(plan: Plan, steps: List[Step]) -> List[Step]:
    """Remove side-effect-free steps whose outputs nobody reads any more (e.g. the AllocEmpty
    that only fed the ignored ``y`` of a ``beta == 0`` Gemv)."""
    live = set(plan.outputs)
    keep = []
    for s in reversed(steps):
        outs = list(s.outputs) + ([s.reduce["out"]] if s.reduce else [])
        pure = s.kind in ("elemwise", "rowdot", "gemv_epi") or \
            (s.kind == "node" and s.node.op in _PURE_NODES)
        if pure and not any(o in live for o in outs):
            continue
        keep.append(s)
        live.update(s.inputs)
        for d in s.dots:
            live.update(d)
    return list(reversed(keep))


def _gemv_splittable(plan: Plan, node: Node) -> bool:
    y, alpha, A, x, beta = (plan.vars[i] for i in node.inputs)
    return (A.ndim == 2 and x.ndim == 1 and A.dtype in ("float32", "float64")
            and A.dtype == x.dtype == y.dtype)


def _split_gemv(plan: Plan, node: Node, steps, producer) -> Step:
    """Gemv(y, alpha, A, x, beta) -> rowdot step + elementwise step beta*y + alpha*D."""
    yv, av, Av, xv, bv = node.inputs
    dt = plan.vars[node.outputs[0]].dtype
    d_var = plan.new_var(dt, [None], name="rowdot")
    dot = Step("rowdot", [Av, xv], [d_var])
    steps.append(dot)
    producer[d_var] = dot
    beta = plan.const_scalar(bv)
    if beta is not None and float(beta) == 0.0:
        # BLAS semantics: beta == 0 never reads y (it is usually an uninitialised AllocEmpty)
        sc = {"n_in": 2, "nodes": [{"op": "mul", "in": [["i", 0], ["i", 1]], "dtype": dt}],
              "out": [["t", 0]]}
        return Step("elemwise", [av, d_var], list(node.outputs), sc, out_refs=[0])
    if beta is not None:
        sc = {"n_in": 4, "nodes": [{"op": "mul", "in": [["i", 3], ["i", 0]], "dtype": dt},
                                   {"op": "mul", "in": [["i", 1], ["i", 2]], "dtype": dt},
                                   {"op": "add", "in": [["t", 0], ["t", 1]], "dtype": dt}],
              "out": [["t", 2]]}
        return Step("elemwise", [yv, av, d_var, bv], list(node.outputs), sc, out_refs=[0])
    # a RUN-TIME beta: the same rule per evaluation — beta == 0 never reads y (tensor/blas.py:236
    # Gemv.perform / BLAS xGEMV: a NaN or inf in y does not reach the result;
    # tests/tensor/test_blas_c.py:146 test_nan_beta_0)
    sc = {"n_in": 4, "nodes": [{"op": "mul", "in": [["i", 3], ["i", 0]], "dtype": dt},
                               {"op": "eq", "in": [["i", 3], ["c", 0.0, dt]], "dtype": "bool"},
                               {"op": "switch", "in": [["t", 1], ["c", 0.0, dt], ["t", 0]], "dtype": dt},
                               {"op": "mul", "in": [["i", 1], ["i", 2]], "dtype": dt},
                               {"op": "add", "in": [["t", 2], ["t", 3]], "dtype": dt}],
          "out": [["t", 4]]}
    return Step("elemwise", [yv, av, d_var, bv], list(node.outputs), sc, out_refs=[0])


def _fuse_dots(plan: Plan, steps: List[Step]) -> List[Step]:
    """Absorb rowdot steps into the elementwise step that consumes them (kind gemv_epi)."""
    from .codegen import AHIP_GV_MAXOPS, AHIP_MAXDOTS

    dot_of = {s.outputs[0]: s for s in steps if s.kind == "rowdot"}
    if not dot_of:
        return steps
    users: Dict[int, List[Step]] = {}
    for s in steps:
        for v in set(s.inputs):
            users.setdefault(v, []).append(s)
    outs = set(plan.outputs)
    for s in steps:
        if s.kind != "elemwise":
            continue
        dvars = [v for v in s.inputs if v in dot_of and len(users[v]) == 1 and v not in outs]
        if not dvars or len(dvars) > AHIP_MAXDOTS:
            continue
        others = [v for v in s.inputs if v not in dvars]
        if len(others) + len(s.outputs) > AHIP_GV_MAXOPS:
            continue
        # reorder the scalar inputs: dot results first, then the other operands
        order = dvars + others
        remap = {pos: ["i", order.index(v)] for pos, v in enumerate(s.inputs)}
        s.scalar = _remap_inputs(s.scalar, remap, len(order))
        s.inputs = others
        s.dots = [list(dot_of[v].inputs) for v in dvars]
        s.kind = "gemv_epi"
        for v in dvars:
            dot_of[v].alive = False
    return [s for s in steps if s.alive]


def _fuse_rowpass(plan: Plan, steps: List[Step]) -> List[Step]:
    """GLM pattern  z = X.w (+ epilogue) -> row-wise Elemwise / full Sum -> X.T.r  ==>  one
    single-pass "rowpass" step (X read once) + deterministic folds of its per-workgroup partials.

    The reference graph of BASELINE config 5 reads X twice (Gemv on X, Gemv on
    X.T); whenever every step between the two is row-wise the linker can legally keep each row
    in registers for both contractions."""
    from .codegen import RP_MAXOPS, RP_MAXRED

    producer_step = {}
    for s in steps:
        for o in list(s.outputs) + ([s.reduce["out"]] if s.reduce else []):
            producer_step[o] = s
    for i1, g1 in enumerate(steps):
        if g1.kind != "gemv_epi" or len(g1.dots) != 1:
            continue
        xv, wv = g1.dots[0]
        if plan.vars[xv].ndim != 2:
            continue
        # G2: a single dot over DimShuffle{1,0}(X)
        for i2 in range(i1 + 1, len(steps)):
            g2 = steps[i2]
            if g2.kind not in ("gemv_epi", "rowdot"):
                continue
            d2 = g2.dots if g2.kind == "gemv_epi" else [list(g2.inputs)]
            if len(d2) != 1:
                continue
            xt, rv = d2[0]
            ds = producer_step.get(xt)
            if not (ds is not None and ds.kind == "node" and ds.node.op == "DimShuffle"
                    and ds.node.params["new_order"] == [1, 0] and ds.inputs == [xv]):
                continue
            fused = _build_rowpass(plan, steps, i1, i2, xv, wv, rv, RP_MAXOPS, RP_MAXRED)
            if fused is not None:
                return fused
    return steps


def _build_rowpass(plan, steps, i1, i2, xv, wv, rv, max_ops, max_red):
    g1, g2 = steps[i1], steps[i2]
    dt = plan.vars[xv].dtype
    group, produced = [g1], set(g1.outputs)
    outside = []
    for s in steps[i1 + 1:i2]:
        ins = set(s.inputs) | {v for d in s.dots for v in d}
        if ins & produced:
            ok = s.kind in ("elemwise", "reduce") and not s.dots and \
                all(plan.vars[v].ndim <= 1 for v in s.inputs) and \
                all(plan.vars[o].ndim == 1 for o in s.outputs)
            if s.kind == "reduce":
                r = s.reduce
                ok = ok and r["scalar_op"] == "add" and (r["axis"] is None or r["axis"] == [0]) \
                    and r["acc_dtype"] in ("float32", "float64")
            if not ok:
                return None
            group.append(s)
            produced |= set(s.outputs) | ({s.reduce["out"]} if s.reduce else set())
        else:
            outside.append(s)
    if rv not in produced or plan.vars[rv].dtype != dt:
        return None
    # ---- merge the group's scalar programs: input 0 = the dot, then external row operands ----
    ext, nodes, ref_of = [], [], {}

    def slot(v):
        if v not in ext:
            ext.append(v)
        return ["i", 1 + ext.index(v)]

    def absorb(st, in_refs):
        base = len(nodes)

        def rr(r):
            if r[0] == "i":
                return list(in_refs[r[1]])
            if r[0] == "t":
                return ["t", r[1] + base]
            return list(r)
        for n in st.scalar["nodes"]:
            nodes.append({"op": n["op"], "dtype": n["dtype"], "in": [rr(r) for r in n["in"]]})
        return [rr(r) for r in st.scalar["out"]]

    reds = []
    for st in group:
        in_refs = ([["i", 0]] if st is g1 else []) + \
            [ref_of[v] if v in ref_of else slot(v) for v in st.inputs]
        outs = absorb(st, in_refs)
        for o, k in zip(st.outputs, st.out_refs):
            ref_of[o] = outs[k]
        if st.reduce:
            reds.append((outs[st.reduce["ref"]], st.reduce["acc_dtype"], st.reduce["out"]))
    if len(reds) > max_red:
        return None
    # which group-produced vectors must be materialised (consumers outside the fused group)
    users = {}
    for s in steps:
        if s in group or s is g2:
            continue
        for v in list(s.inputs) + [v for d in s.dots for v in d]:
            users.setdefault(v, []).append(s)
    g2_other = set(g2.inputs) if g2.kind == "gemv_epi" else set()
    mat = [v for st in group for v in st.outputs
           if v in users or v in plan.outputs or v in g2_other]
    if len(ext) + len(mat) > max_ops:
        return None
    scalar_out = [ref_of[v] for v in mat] + [r[0] for r in reds] + [ref_of[rv]]
    scalar = {"n_in": 1 + len(ext), "nodes": nodes, "out": scalar_out}
    n_mat = len(mat)
    col_ws = plan.new_var(dt, [None, None], name="rowpass_col_ws")
    d_var = plan.new_var(dt, [None], name="rowpass_xt_r")
    red_ws = [plan.new_var("float64", [None], name="rowpass_red_ws") for _ in reds]
    ident = {"n_in": 1, "nodes": [], "out": [["i", 0]]}
    post = [Step("reduce", [col_ws], [], ident, out_refs=[],
                 reduce={"scalar_op": "add", "axis": [0], "acc_dtype": "float64", "out": d_var,
                         "ref": 0})]
    if g2.kind == "gemv_epi":
        post.append(Step("elemwise", [d_var] + list(g2.inputs), list(g2.outputs), g2.scalar,
                         out_refs=list(g2.out_refs)))
    else:
        post.append(Step("elemwise", [d_var], list(g2.outputs), ident, out_refs=[0]))
    for (ref, acc, out), wsv in zip(reds, red_ws):
        post.append(Step("reduce", [wsv], [], ident, out_refs=[],
                         reduce={"scalar_op": "add", "axis": None, "acc_dtype": "float64",
                                 "out": out, "ref": 0}))
    rp = Step("rowpass", list(ext), list(mat), scalar, out_refs=list(range(n_mat)),
              dots=[[xv, wv]],
              extra={"reds": [[n_mat + j, acc] for j, (_, acc, _) in enumerate(reds)],
                     "col_ref": n_mat + len(reds), "col_ws": col_ws, "red_ws": red_ws,
                     "dtype": dt},
              post=post, fallback=group + [g2])
    return steps[:i1] + outside + [rp] + steps[i2 + 1:]


# ----------------------------------------------------------------------------------------
# row chains: last-axis reductions + the Elemwise steps between them -> one kernel
# ----------------------------------------------------------------------------------------
def _step_reads(st: Step):
    used = list(st.inputs) + [v for d in st.dots for v in d]
    for xp in st.extra.get("xprog", {}).values():
        used += list(xp["step"].inputs)
    for q in st.fallback + st.post:
        used += _step_reads(q)
    return used


def _fuse_rowchain(plan: Plan, steps: List[Step], max_ops: int = 16) -> List[Step]:
    """A last-axis CAReduce whose (keepdims) result feeds Elemwise / further last-axis CAReduce
    steps over the same [..., K] space (softmax = max -> exp-sum -> scale; log-softmax; softmax
    gradient; mean/variance normalisation) becomes ONE "rowchain" step: every operand is read
    once, every intermediate between the reductions lives in registers (codegen.rowchain.RowChainSpec).
    The reference runs such chains as separate passes (Softmax.c_code tensor/special.py:372-415)
    or separate nodes.  Run-time layout checks are the executor's; the original steps are kept
    as the fallback."""
    while True:
        fused = _fuse_one_rowchain(plan, steps, max_ops)
        if fused is None:
            return steps
        steps = fused


def _fuse_one_rowchain(plan: Plan, steps: List[Step], max_ops: int):
    out_set = set(plan.outputs)
    for i, seed in enumerate(steps):
        if seed.kind != "reduce" or not seed.inputs:
            continue
        D = plan.vars[seed.inputs[0]].ndim
        if D < 2 or seed.reduce["axis"] != [D - 1]:
            continue
        if any(plan.vars[v].ndim != D for v in seed.inputs):
            continue
        keep_order = list(range(D - 1)) + ["x"]
        members, glue = [i], []
        red_of = {seed.reduce["out"]: i}           # raw reduce result -> step index
        row_vars: Dict[int, int] = {}              # keepdims var -> step index of its reduce
        full_vars = {o: i for o in seed.outputs}   # [..., K] intermediates -> producing step
        for j in range(i + 1, len(steps)):
            t = steps[j]
            if (t.kind == "node" and t.node.op == "DimShuffle" and t.inputs[0] in red_of
                    and t.node.params["new_order"] == keep_order):
                row_vars[t.outputs[0]] = red_of[t.inputs[0]]
                glue.append(j)
                continue
            reads = _step_reads(t)
            if not any(v in row_vars or v in full_vars or v in red_of for v in reads):
                continue
            ok = (t.kind in ("elemwise", "reduce") and t.inputs and not t.dots
                  and all(plan.vars[v].ndim == D for v in t.inputs)
                  and not any(v in red_of for v in t.inputs)
                  and (t.kind != "reduce" or t.reduce["axis"] == [D - 1]))
            if not ok:
                break
            members.append(j)
            for o in t.outputs:
                full_vars[o] = j
            if t.kind == "reduce":
                red_of[t.reduce["out"]] = j
        if len(members) < 2:
            continue
        # absorb Elemwise producers whose results only the chain reads (softmax(x / T + mask):
        # the logits never go to memory)
        readers: Dict[int, set] = {}
        made_by: Dict[int, int] = {}
        for j, t in enumerate(steps):
            for v in _step_reads(t):
                readers.setdefault(v, set()).add(j)
            if t.kind == "elemwise" and not t.dots:
                for o in t.outputs:
                    made_by[o] = j
        grown = True
        while grown:
            grown = False
            for j in list(members):
                for v in steps[j].inputs:
                    pj = made_by.get(v)
                    if pj is None or pj in members or pj > members[-1]:
                        continue
                    P = steps[pj]
                    if not P.inputs or any(plan.vars[u].ndim != D for u in P.inputs):
                        continue
                    if any(o in out_set or not readers.get(o, set()) <= set(members)
                           for o in P.outputs):
                        continue
                    members = sorted(members + [pj])
                    for o in P.outputs:
                        full_vars[o] = pj
                    grown = True
                    break
                if grown:
                    break
        last = members[-1]
        glue = [g for g in glue if g < last]
        inside = set(members) | set(glue)
        used_outside = set(out_set)
        for j, t in enumerate(steps):
            if j not in inside:
                used_outside.update(_step_reads(t))
        pos = {j: k for k, j in enumerate(members)}
        ext: List[int] = []
        mlist, stored, keep = [], [], {}
        for j in members:
            t = steps[j]
            ins = []
            for v in t.inputs:
                if v in full_vars and full_vars[v] != j:
                    p = steps[full_vars[v]]
                    ins.append(["f", pos[full_vars[v]], p.out_refs[p.outputs.index(v)]])
                elif v in row_vars:
                    ins.append(["r", pos[row_vars[v]]])
                else:
                    if v not in ext:
                        ext.append(v)
                    ins.append(["e", ext.index(v)])
            m = {"scalar": copy.deepcopy(t.scalar), "ins": ins, "reduce": None, "stores": []}
            for o, ref in zip(t.outputs, t.out_refs):
                if o in used_outside:
                    m["stores"].append([ref, o])
                    stored.append(o)
            if t.kind == "reduce":
                r = t.reduce
                m["reduce"] = {"op": r["scalar_op"], "acc": r["acc_dtype"], "ref": r["ref"],
                               "out": r["out"], "store": False}
                need = r["out"] in used_outside
                for g in glue:
                    gk = steps[g]
                    if gk.inputs[0] == r["out"] and gk.outputs[0] in used_outside:
                        keep[gk.outputs[0]] = r["out"]
                        need = True
                if need:
                    m["reduce"]["store"] = True
                    stored.append(r["out"])
            mlist.append(m)
        if not stored or len(ext) + len(stored) > max_ops:
            continue
        fb = [steps[j] for j in sorted(inside)]
        rc = Step("rowchain", ext, stored, extra={"members": mlist, "D": D, "keep": keep},
                  fallback=fb)
        return [rc if j == last else s for j, s in enumerate(steps) if j == last or j not in inside]
    return None


# ----------------------------------------------------------------------------------------
# small-M GEMM chain + Elemwise consumer -> one kernel (kind "gemm_epi")
# ----------------------------------------------------------------------------------------
def _fuse_gemm_epi(plan: Plan, steps: List[Step], max_dots: int = 3, max_ops: int = 12) -> List[Step]:
    """``Gemm`` / ``Dot22`` nodes whose only reader is one Elemwise step (a recurrent gate
    ``sigmoid(h @ U + V_t) * h``, an MLP layer ``tanh(x @ W + b)``) become one "gemm_epi" step: the
    products are accumulated by the 16-row split-K MFMA schedule and the Elemwise runs on the
    accumulators.  Only worth it (and only generated) for outputs too small to fill the chip with
    128x128 tiles — the executor decides from the run-time shapes and otherwise runs the original
    steps, which are kept as the fallback (the big GEMM has its own alpha/beta epilogue)."""
    out_set = set(plan.outputs)
    readers: Dict[int, List[int]] = {}
    for j, t in enumerate(steps):
        for v in set(_step_reads(t)):
            readers.setdefault(v, []).append(j)

    def const1(vid):
        return plan.const_scalar(vid) is not None

    producer = {}
    for j, t in enumerate(steps):
        if t.kind == "node" and t.node.op in ("Gemm", "Dot22", "Dot22Scalar"):
            producer[t.outputs[0]] = j
    if not producer:
        return steps
    removed, replaced = set(), {}
    for j, e in enumerate(steps):
        if e.kind != "elemwise" or e.dots or any(plan.vars[v].ndim != 2 for v in e.inputs):
            continue
        prods = []
        for v in e.inputs:
            pj = producer.get(v)
            if pj is None or pj in removed or v in out_set or readers.get(v) != [j]:
                continue
            n = steps[pj].node
            if plan.vars[v].dtype not in ("float32", "float64"):
                continue
            if n.op == "Gemm" and not (const1(n.inputs[1]) and const1(n.inputs[4])):
                continue
            if n.op == "Dot22Scalar" and not const1(n.inputs[2]):
                continue
            prods.append((v, pj))
        if not prods or len(prods) > max_dots:
            continue
        merged = Step("elemwise", list(e.inputs), list(e.outputs), copy.deepcopy(e.scalar),
                      out_refs=list(e.out_refs))
        dvars, dots = [], []
        for v, pj in prods:
            n = steps[pj].node
            dt = plan.vars[v].dtype
            d_var = plan.new_var(dt, [None, None], name="matdot")
            if n.op == "Dot22":
                dots.append([n.inputs[0], n.inputs[1]])
                pseudo = Step("elemwise", [d_var], [v], {"n_in": 1, "nodes": [], "out": [["i", 0]]},
                              out_refs=[0])
            elif n.op == "Dot22Scalar":   # dot(x, y) * a
                dots.append([n.inputs[0], n.inputs[1]])
                sc = {"n_in": 2, "out": [["t", 0]], "nodes": [
                    {"op": "mul", "dtype": dt, "in": [["i", 0], ["i", 1]]}]}
                pseudo = Step("elemwise", [d_var, n.inputs[2]], [v], sc, out_refs=[0])
                _inline_constants(pseudo, plan)
            else:   # Gemm(z, alpha, x, y, beta) = beta*z + alpha*dot(x, y)
                z, al, x, y, be = n.inputs
                dots.append([x, y])
                sc = {"n_in": 4, "out": [["t", 2]], "nodes": [
                    {"op": "mul", "dtype": dt, "in": [["i", 1], ["i", 0]]},
                    {"op": "mul", "dtype": dt, "in": [["i", 3], ["i", 2]]},
                    {"op": "add", "dtype": dt, "in": [["t", 1], ["t", 0]]}]}
                pseudo = Step("elemwise", [d_var, al, z, be], [v], sc, out_refs=[0])
                _inline_constants(pseudo, plan)
            _merge_producer(merged, pseudo, v)
            dvars.append(d_var)
        others = [v for v in merged.inputs if v not in dvars]
        if len(others) + len(merged.outputs) > max_ops or \
                any(plan.vars[v].ndim != 2 for v in others):
            continue
        order = dvars + others
        remap = {pos: ["i", order.index(v)] for pos, v in enumerate(merged.inputs)}
        merged.scalar = _remap_inputs(merged.scalar, remap, len(order))
        merged.inputs = others
        merged.dots = dots
        merged.kind = "gemm_epi"
        merged.fallback = [steps[pj] for _, pj in prods] + [e]
        replaced[j] = merged
        removed.update(pj for _, pj in prods)
    if not replaced:
        return steps
    return [replaced.get(j, s) for j, s in enumerate(steps) if j not in removed]


def _fuse_xprologue(plan: Plan, steps: List[Step]) -> List[Step]:
    """The vector of a fused GEMV chain that is itself a small Elemwise of vectors (the
    ``delta * (1 - h**2)`` feeding ``W . (...)`` in every step of a backward RNN Scan) is evaluated
    by the GEMV kernel while it loads the vector (and stored by its first wavefront when anything
    else reads it): one launch less per step.  The Elemwise step is kept inside the fused step and
    run as before whenever the run-time layout does not qualify."""
    out_set = set(plan.outputs)
    readers: Dict[int, List[int]] = {}
    made_by: Dict[int, int] = {}
    for j, t in enumerate(steps):
        for v in set(_step_reads(t)):
            readers.setdefault(v, []).append(j)
        if t.kind == "elemwise" and not t.dots and len(t.outputs) == 1:
            made_by[t.outputs[0]] = j
    removed = set()
    for j, g in enumerate(steps):
        if g.kind != "gemv_epi":
            continue
        for d, (_a, xv) in enumerate(g.dots):
            pj = made_by.get(xv)
            if pj is None or pj in removed or pj > j:
                continue
            P = steps[pj]
            if not (1 <= len(P.inputs) <= 4 and len(P.scalar["nodes"]) <= 12
                    and all(plan.vars[u].ndim <= 1 for u in P.inputs)
                    and all(plan.vars[u].dtype == plan.vars[xv].dtype for u in P.inputs)):
                continue
            rd = [r for r in readers.get(xv, []) if r != j]
            if any(pj < r < j for r in rd):
                continue          # something between needs the vector before the GEMV runs
            g.extra.setdefault("xprog", {})[d] = {"step": P, "store": bool(rd) or xv in out_set}
            removed.add(pj)
    if not removed:
        return steps
    return [s_ for j, s_ in enumerate(steps) if j not in removed]
