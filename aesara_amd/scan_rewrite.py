"""Plan-to-plan rewrites around ``Scan`` nodes: what leaves a loop before it runs.

Two groups.  The OUTER rewrites take a plan with Scan nodes and move work in front of or behind
the loop (``PlanExecutor.__init__`` applies them in this order; ``ScanMixin._op_Scan`` applies the
third to a single node once buffer lengths are known):

* :func:`push_out_sequence_glue` — index glue on sequence rows, restated over whole sequences;
* :func:`push_out_accumulators` — sit-sot sums of a nit-sot output, rebuilt by one cumulative sum;
* :func:`push_out_product_accumulators` — products / scatters summed in the loop, as one product;
* :func:`split_assembled_columns` — gate gradients assembled per step, handed out as blocks.

The STEP rewrites take a Scan's inner plan: :func:`split_column_slices`, :func:`split_invariant`,
:func:`hoist_sequence_only`, :func:`hoist_sequence_dots`, :func:`batch_map_step` (no recurrence at
all) and :func:`merge_shared_left_dots` on a lifted plan.  Together they decide whether a
recurrence reaches the persistent kernels (scan_persist*.py).

Variable ids come from ``Plan.new_var`` in creation order, and golden launch records depend on
them: a rewrite creates its variables in the order it emits their nodes (:class:`_Emit`), and the
few places that create a constant between an output variable and its node say so.
"""
from __future__ import annotations

import copy
from typing import Dict, List

import numpy as np

from .plan import Node, Plan


def _cfloat(plan: Plan, vid):
    """value of a size-1 constant as a float, else None"""
    c = plan.const_scalar(vid)
    return None if c is None else float(c)


def _cint(plan: Plan, vid):
    """value of a size-1 INTEGER constant, else None"""
    c = plan.const_scalar(vid)
    return int(c) if c is not None and plan.vars[vid].dtype.startswith("int") else None


def _is_add(sc) -> bool:
    """the scalar expression ``i0 + i1``"""
    return (sc.get("n_in") == 2 and len(sc["nodes"]) == 1 and sc["nodes"][0]["op"] == "add"
            and sorted(map(tuple, sc["nodes"][0]["in"])) == [("i", 0), ("i", 1)] and sc["out"] == [["t", 0]])


def _host_int(op, n_in=2, clamp=False):
    """Elemwise params of ``op(i0[, i1])`` on host integers; ``clamp``: ``max(.., 0)`` of it"""
    nodes = [{"op": op, "in": [["i", k] for k in range(n_in)], "dtype": "int64"}]
    if clamp:
        nodes.append({"op": "maximum", "in": [["t", 0], ["c", 0, "int64"]], "dtype": "int64"})
    return {"scalar": {"n_in": n_in, "nodes": nodes, "out": [["t", len(nodes) - 1]]}}


class _Emit:
    """Node builder bound to a plan and a sink list: ``emit(op, ins, dtype, shape, params)`` creates
    the output variable, appends the node and returns the variable."""

    def __init__(self, plan: Plan, sink: list):
        self.plan, self.sink = plan, sink

    def __call__(self, op, ins, dtype, shape, params=None):
        o = self.plan.new_var(dtype, list(shape))
        self.sink.append(Node(op, list(ins), [o], dict(params or {})))
        return o


class ScanSlots:
    """Where the operand classes of a Scan node sit (the reference's order, scan/op.py:286
    ``ScanMethodsMixin``): the counts, and the POSITIONS the rewrites use — ``in_*`` in
    ``node.inputs`` (n_steps, sequences, mit-mot / mit-sot / sit-sot inits, shared, nit-sot lengths,
    non-sequences), ``out_*`` in ``node.outputs`` (mit-mot, mit-sot, sit-sot, nit-sot, shared),
    ``iin_*`` in ``inner.inputs`` (sequences, mit-mot / mit-sot / sit-sot taps, shared,
    non-sequences) and ``iout_*`` in ``inner.outputs`` (mit-mot out-taps, mit-sot, sit-sot, nit-sot,
    shared)."""

    def __init__(self, node: Node):
        p = node.params
        self.node, self.inner = node, p["inner"]
        mm_in, mm_out, ms = p.get("mit_mot_in_slices", []), p.get("mit_mot_out_slices", []), p["mit_sot_in_slices"]
        self.n_seqs, self.n_mm, self.n_ms, self.n_ss = p["n_seqs"], len(mm_in), len(ms), len(p["sit_sot_in_slices"])
        self.n_sh, self.n_nit, self.n_non = p.get("n_shared_outs", 0), p["n_nit_sot"], p["n_non_seqs"]
        self._in0 = 1 + self.n_seqs + self.n_mm + self.n_ms                 # first sit-sot init
        self._iin0 = self.n_seqs + sum(len(t) for t in mm_in) + sum(len(t) for t in ms)   # first sit-sot tap
        self._iout0 = sum(len(t) for t in mm_out) + self.n_ms               # first inner sit-sot output
        self.in_non0 = len(node.inputs) - self.n_non                        # first non-sequence
        self.iin_inv0 = len(self.inner.inputs) - self.n_non                 # first invariant of the step

    def in_seq(self, k):
        return 1 + k

    def in_init(self, q):
        return self._in0 + q

    def in_nit_len(self, j):
        return self._in0 + self.n_ss + self.n_sh + j

    def out_ss(self, q):
        return self.n_mm + self.n_ms + q

    def out_nit(self, j):
        return self.n_mm + self.n_ms + self.n_ss + j

    def iin_tap(self, q):
        return self._iin0 + q

    def iout_ss(self, q):
        return self._iout0 + q

    def iout_nit(self, j):
        return self._iout0 + self.n_ss + j

    def drop_sit_sots(self, dq):
        """[node.inputs, node.outputs, inner.inputs, inner.outputs] without the sit-sots ``dq``"""
        return [[v for k, v in enumerate(lst) if k - first not in dq]
                for lst, first in ((self.node.inputs, self.in_init(0)), (self.node.outputs, self.out_ss(0)),
                                   (self.inner.inputs, self.iin_tap(0)), (self.inner.outputs, self.iout_ss(0)))]

    def insert_nit_sots(self, lists, j, lengths, outs, inner_outs, n_old=0, n_dropped=0):
        """The four lists (as above; ``n_dropped`` sit-sots already gone) with further nit-sots in
        front of nit-sot ``j`` (None: behind the last), replacing ``n_old`` there: their lengths
        (node.inputs), their outer and their inner outputs."""
        j = self.n_nit if j is None else j
        ins, outs0, iins, iouts = lists
        a, b, c = (at - n_dropped for at in (self.in_nit_len(j), self.out_nit(j), self.iout_nit(j)))
        return [ins[:a] + list(lengths) + ins[a + n_old:], outs0[:b] + list(outs) + outs0[b + n_old:], iins,
                iouts[:c] + list(inner_outs) + iouts[c + n_old:]]


def _patch(plan: Plan, nodes: List[Node], replaced: dict) -> Plan:
    """``plan`` with ``nodes``, every reader of a key of ``replaced`` (the outputs too) reading its value"""
    plan.nodes = [Node(n.op, [replaced.get(i, i) for i in n.inputs], list(n.outputs), n.params) for n in nodes]
    plan.outputs = [replaced.get(o, o) for o in plan.outputs]
    return plan


def _rewrite_scans(plan: Plan, rewrite) -> Plan:
    """The frame of the outer rewrites: ``rewrite(work, node, slots, replaced)`` for every Scan node
    (no do-while) gives the nodes that take its place, or None; old outputs are renamed through
    ``replaced``.  Returns ``plan`` itself when no node changed."""
    work = plan.copy()
    out_nodes, replaced, changed = [], {}, False
    for node in plan.nodes:
        new = None
        if node.op == "Scan" and not node.params.get("as_while"):
            new = rewrite(work, node, ScanSlots(node), replaced)
        if new is None:
            out_nodes.append(node)
        else:
            out_nodes.extend(new)
            changed = True
    return _patch(work, out_nodes, replaced) if changed else plan


def _prune_dead(plan: Plan, keep: List[Node]) -> List[Node]:
    pure = {"AllocEmpty", "Shape_i", "Shape", "DimShuffle", "Elemwise", "ScalarFromTensor",
            "TensorFromScalar", "MakeVector", "Alloc", "ViewOp", "CAReduce", "Subtensor", "IncSubtensor",
            "Assert"}      # (an Assert nobody reads guards nothing that is still computed)
    while True:
        read = {i for n in keep for i in n.inputs} | set(plan.outputs)
        dead = [n for n in keep if n.op in pure and not any(o in read for o in n.outputs)]
        if not dead:
            return keep
        dead_ids = {id(n) for n in dead}
        keep = [n for n in keep if id(n) not in dead_ids]


def split_invariant(plan: Plan, invariant_inputs: List[int]):
    """Hoist loop-invariant nodes out of a Scan inner plan.

    ``invariant_inputs``: ids of the inner inputs that do not change across steps (the
    non-sequences).  Returns ``(pre_plan, loop_plan, hoisted)``: ``pre_plan`` maps the
    invariant inputs to the hoisted values (run once per Scan call), ``loop_plan`` takes the
    original inputs followed by the hoisted values.  Only view/shape ops are hoisted (they are
    free to recompute but hide loop-invariant *layouts* — e.g. the ``W.T`` DimShuffles feeding
    every Gemv of a GRU step — from the executor, which materialises them once)."""
    hoistable = {"DimShuffle", "Shape_i", "Shape", "ViewOp", "SpecifyShape", "Subtensor",
                 "Reshape", "ScalarFromTensor", "TensorFromScalar", "MakeVector"}
    inv = set(invariant_inputs)
    const_ids = {vid for vid, v in plan.vars.items() if v.const is not None}
    pre_nodes, loop_nodes = [], []
    for n in plan.nodes:
        if n.op in hoistable and all(i in inv or i in const_ids for i in n.inputs):
            pre_nodes.append(n)
            inv.update(n.outputs)
        else:
            loop_nodes.append(n)
    hoisted = []
    used = {i for n in loop_nodes for i in n.inputs} | set(plan.outputs)
    for n in pre_nodes:
        hoisted.extend(o for o in n.outputs if o in used)
    if not hoisted:
        return None, plan, []
    pre = Plan(plan.name + "_invariant", plan.vars, list(invariant_inputs), hoisted, pre_nodes)
    loop = Plan(plan.name + "_loop", plan.vars, list(plan.inputs) + hoisted, list(plan.outputs),
                loop_nodes)
    return pre, loop, hoisted


def split_column_slices(plan: Plan, invariant: set) -> Plan:
    """Fused-gate recurrences compute ONE product for all gates and slice it along its last axis::

        pre = b + x_t @ Wx + h @ Wh          # [B, 4H]   (or a vector of length 4H)
        i, f, o, g = pre[:, 0:H], pre[:, H:2H], ...

    (the usual Theano / Aesara LSTM step).  Every consumer sees only its slice, so the chain is
    split per slice with views of the invariant operands — ``x_t @ Wx[:, kH:(k+1)H]`` … — which
    leaves H-wide products with H-wide epilogues: the shape the sequence hoisting and the
    persistent kernels work on.  Handles a chain of ``Dot22`` / ``Gemm`` (matrix state) or ``Gemv``
    (vector state; the slice selects rows of the matrix) with an invariant matrix operand and
    ``Elemwise`` nodes (chain operands and invariant rows ``[1, N]`` / vectors), every value of
    which is read only inside the chain or by ``Subtensor`` nodes ``[..., a:b]`` with constant
    bounds.  Returns the plan unchanged when nothing matches."""
    V = plan.vars
    clients = plan.clients()
    # invariants and views of them computed in the step (the W.T of every Gemv)
    inv = set(invariant)
    for n in plan.nodes:
        if n.op in ("DimShuffle", "ViewOp") and all(i in inv for i in n.inputs):
            inv.update(n.outputs)

    def last_slice(n):
        """(a, b) when node n is Subtensor [..., a:b] on the last axis with constant bounds"""
        if n.op != "Subtensor":
            return None
        nd = V[n.inputs[0]].ndim
        idx = n.params["idx_list"]
        if nd not in (1, 2) or len(idx) != nd or any("slice" not in e for e in idx):
            return None
        if nd == 2 and idx[0]["slice"] != [None, None, None]:
            return None
        if idx[-1]["slice"][2] not in (None, 1):
            return None
        extra, ab = list(n.inputs[1:]), []
        for e in idx[-1]["slice"][:2]:
            if e == "in":
                c = _cint(plan, extra.pop(0)) if extra else None
                if c is None:
                    return None
                ab.append(c)
            elif isinstance(e, int):
                ab.append(e)
            else:
                return None
        return (ab[0], ab[1]) if 0 <= ab[0] < ab[1] and not extra else None

    producer = {o: (ni, n) for ni, n in enumerate(plan.nodes) for o in n.outputs}

    def chain_of(root):
        """node indices of the chain ending in `root`, or None"""
        nd = V[root].ndim
        chain, todo = set(), [root]
        while todo:
            v = todo.pop()
            if v not in producer:
                return None
            ni, n = producer[v]
            if ni in chain:
                continue
            if nd == 2 and n.op in ("Dot22", "Dot") and len(n.inputs) == 2 and n.inputs[1] in inv \
                    and V[n.inputs[1]].ndim == 2 and V[n.outputs[0]].ndim == 2:
                chain.add(ni)
            elif nd == 2 and n.op == "Gemm" and n.inputs[3] in inv and V[n.inputs[3]].ndim == 2:
                chain.add(ni)
                todo.append(n.inputs[0])
            elif nd == 1 and n.op == "Gemv" and n.inputs[2] in inv and V[n.inputs[2]].ndim == 2:
                chain.add(ni)
                y = n.inputs[0]
                if not (y in producer and producer[y][1].op == "AllocEmpty"):
                    todo.append(y)                 # beta != 0: accumulates onto a chain value
            elif n.op == "Elemwise" and len(n.outputs) == 1 and V[n.outputs[0]].ndim == nd \
                    and V[n.outputs[0]].shape[-1] != 1:
                chain.add(ni)
                for i in n.inputs:
                    if (i in inv or V[i].const is not None) and V[i].ndim == nd and \
                            (nd == 1 or V[i].shape[0] == 1):
                        continue
                    todo.append(i)
            else:
                return None
        return chain

    new_nodes, replaced, removed = {}, {}, set()
    work = plan.copy(nodes=[])
    for root, (rni, rn) in list(producer.items()):
        cl = clients.get(root, [])
        if len(cl) < 2 or any(c[0] == "out" for c in cl):
            continue
        slices = [last_slice(plan.nodes[c[0]]) if c[1] == 0 else None for c in cl]
        if any(sl is None for sl in slices):
            continue
        chain = chain_of(root)
        if not chain or chain & removed:
            continue
        nd = V[root].ndim
        chain_vars = {o for ni in chain for o in plan.nodes[ni].outputs}
        if not all(all(c[0] != "out" and (c[0] in chain or (v == root and last_slice(plan.nodes[c[0]])))
                       for c in clients[v]) for v in chain_vars):
            continue
        order = sorted(chain)
        for (cni, _pos), (a, b) in zip(cl, slices):
            m = {}
            sink = new_nodes.setdefault(cni, [])
            emit = _Emit(work, sink)

            def part(v, axis, a=a, b=b, m=m, emit=emit):
                """v[..., a:b] (axis = -1) or v[a:b] (axis = 0: rows of a Gemv matrix, the y of a
                beta = 0 Gemv) of an operand that is not a chain value"""
                key = ("p", v, axis)
                if key not in m:
                    src = V[v]
                    shp = list(src.shape)
                    shp[axis] = None
                    idx = [{"slice": [a, b, None]}] if axis == 0 else \
                        [{"slice": [None, None, None]}] * (src.ndim - 1) + [{"slice": [a, b, None]}]
                    m[key] = emit("Subtensor", [v], src.dtype, shp, {"idx_list": idx})
                return m[key]
            for ni in order:
                n = plan.nodes[ni]
                ov = V[n.outputs[0]]
                out = work.new_var(ov.dtype, list(ov.shape[:-1]) + [None])      # (before the operands' views)
                if n.op in ("Dot22", "Dot"):
                    nn = Node("Dot22", [n.inputs[0], part(n.inputs[1], -1)], [out], {})
                elif n.op == "Gemm":
                    nn = Node("Gemm", [m[n.inputs[0]], n.inputs[1], n.inputs[2], part(n.inputs[3], -1),
                                       n.inputs[4]], [out], dict(n.params))
                elif n.op == "Gemv":
                    y = n.inputs[0]
                    nn = Node("Gemv", [m[y] if y in m else part(y, 0), n.inputs[1], part(n.inputs[2], 0),
                                       n.inputs[3], n.inputs[4]], [out], dict(n.params))
                else:
                    # an operand that is broadcast along the sliced axis (static extent 1: a
                    # scalar handed in as [1, 1], a length-1 vector) has no columns a:b to cut —
                    # it stays whole and keeps broadcasting
                    nn = Node("Elemwise", [m[i] if i in m else (i if V[i].shape[-1] == 1 else part(i, -1))
                                           for i in n.inputs], [out], copy.deepcopy(n.params))
                m[n.outputs[0]] = out
                sink.append(nn)
            replaced[plan.nodes[cni].outputs[0]] = m[root]
            removed.add(cni)
        removed |= chain
    if not replaced:
        return plan
    nodes = []
    for ni, n in enumerate(plan.nodes):
        nodes.extend(new_nodes.get(ni, []))
        if ni not in removed:
            nodes.append(n)
    _patch(work, nodes, replaced)
    work.name = plan.name + "_cols"
    work.nodes = _prune_dead(work, list(work.nodes))
    return work


def _accumulators_out(plan: Plan, node: Node, L: ScanSlots, replaced: dict):
    """:func:`push_out_accumulators` for one Scan node"""
    inner, V = L.inner, plan.vars
    ss = [list(t) for t in node.params["sit_sot_in_slices"]]
    iprod, iclients = inner.producers(), inner.clients()
    nits = [inner.outputs[L.iout_nit(j)] for j in range(L.n_nit)]
    drop = []          # (q, nit index j, reduce params or None)
    for q in range(L.n_ss):
        if ss[q] != [-1]:
            continue
        tq, oq = inner.inputs[L.iin_tap(q)], inner.outputs[L.iout_ss(q)]
        upd = iprod.get(oq)
        if upd is None or upd.op != "Elemwise" or not _is_add(upd.params["scalar"]) or tq not in upd.inputs:
            continue
        if [c for c in iclients[tq]] != [c for c in iclients[tq] if c[0] != "out" and inner.nodes[c[0]] is upd] \
                or len(iclients[tq]) != 1 or len(iclients[oq]) != 1:
            continue
        a = [i for i in upd.inputs if i != tq]
        if len(a) != 1:
            continue
        a, red = a[0], None
        an = iprod.get(a)
        if an is not None and an.op == "CAReduce" and an.params["scalar_op"] == "add" and \
                an.params["axis"] == [0] and inner.vars[an.inputs[0]].ndim == 2:
            red, a = dict(an.params), an.inputs[0]
        if inner.vars[a].ndim != (2 if red else 1) or inner.vars[a].dtype != inner.vars[oq].dtype:
            continue
        if a in nits:
            drop.append((q, nits.index(a), red))
            continue
        # a vector handed out as a row ([1, n]: DimShuffle 'x', 0): summing the size-1 axis of
        # the [T, 1, n] output gives the [T, n] addends back
        via = [o for o in nits if o in iprod and iprod[o].op == "DimShuffle" and iprod[o].inputs[0] == a
               and iprod[o].params["new_order"] == ["x", 0]]
        if red is None and via:
            drop.append((q, nits.index(via[0]), {"scalar_op": "add", "axis": [0],
                                                 "acc_dtype": inner.vars[a].dtype}))
    if not drop:
        return None
    dq = {q for q, _j, _r in drop}
    new_inputs, new_outputs, in_keep, out_keep = L.drop_sit_sots(dq)
    new_inner = Plan(inner.name + "_noacc", inner.vars, in_keep, out_keep, list(inner.nodes))
    new_inner.nodes = _prune_dead(new_inner, list(new_inner.nodes))
    out = [Node("Scan", new_inputs, new_outputs, dict(
        node.params, inner=new_inner, sit_sot_in_slices=[t for q, t in enumerate(ss) if q not in dq]))]
    emit = _Emit(plan, out)
    for q, j, red in drop:
        old, init_buf, r = node.outputs[L.out_ss(q)], node.inputs[L.in_init(q)], node.outputs[L.out_nit(j)]
        dt = V[old].dtype
        width = V[init_buf].shape[1:]
        rows = [None] + list(width)
        if red is not None:
            r = emit("CAReduce", [r], dt, rows, dict(red, axis=[1]))
        # rows 0..T of the old buffer: init, init + g_1, (init + g_1) + g_2, ... — ONE cumulative
        # sum over [init; g_1; ...; g_T] (the loop's additions up to the association the CumOp
        # kernel uses for long columns: tolerance-level, like any reordered float sum)
        row = emit("Subtensor", [init_buf], dt, [1] + list(width), {"idx_list": [{"slice": [0, 1, None]}]})
        ax = plan.add_const(0, "int8")
        cat = emit("Join", [ax, row, r], dt, rows)
        full0 = emit("CumOp", [cat], dt, rows, {"axis": 0, "mode": "add"})
        # the caller's buffer holds `store` rows.  store <= T + 1 (the usual case, and what
        # Scan's memory-saving rewrites produce): the LAST `store` rows.  store > T + 1
        # (truncated BPTT): rows beyond T stay zero, scan/op.py:2139-2144.
        n1 = emit("Shape_i", [full0], "int64", [], {"i": 0})
        store = emit("Shape_i", [init_buf], "int64", [], {"i": 0})
        start = emit("Elemwise", [n1, store], "int64", [], _host_int("sub", clamp=True))
        npad = emit("Elemwise", [store, n1], "int64", [], _host_int("sub", clamp=True))
        wdims = [emit("Shape_i", [init_buf], "int64", [], {"i": d_}) for d_ in range(1, len(width) + 1)]
        tail = plan.new_var(dt, rows)                                   # (before its fill constant)
        out.append(Node("Alloc", [plan.add_const(0, dt), npad] + wdims, [tail], {}))
        full = emit("Join", [ax, full0, tail], dt, rows)
        replaced[old] = emit("Subtensor", [full, start], dt, V[old].shape, {"idx_list": [{"slice": ["in", None, None]}]})
    return out


def push_out_accumulators(plan: Plan) -> Plan:
    """A gradient Scan sums what it computes for every step into sit-sot accumulators —
    ``acc_t = acc_{t-1} + g_t`` for the gradient of a non-sequence such as a bias, with
    ``g_t = sum(delta_t, axis=0)`` for a batch (Scan.L_op, scan/op.py:2379) — although ``delta_t`` is
    a nit-sot output of the same Scan anyway (the weight gradients are GEMMs over it after the loop).
    Such an accumulator is taken out of the loop: its whole buffer is rebuilt after the Scan as
    ``cumsum([init; reduce(delta_1); ...; reduce(delta_T)])`` (the loop's additions, associated as
    the CumOp kernel associates long columns — equal up to float reordering; one CAReduce + one CumOp
    over [T + 1, H]), cut — or, for a buffer longer than T + 1, zero-padded like the reference's
    scan/op.py:2139 — to the buffer length the caller allocated, so every use of the old output —
    whatever row it reads — sees the same values.  The step loses its batch reduction, which is
    what kept batched recurrences with biases off the persistent gradient kernel."""
    return _rewrite_scans(plan, _accumulators_out)


def zero_filled_vars(plan: Plan) -> set:
    """Variables of ``plan`` that are ``Alloc`` of a constant 0 (``zeros_like`` of the front end)."""
    return {n_.outputs[0] for n_ in plan.nodes if n_.op == "Alloc" and _cfloat(plan, n_.inputs[0]) == 0.0}


def read_last_row_only(plan: Plan) -> set:
    """Variables of ``plan`` whose every use is ``v[-1]`` (what the caller of a Scan accumulator reads)."""
    uses = {}
    for n_ in plan.nodes:
        for k, i in enumerate(n_.inputs):
            uses.setdefault(i, []).append(n_.op == "Subtensor" and k == 0 and n_.params.get("idx_list") == [{"index": -1}])
    return {v for v, u in uses.items() if all(u) and v not in plan.outputs}


def _match_product_accumulators(plan, node, L, iprod, iclients, inner_zero, last_set, any_length, two_rows):
    """[(q, alpha, "gemm" | "ger" | "scatter" | "scatter1", a var, b var)]: the one-tap sit-sots q of
    the Scan that accumulate a product / scatter rows.  ``any_length``: the buffer need not be
    statically one row long; ``two_rows``: a scatter accumulator may be read beyond its last row."""
    inner, V = L.inner, plan.vars
    ss = node.params["sit_sot_in_slices"]

    def is_acc(v, tq_):
        """v is the accumulator tap itself, or ``tap + zeros`` (what the gradient of a lookup
        leaves: acc + inc_subtensor(zeros[i], g) rewritten to inc_subtensor((acc + zeros)[i], g))"""
        if v == tq_:
            return True
        pn_ = iprod.get(v)
        if pn_ is None or pn_.op != "Elemwise" or len(pn_.inputs) != 2 or len(iclients[v]) != 1:
            return False
        return (tq_ in pn_.inputs and any(i in inner_zero for i in pn_.inputs) and _is_add(pn_.params["scalar"])
                and inner.vars[v].shape == inner.vars[tq_].shape)
    found = []
    for q in range(L.n_ss):
        if list(ss[q]) != [-1]:
            continue
        tq, oq = inner.inputs[L.iin_tap(q)], inner.outputs[L.iout_ss(q)]
        upd = iprod.get(oq)
        scatter = upd is not None and upd.op in ("IncSubtensor", "AdvancedIncSubtensor1")
        if upd is None or len(iclients[tq]) != 1 or len(iclients[oq]) != 1 or \
                inner.vars[oq].dtype not in ("float32", "float64"):
            continue
        if scatter and node.outputs[L.out_ss(q)] not in last_set and not two_rows:
            continue          # (a scatter accumulator: only its LAST row may be read, or — decided by
            #                    the caller at run time — the buffer holds at most two rows)
        if not scatter and not any_length and V[node.inputs[L.in_init(q)]].shape[0] != 1:
            continue
        alpha = _cfloat(inner, upd.inputs[1]) if upd.op in ("Gemm", "Ger") else None
        if upd.op == "Gemm" and upd.inputs[0] == tq and alpha is not None and \
                _cfloat(inner, upd.inputs[4]) == 1.0 and tq not in upd.inputs[1:]:
            found.append((q, alpha, "gemm", upd.inputs[2], upd.inputs[3]))
        elif upd.op == "Ger" and upd.inputs[0] == tq and alpha is not None and tq not in upd.inputs[1:]:
            found.append((q, alpha, "ger", upd.inputs[2], upd.inputs[3]))
        elif upd.op == "IncSubtensor" and is_acc(upd.inputs[0], tq) and not upd.params["set_instead_of_inc"] and \
                upd.params["idx_list"] == [{"index": "in"}] and len(upd.inputs) == 3 and tq not in upd.inputs[1:] \
                and inner.vars[upd.inputs[1]].ndim == inner.vars[tq].ndim - 1:
            # acc[i_t] += v_t (the gradient of a table whose rows the step looks up itself,
            # subtensor.py:1419 IncSubtensor): acc_T = acc_0 with rows v_1 .. v_T added at i_1 .. i_T
            found.append((q, 1.0, "scatter", upd.inputs[1], upd.inputs[2]))
        elif upd.op == "AdvancedIncSubtensor1" and is_acc(upd.inputs[0], tq) and not upd.params["set_instead_of_inc"] \
                and tq not in upd.inputs[1:] and inner.vars[upd.inputs[2]].ndim == 1 and \
                inner.vars[upd.inputs[1]].ndim == inner.vars[tq].ndim:
            found.append((q, 1.0, "scatter1", upd.inputs[1], upd.inputs[2]))
    return found


def _rows_of(v, L: ScanSlots, emit: _Emit, iprod, nits: dict, need_equal):
    """Outer variable holding [T, ...] = the value of inner variable v at every step (None: not a
    per-step value we can take out): rows 0 .. n_steps - 1 of a sequence the Scan receives, a
    nit-sot output it already has, or one more nit-sot output of n_steps rows (``nits``: inner
    variable -> outer variable of those handed out additionally)."""
    node, inner = L.node, L.inner
    n_steps_v, rows = node.inputs[0], [None] + list(inner.vars[v].shape)
    pn = iprod.get(v)
    if pn is not None and pn.op in ("ScalarFromTensor", "TensorFromScalar"):
        return _rows_of(pn.inputs[0], L, emit, iprod, nits, need_equal)
    if pn is not None and pn.op == "DimShuffle":
        r = _rows_of(pn.inputs[0], L, emit, iprod, nits, need_equal)
        if r is None:
            return None
        order = [0] + [(o if o == "x" else o + 1) for o in pn.params["new_order"]]
        return emit("DimShuffle", [r], inner.vars[v].dtype, rows, {"new_order": order})
    if v in inner.inputs:
        k = inner.inputs.index(v)
        if k >= L.n_seqs:
            return None        # a tap or an invariant: not a stack of per-step rows
        return emit("Subtensor", [node.inputs[L.in_seq(k)], n_steps_v], inner.vars[v].dtype, rows,
                    {"idx_list": [{"slice": [None, "in", None]}]})
    if pn is None:
        return None            # a constant

    def whole(j_):             # nit-sot j_ must keep all n_steps rows
        len_v = node.inputs[L.in_nit_len(j_)]
        if len_v != n_steps_v:
            need_equal.append((len_v, n_steps_v))
        return node.outputs[L.out_nit(j_)]
    nits_ = [inner.outputs[L.iout_nit(j_)] for j_ in range(L.n_nit)]
    if v in nits_ and need_equal is not None:
        return whole(nits_.index(v))
    if need_equal is not None:
        # ... or handed out with broadcast axes added (a vector as a [1, n] row): the same rows
        for j_, o in enumerate(nits_):
            on = iprod.get(o)
            if on is not None and on.op == "DimShuffle" and on.inputs[0] == v and \
                    [d for d in on.params["new_order"] if d != "x"] == list(range(inner.vars[v].ndim)):
                keep = [0] + [1 + k for k, d in enumerate(on.params["new_order"]) if d != "x"]
                return emit("DimShuffle", [whole(j_)], inner.vars[v].dtype, rows, {"new_order": keep})
    if v not in nits:
        nits[v] = emit.plan.new_var(inner.vars[v].dtype, rows)
    return nits[v]


def _scatter_total(kind, ra, rb, old, init_buf, emit: _Emit, two_rows: bool, n_steps_v):
    """What replaces the accumulator output ``old``: acc_0 with the rows ``ra`` [T, ...] ([T, B, ...])
    added at the indices ``rb`` [T] ([T, B]) in step order, written into the caller's buffer
    ``init_buf`` — its last row, or ``two_rows``: a buffer of one or two rows, [acc_{T-1}, acc_T]."""
    plan = emit.plan
    V = plan.vars
    dt, out_shape, tail = V[old].dtype, V[old].shape, list(V[init_buf].shape[1:])
    neg = plan.add_const(-1, "int64")
    base = emit("Subtensor", [init_buf], dt, tail, {"idx_list": [{"index": 0}]})

    def scatter_sum(rv, iv):
        """acc_0 with the rows ``rv`` added at ``iv`` (in step order per destination row)"""
        if kind == "scatter1":
            dims = [neg] + [emit("Shape_i", [init_buf], "int64", [], {"i": d_ + 2}) for d_ in range(V[init_buf].ndim - 2)]
            sv = emit("MakeVector", dims, "int64", [len(dims)], {"dtype": "int64"})
            si = emit("MakeVector", [neg], "int64", [1], {"dtype": "int64"})
            rv = emit("Reshape", [rv, sv], dt, [None] * len(dims), {"ndim": len(dims)})
            iv = emit("Reshape", [iv, si], V[rb].dtype, [None], {"ndim": 1})
        return emit("AdvancedIncSubtensor1", [base, rv, iv], dt, tail, {"set_instead_of_inc": False, "inplace": False})
    summed = scatter_sum(ra, rb)
    if not two_rows:
        # the buffer the caller allocated, its last row = the final sum
        return emit("IncSubtensor", [init_buf, summed], dt, out_shape,
                    {"idx_list": [{"index": -1}], "set_instead_of_inc": True, "inplace": False})
    # a buffer of TWO rows keeps [acc_{T-1}, acc_T] (chronological, scan/op.py:2105): the row
    # before the last is the same sum over the first T - 1 steps
    tm1 = plan.new_var("int64", [])                                     # (before the constant 1)
    emit.sink.append(Node("Elemwise", [n_steps_v, plan.add_const(1, "int64")], [tm1], _host_int("sub")))
    cut = [emit("Subtensor", [v_, tm1], V[v_].dtype, V[v_].shape, {"idx_list": [{"slice": [None, "in", None]}]})
           for v_ in (ra, rb)]
    prev = scatter_sum(*cut)
    # [acc_{T-1}; acc_T] written once, cut to the caller's one or two rows (a view): the
    # sums of a large table are not copied through the buffer twice
    both = [emit("DimShuffle", [v_], dt, [1] + tail, {"new_order": ["x"] + list(range(len(tail)))})
            for v_ in (prev, summed)]
    two = plan.new_var(dt, [2] + tail)                                  # (before the axis constant)
    emit.sink.append(Node("Join", [plan.add_const(0, "int64")] + both, [two], {}))
    s_ = emit("Shape_i", [init_buf], "int64", [], {"i": 0})
    ms_ = emit("Elemwise", [s_], "int64", [], _host_int("neg", 1))
    return emit("Subtensor", [two, ms_], dt, out_shape, {"idx_list": [{"slice": ["in", None, None]}]})


def _stacked_product(kind, alpha, ra, rb, old, init_buf, emit: _Emit):
    """What replaces the accumulator output ``old``: ``acc_0 + alpha * sum_t A_t @ B_t`` ("gemm") or
    ``.. outer(x_t, y_t)`` ("ger") as ONE product over the stacked per-step operands ``ra`` / ``rb``"""
    dt, out_shape = emit.plan.vars[old].dtype, emit.plan.vars[old].shape
    if kind == "gemm":
        # sum_t A_t[m, k] @ B_t[k, n] = [m, T*k] @ [T*k, n]
        at_ = emit("DimShuffle", [ra], dt, [None, None, None], {"new_order": [1, 0, 2]})
        m_ = emit("Shape_i", [init_buf], "int64", [], {"i": 1})
        n_ = emit("Shape_i", [init_buf], "int64", [], {"i": 2})
        neg = emit.plan.add_const(-1, "int64")
        sa = emit("MakeVector", [m_, neg], "int64", [2], {"dtype": "int64"})
        sb = emit("MakeVector", [neg, n_], "int64", [2], {"dtype": "int64"})
        a2 = emit("Reshape", [at_, sa], dt, [None, None], {"ndim": 2})
        b2 = emit("Reshape", [rb, sb], dt, [None, None], {"ndim": 2})
    else:
        # sum_t outer(x_t, y_t) = X[T, m]^T @ Y[T, n]
        a2, b2 = emit("DimShuffle", [ra], dt, [None, None], {"new_order": [1, 0]}), rb
    prod = emit("Dot22", [a2, b2], dt, [None, None])
    prod3 = emit("DimShuffle", [prod], dt, [1, None, None], {"new_order": ["x", 0, 1]})
    sc = {"n_in": 2, "nodes": [{"op": "mul", "in": [["c", alpha, dt], ["i", 1]], "dtype": dt},
                               {"op": "add", "in": [["i", 0], ["t", 0]], "dtype": dt}],
          "out": [["t", 1]]}
    return emit("Elemwise", [init_buf, prod3], dt, out_shape, {"scalar": sc})


def _product_accumulators_out(plan, node, L, replaced, need_one_row, need_equal, zeros, last_only, need_le2):
    """:func:`push_out_product_accumulators` for one Scan node"""
    p, inner = node.params, L.inner
    if not p.get("sit_sot_in_slices"):
        return None
    iprod, iclients = inner.producers(), inner.clients()
    zero_set = zero_filled_vars(plan) if zeros is None else zeros
    last_set = read_last_row_only(plan) if last_only is None else last_only
    inner_zero = {iv for iv, ov in zip(inner.inputs[L.iin_inv0:], node.inputs[L.in_non0:])
                  if ov in zero_set} if L.n_non else set()
    found = _match_product_accumulators(plan, node, L, iprod, iclients, inner_zero, last_set,
                                        need_one_row is not None, need_le2 is not None)
    # where the per-step operands come from: a sequence the Scan receives (rows 0 .. n_steps - 1
    # of it), or a value of the step, handed out as one more nit-sot output of n_steps rows
    post, nits, done = [], {}, []      # nodes behind the Scan; inner var -> outer var of a new nit-sot
    emit = _Emit(plan, post)
    for q, alpha, kind, a, b in found:
        mark = (len(post), dict(nits))
        ra, rb = (_rows_of(v, L, emit, iprod, nits, need_equal) for v in (a, b))
        if ra is None or rb is None:
            del post[mark[0]:]
            nits.clear()
            nits.update(mark[1])
            continue
        old, init_buf = node.outputs[L.out_ss(q)], node.inputs[L.in_init(q)]
        if kind in ("scatter", "scatter1"):
            # (read beyond its last row: the matching lets that through only with ``need_le2``, where
            # the caller decides at run time whether the buffer holds at most two rows)
            two_rows = old not in last_set
            replaced[old] = _scatter_total(kind, ra, rb, old, init_buf, emit, two_rows, node.inputs[0])
            if two_rows:
                need_le2.append(init_buf)
        else:
            replaced[old] = _stacked_product(kind, alpha, ra, rb, old, init_buf, emit)
            if need_one_row is not None:
                need_one_row.append(init_buf)
        done.append(q)
    if not done:
        return None
    dq = set(done)
    # the additional nit-sot outputs: behind the existing ones (inner outputs, Scan outputs) and
    # their lengths behind the existing lengths (Scan inputs: ..., shared, nit-sot lengths, non-seqs)
    new_inputs, new_outputs, in_keep, out_keep = L.insert_nit_sots(
        L.drop_sit_sots(dq), None, [node.inputs[0]] * len(nits), nits.values(), nits, n_dropped=len(dq))
    gone = {id(iprod[inner.outputs[L.iout_ss(q)]]) for q in dq}        # the accumulating products themselves
    new_inner = Plan(inner.name + "_noprod", inner.vars, in_keep, out_keep,
                     [n_ for n_ in inner.nodes if id(n_) not in gone])
    new_inner.nodes = _prune_dead(new_inner, list(new_inner.nodes))
    p = dict(p, inner=new_inner, sit_sot_in_slices=[list(t) for q, t in enumerate(p["sit_sot_in_slices"]) if q not in dq],
             n_nit_sot=L.n_nit + len(nits))
    # (every output was an accumulator over sequence rows: no loop is left)
    return ([Node("Scan", new_inputs, new_outputs, p)] if new_outputs else []) + post


def push_out_product_accumulators(plan: Plan, need_one_row: list = None, need_equal: list = None,
                                  zeros: set = None, last_only: set = None, need_le2: list = None) -> Plan:
    """The weight gradient a gradient Scan accumulates IN the loop — ``acc_t = acc_{t-1} + a_t^T @ g_t``
    (``Gemm(acc, alpha, A_t, B_t, 1)``; for a vector state the outer product ``Ger(acc, alpha, x_t,
    y_t)``) in a sit-sot output — is what the reference's ``PushOutDot1`` (scan/rewriting.py) turns
    into ONE product over the stacked operands behind the loop.  That rewrite matches the gradient
    of a one-tap recurrence; for taps [-1, -2] (mit-mot [0, 2, 1] -> [2, 1]) it leaves T small
    products inside the step, which also keeps the step off the persistent kernels.  Done here for
    every such accumulator whose buffer holds ONE row (only the final sum is kept: what Scan's
    memory-saving rewrite leaves when the caller reads ``acc[-1]``):
    ``acc_T = acc_0 + alpha * sum_t A_t @ B_t = acc_0 + alpha * [A_1 .. A_T] @ [B_1; ..; B_T]``,
    the per-step operands taken from the sequences the Scan already receives or handed out as one
    more nit-sot output.  Same sum in another association (one long-K GEMM): equal to the loop's up
    to float reordering, like PushOutDot1's.  A scatter accumulator ``acc[i_t] += v_t`` becomes one
    scatter-add of all rows the same way.

    The buffer length is rarely static (``Alloc`` of a shape expression): with ``need_one_row`` (a
    list) the static test is skipped and the variables that must turn out to hold one row are
    appended to it — ``ScanMixin._op_Scan`` applies the rewrite to the single Scan node at hand
    and runs the rewritten form when the buffers it is handed have one row (``need_le2``: at most
    two rows, for a scatter accumulator that is not only read at its last row).  ``need_equal``
    collects pairs of host integers that must be equal then: a per-step operand that already IS a
    nit-sot output is taken from there when that output keeps all ``n_steps`` rows."""
    return _rewrite_scans(plan, lambda *at: _product_accumulators_out(
        *at, need_one_row, need_equal, zeros, last_only, need_le2))


def merge_shared_left_dots(plan: Plan) -> Plan:
    """Several ``Dot22(x, W_k)`` with the SAME left operand and plan-input right operands (the
    ``x_t @ W_gate`` products of every gate, lifted over a whole sequence: ``[T*B, K] @ [K, H]``
    three times) become ONE product against the weights side by side —
    ``P = Dot22(x, Join(1, W_1, .., W_G))``, each result a column view ``P[:, c_{k-1}:c_k]`` (no
    copies of P; the 12 MiB of weights are joined once per call).  A wider N keeps more of the chip
    busy per tile wave and saves G - 1 launch boundaries.  Returns the plan unchanged when no group
    of >= 2 such products exists."""
    groups: Dict[int, list] = {}
    ins = set(plan.inputs)
    for ni, n in enumerate(plan.nodes):
        if n.op == "Dot22" and n.inputs[1] in ins and plan.vars[n.inputs[1]].ndim == 2:
            groups.setdefault(n.inputs[0], []).append(ni)
    groups = {x: g for x, g in groups.items() if len(g) >= 2 and
              len({plan.vars[plan.nodes[ni].inputs[1]].dtype for ni in g}) == 1}
    if not groups:
        return plan
    work = plan.copy(plan.name + "_wide", nodes=[])
    drop, emitted_at = set(), {}
    for x, g in groups.items():
        first = min(g)
        dt = work.vars[plan.nodes[first].outputs[0]].dtype
        Ws = [plan.nodes[ni].inputs[1] for ni in g]
        new = emitted_at[first] = []
        emit = _Emit(work, new)
        wcat = work.new_var(dt, [None, None])                           # (before the axis constant)
        new.append(Node("Join", [work.add_const(1, "int8")] + Ws, [wcat], {}))
        P = emit("Dot22", [x, wcat], dt, [None, None])
        lo = None
        for k, ni in enumerate(g):
            nk = emit("Shape_i", [Ws[k]], "int64", [], {"i": 1})
            hi = nk if lo is None else emit("Elemwise", [lo, nk], "int64", [], _host_int("add"))
            idx = [{"slice": [None, None, None]}, {"slice": [None if lo is None else "in", "in", None]}]
            new.append(Node("Subtensor", [P] + ([] if lo is None else [lo]) + [hi], [plan.nodes[ni].outputs[0]],
                            {"idx_list": idx}))
            lo = hi
            drop.add(ni)
    for ni, n in enumerate(plan.nodes):
        work.nodes.extend(emitted_at.get(ni, []))
        if ni not in drop:
            work.nodes.append(n)
    return work


def _match_assembled(L: ScanSlots, iprod, icl, inv):
    """(j, X, view, parts, product node, ndim) of the first nit-sot j of the Scan that is an
    assembly ``X`` of column blocks ``parts`` = [(a, b, value)] read by exactly one product"""
    inner = L.inner
    for j in range(L.n_nit):
        o = inner.outputs[L.iout_nit(j)]
        X, view = o, None
        if o in iprod and iprod[o].op == "DimShuffle" and \
                [d for d in iprod[o].params["new_order"] if d != "x"] == list(range(inner.vars[iprod[o].inputs[0]].ndim)):
            X, view = iprod[o].inputs[0], iprod[o]       # handed out with broadcast axes added
        nd = inner.vars[X].ndim
        if nd not in (1, 2) or inner.outputs.count(o) != 1 or (view is not None and len(icl[o]) != 1):
            continue
        parts, v = [], X
        while v in iprod and iprod[v].op == "IncSubtensor":
            n_ = iprod[v]
            idx = n_.params["idx_list"]
            if len(idx) != nd or any("slice" not in e for e in idx) or \
                    (nd == 2 and idx[0]["slice"] != [None, None, None]) or idx[-1]["slice"][2] not in (None, 1):
                parts = None
                break
            extra, ab = list(n_.inputs[2:]), []
            for e in idx[-1]["slice"][:2]:
                ab.append(_cint(inner, extra.pop(0)) if e == "in" and extra else (e if isinstance(e, int) else None))
            if None in ab or extra:
                parts = None
                break
            parts.append((ab[0], ab[1], n_.inputs[1]))
            v = n_.inputs[0]
            if len(icl[v]) != 1:
                parts = None
                break
        if not parts or v not in iprod or iprod[v].op != "Alloc":
            continue
        fill = inner.vars[iprod[v].inputs[0]]
        if fill.const is None or any(float(d) != 0.0 for d in fill.const.get("data", [1])):
            continue
        parts.sort()
        if parts[0][0] != 0 or any(parts[k][1] != parts[k + 1][0] for k in range(len(parts) - 1)):
            continue
        # X is read by exactly two things: the product and the output (or the view handed out)
        uses = [c for c in icl[X] if c[0] != "out" and inner.nodes[c[0]] is not view]
        if len(uses) != 1 or len(icl[X]) != 2:
            continue
        un = inner.nodes[uses[0][0]]
        if not ((nd == 2 and un.op == "Gemm" and uses[0][1] == 2 and un.inputs[3] in inv) or
                (nd == 1 and un.op == "Gemv" and uses[0][1] == 3 and un.inputs[2] in inv)):
            continue
        return j, X, view, parts, un, nd
    return None


def _assembled_columns_out(plan: Plan, node: Node, L: ScanSlots, replaced: dict):
    """:func:`split_assembled_columns` for one Scan node"""
    inner = L.inner
    if not L.n_nit:
        return None
    inv = set(inner.inputs[L.iin_inv0:])
    for n_ in inner.nodes:
        if n_.op in ("DimShuffle", "ViewOp") and all(i in inv for i in n_.inputs):
            inv.update(n_.outputs)
    found = _match_assembled(L, inner.producers(), inner.clients(), inv)
    if found is None:
        return None
    j, X, view, parts, un, nd = found
    work = inner.copy(inner.name + "_blocks", nodes=[])
    if nd == 2:
        z, al, _x, W, be = un.inputs
    else:
        z, al, W, _x, be = un.inputs
    one = work.add_const(1.0, inner.vars[al].dtype)
    nodes = []
    emit = _Emit(work, nodes)
    for n_ in inner.nodes:
        if n_ is not un:
            nodes.append(n_)
            continue
        acc, wv = z, inner.vars[W]
        for k, (a, b, pk) in enumerate(parts):
            if nd == 2:      # rows a:b of W
                wk = emit("Subtensor", [W], wv.dtype, [None, wv.shape[1]], {"idx_list": [{"slice": [a, b, None]}]})
            else:            # columns a:b of A
                wk = emit("Subtensor", [W], wv.dtype, [wv.shape[0], None],
                          {"idx_list": [{"slice": [None, None, None]}, {"slice": [a, b, None]}]})
            out = un.outputs[0] if k == len(parts) - 1 else \
                work.new_var(inner.vars[un.outputs[0]].dtype, list(inner.vars[un.outputs[0]].shape))
            ins_ = [acc, al, pk, wk, be if k == 0 else one] if nd == 2 else \
                [acc, al, wk, pk, be if k == 0 else one]
            nodes.append(Node(un.op, ins_, [out], dict(un.params)))
            acc = out
    old = node.outputs[L.out_nit(j)]
    ov = plan.vars[old]
    pshape = [None] + list(inner.vars[X].shape[:-1]) + [None]               # [T, (B,) width]
    pouts = [plan.new_var(ov.dtype, pshape) for _ in parts]
    new_inputs, new_outputs, _iins, work.outputs = L.insert_nit_sots(
        [list(node.inputs), list(node.outputs), inner.inputs, list(inner.outputs)], j,
        [node.inputs[L.in_nit_len(j)]] * len(parts), pouts, [pk for _a, _b, pk in parts], n_old=1)
    work.nodes = _prune_dead(work, nodes)
    out = [Node("Scan", new_inputs, new_outputs, dict(node.params, inner=work, n_nit_sot=L.n_nit + len(parts) - 1))]
    emit = _Emit(plan, out)
    ax = plan.add_const(nd, "int8")
    if view is None:
        whole = emit("Join", [ax] + pouts, ov.dtype, ov.shape)
    else:
        wide = emit("Join", [ax] + pouts, ov.dtype, pshape)
        order = [0] + [d if d == "x" else d + 1 for d in view.params["new_order"]]
        whole = emit("DimShuffle", [wide], ov.dtype, ov.shape, {"new_order": order})
    replaced[old] = whole
    return out


def split_assembled_columns(plan: Plan) -> Plan:
    """The gradient step of a fused-gate recurrence assembles the gate gradients into ONE wide
    value — ``X = zeros(B, 4H); X[:, 0:H] = p_i; X[:, H:2H] = p_f; ...`` (a vector of length 4H for
    a vector state) — only to multiply it with the (transposed) fused weight matrix and to hand it
    out as a nit-sot output.  The product is a sum over the blocks, ``z + X @ W = z + sum_k p_k @
    W[a_k:b_k, :]`` (``z + A x = z + sum_k A[:, a_k:b_k] p_k`` for a Gemv), and the output is the
    blocks side by side, so the assembly leaves the step: the Scan returns the blocks as separate
    nit-sot outputs (H-wide, what the persistent kernels write) and ONE ``Join`` after the loop
    rebuilds the wide array for the weight-gradient GEMMs."""
    return _rewrite_scans(plan, _assembled_columns_out)


def _hoist_sequence_only_stacked(plan: Plan, seq_inputs: List[int], invariant: set):
    """The matrix-state class of :func:`hoist_sequence_only` (a batch of recurrences: per-step
    values are ``[B, n]`` matrices).  The steps are stacked along the rows — a sequence ``[T, B, n]``
    is read as ``[T * B, n]`` — so the hoisted nodes run unchanged on the stacked operands:
    ``Elemwise`` (invariant operands must broadcast along the rows: static leading extent 1),
    ``Dot22`` / ``Dot22Scalar`` / ``Gemm`` with an invariant right-hand matrix.  ``lifted["stacked"]``
    tells the executor to fold / unfold the two leading axes."""
    V = plan.vars
    floats = ("float32", "float64")

    Q = {v for v in seq_inputs if V[v].ndim == 2 and V[v].dtype in floats}
    seq_set = set(seq_inputs)
    hoisted, keep = [], []
    for n in plan.nodes:
        ok = False
        if n.op == "Elemwise" and n.inputs and any(i in Q for i in n.inputs):
            ok = all(i in Q or ((i in invariant or V[i].const is not None) and V[i].ndim == 2
                                and V[i].shape[0] == 1) for i in n.inputs) and \
                all(V[o].ndim == 2 and V[o].dtype in floats for o in n.outputs)
        elif n.op in ("Dot22", "Dot") and len(n.inputs) == 2:
            a, b = n.inputs
            ok = a in Q and b in invariant and V[b].ndim == 2 and V[n.outputs[0]].dtype in floats
        elif n.op == "Dot22Scalar":
            a, b, sc = n.inputs
            ok = a in Q and b in invariant and V[b].ndim == 2 and plan.const_scalar(sc) is not None
        elif n.op == "Gemm":
            z, al, a, b, be = n.inputs
            ok = z in Q and a in Q and b in invariant and V[b].ndim == 2 and \
                plan.const_scalar(al) is not None and plan.const_scalar(be) is not None
        if ok:
            hoisted.append(n)
            Q.update(n.outputs)
        else:
            keep.append(n)
    used_later = {i for n in keep for i in n.inputs} | set(plan.outputs)
    outs = [o for n in hoisted for o in n.outputs if o in used_later]
    if not outs:
        return plan, None
    need, live = set(outs), []
    for n in reversed(hoisted):
        if any(o in need for o in n.outputs):
            live.append(n)
            need.update(n.inputs)
    live.reverse()
    live_ids = {id(n) for n in live}
    keep = _prune_dead(plan, [n for n in plan.nodes if id(n) not in live_ids])
    lp = Plan(plan.name + "_allsteps", {}, [], [], [])
    m, seq_in, inv_in = {}, [], []

    def var(v):
        if v not in m:
            src = V[v]
            m[v] = lp.new_var(src.dtype, list(src.shape), src.name, src.const)
            if src.const is None:
                if v in seq_set:
                    seq_in.append(v)
                elif v in invariant:
                    inv_in.append(v)
        return m[v]

    for n in live:
        lp.nodes.append(Node("Dot22" if n.op == "Dot" else n.op, [var(i) for i in n.inputs],
                             [var(o) for o in n.outputs], dict(n.params)))
    lp.inputs = [m[v] for v in seq_in] + [m[v] for v in inv_in]
    lp.outputs = [m[o] for o in outs]
    loop = Plan(plan.name + "_seqonly", plan.vars, list(plan.inputs) + outs, list(plan.outputs), keep)
    return loop, {"plan": lp, "seq_in": seq_in, "inv_in": inv_in, "outs": outs, "stacked": True}


def hoist_sequence_only(plan: Plan, seq_inputs: List[int], invariant: set):
    """Everything in a Scan step that depends only on *sequence* rows and loop invariants does not
    take part in the recurrence: it is computed for ALL steps before the loop and the step reads
    row t of the result.  Covers the vector class: ``Elemwise`` on per-step vectors and ``Gemv``
    chains with invariant matrices (``W1 x_t + W2 h_t`` of a gate — a gradient Scan recomputes the
    forward gates from stored states this way, scan/op.py:2379 ``Scan.L_op``); the lifted plan runs
    them as ``[T, n]`` Elemwise kernels and GEMMs (T x K @ K x M fills the chip; T separate GEMVs
    cannot).  The reference's ``scan_pushout_seqs_ops`` (scan/rewriting.py) has the same aim but
    leaves the dots, and whatever depends on them, inside.

    Returns ``(loop_plan, lifted)``; ``lifted`` = None or ``{"plan": Plan over whole sequences,
    "seq_in": step-plan ids of the sequences it reads, "inv_in": ids of the invariants it reads,
    "outs": step-plan ids of its results (appended to the loop plan's inputs, in this order)}``."""
    V = plan.vars
    floats = ("float32", "float64")

    Q = {v for v in seq_inputs if V[v].ndim == 1 and V[v].dtype in floats}
    seq_set = set(seq_inputs)
    if not Q and any(V[v].ndim == 2 and V[v].dtype in floats for v in seq_inputs):
        return _hoist_sequence_only_stacked(plan, seq_inputs, invariant)
    hoisted, keep = [], []
    for n in plan.nodes:
        ok = False
        if n.op == "Elemwise" and n.inputs and any(i in Q for i in n.inputs):
            ok = all(i in Q or ((i in invariant or V[i].const is not None) and V[i].ndim == 1)
                     for i in n.inputs) and \
                all(V[o].ndim == 1 and V[o].dtype in floats for o in n.outputs)
        elif n.op == "Gemv":
            y, alpha, A, x, beta = n.inputs
            ok = A in invariant and V[A].ndim == 2 and x in Q and _cfloat(plan, alpha) is not None and \
                _cfloat(plan, beta) is not None and (_cfloat(plan, beta) == 0.0 or y in Q) and \
                V[n.outputs[0]].dtype in floats
        if ok:
            hoisted.append(n)
            Q.update(n.outputs)
        else:
            keep.append(n)
    used_later = {i for n in keep for i in n.inputs} | set(plan.outputs)
    outs = [o for n in hoisted for o in n.outputs if o in used_later]
    if not outs:
        return plan, None
    # keep only the hoisted nodes the results depend on
    need, live = set(outs), []
    for n in reversed(hoisted):
        if any(o in need for o in n.outputs):
            live.append(n)
            need.update(n.inputs)
    live.reverse()
    dropped = [n for n in hoisted if n not in live]
    if dropped:        # (they fed nothing that is kept: leave them where they were)
        live_ids = {id(n) for n in live}
        keep = [n for n in plan.nodes if id(n) not in live_ids]

    # what only fed the hoisted nodes (the AllocEmpty "y" of a beta = 0 Gemv and its shape
    # arithmetic) is dead in the loop now
    keep = _prune_dead(plan, keep)

    lp = Plan(plan.name + "_allsteps", {}, [], [], [])
    m, seq_in, inv_in = {}, [], []

    def same(v):                      # invariant / constant operand: the same variable
        if ("s", v) not in m:
            src = V[v]
            m[("s", v)] = lp.new_var(src.dtype, list(src.shape), src.name, src.const)
            if src.const is None:
                inv_in.append(v)
        return m[("s", v)]

    def rows(v):                      # per-step vector -> [T, n]
        if ("r", v) not in m:
            m[("r", v)] = lp.new_var(V[v].dtype, [None, V[v].shape[0]])
            if v in seq_set:
                seq_in.append(v)
        return m[("r", v)]

    def as_row(v):                    # invariant vector next to [T, n] operands: [1, n]
        if ("b", v) not in m:
            src = V[v]
            if src.const is not None:
                c = dict(src.const)
                c["shape"] = [1] + list(c["shape"])
                m[("b", v)] = lp.new_var(src.dtype, [1] + list(src.shape), None, c)
            else:
                o = lp.new_var(src.dtype, [1] + list(src.shape))
                lp.nodes.append(Node("DimShuffle", [same(v)], [o], {"new_order": ["x", 0]}))
                m[("b", v)] = o
        return m[("b", v)]

    for n in live:
        if n.op == "Elemwise":
            ins = [rows(i) if i in Q else as_row(i) for i in n.inputs]
            lp.nodes.append(Node("Elemwise", ins, [rows(o) for o in n.outputs], dict(n.params)))
        else:
            y, alpha, A, x, beta = n.inputs
            at_ = lp.new_var(V[A].dtype, [V[A].shape[1], V[A].shape[0]])
            lp.nodes.append(Node("DimShuffle", [same(A)], [at_], {"new_order": [1, 0]}))
            if _cfloat(plan, beta) == 0.0:
                lp.nodes.append(Node("Dot22Scalar", [rows(x), at_, same(alpha)], [rows(n.outputs[0])], {}))
            else:
                lp.nodes.append(Node("Gemm", [rows(y), same(alpha), rows(x), at_, same(beta)],
                                     [rows(n.outputs[0])], {"inplace": False}))
    lp.inputs = [m[("r", v)] for v in seq_in] + [m[("s", v)] for v in inv_in]
    lp.outputs = [m[("r", o)] for o in outs]
    loop = Plan(plan.name + "_seqonly", plan.vars, list(plan.inputs) + outs, list(plan.outputs), keep)
    return loop, {"plan": lp, "seq_in": seq_in, "inv_in": inv_in, "outs": outs}


_BATCH_ALIAS = ("ScalarFromTensor", "TensorFromScalar", "ViewOp", "DeepCopyOp")


def batch_map_step(plan: Plan, n_seqs: int):
    """A Scan WITHOUT recurrence (nit-sot outputs only: ``aesara.map``, the row loops of
    ``gradient.jacobian`` / ``hessian`` and of ``Rop`` / ``Lop`` helpers — scan/basic.py:71 with no
    ``outputs_info``) evaluates the same function on every sequence row; no step reads what another
    step wrote (scan_perform.pyx:309-541 with n_mit_mot = n_mit_sot = n_sit_sot = 0), so the loop
    is not a loop: this returns the step plan restated over WHOLE sequences — every per-step
    value ``v[S]`` becomes ``V[T, S]``, invariants stay as they are — or None when a node has no
    such restatement here.  Rules (``step`` = depends on a sequence row):

    * 0-d glue (``ScalarFromTensor`` ...) : the same variable, now ``[T]``;
    * ``Elemwise``: step operands as they are, invariant operands with a leading broadcastable dim;
    * ``CAReduce`` / ``DimShuffle``: axes shifted by one; ``Shape_i`` of a step value: invariant;
    * ``Subtensor(M, i_t, ...)`` of an invariant by the step's index: ``AdvancedSubtensor1(M, i)``
      (the same bounds check and negative wrap, subtensor.py:756 / :2080), then the rest of the index;
      of a step value by invariant indices: one more leading slice;
    * ``AdvancedSubtensor1(M, idx_t)`` with the step's index vector: one gather over all T * B indices;
    * ``IncSubtensor(base, val, i_t)`` (the unit vectors of a Jacobian loop: ``set_subtensor(zeros[i], 1)``):
      ``base`` repeated T times, then ``B[arange(T), i] = val`` (``AdvancedIncSubtensor``; the (t, i_t)
      pairs are distinct); on a step value with invariant indices: one more leading slice;
    * ``Gemv(y, alpha, A, x_t, beta)`` with an invariant matrix: ``X @ A.T`` (``Dot22Scalar`` / ``Gemm``);
    * ``Alloc(v_t, *shape)`` / ``Reshape(v_t, shape)`` / ``SpecifyShape(v_t, *shape)`` with an invariant
      shape: the same node with T in front of the shape.

    Returns ``{"plan": Plan(inputs = sequences + the other step-plan inputs), "outs": n}``."""
    V = plan.vars
    seqs = list(plan.inputs[:n_seqs])
    if not seqs:
        return None
    bp = Plan(plan.name + "_allrows", {}, [], [], [])
    step, m = set(seqs), {}

    def nv(dtype, shape, const=None):
        return bp.new_var(dtype, list(shape), None, const)

    emit = _Emit(bp, bp.nodes)

    def get(v):
        if v not in m:
            src = V[v]
            m[v] = nv(src.dtype, ([None] + list(src.shape)) if v in step else src.shape, src.const)
        return m[v]

    def lead(v):
        """invariant ``v`` next to ``[T, ...]`` operands"""
        src = V[v]
        if src.const is not None and "data" in src.const:
            c = dict(src.const)
            c["shape"] = [1] + list(c["shape"])
            return nv(src.dtype, [1] + list(src.shape), c)
        return emit("DimShuffle", [get(v)], src.dtype, [1] + list(src.shape),
                    {"new_order": ["x"] + list(range(src.ndim))})

    def i64(x):
        return bp.add_const(np.asarray(x, dtype="int64"), "int64")

    for v in plan.inputs:
        get(v)
    bp.inputs = [m[v] for v in plan.inputs]
    tlen = [None]

    def T_():
        if tlen[0] is None:
            tlen[0] = emit("Shape_i", [m[seqs[0]]], "int64", [], {"i": 0})
        return tlen[0]

    def entries(idx_list, extra):
        """[(entry, its dynamic inputs)]"""
        extra, out = list(extra), []
        for e in idx_list:
            n_dyn = sum(1 for t in (e["slice"] if "slice" in e else [e["index"]]) if t == "in")
            out.append((e, extra[:n_dyn]))
            extra = extra[n_dyn:]
        return out

    full = {"slice": [None, None, None]}
    for n in plan.nodes:
        s_in = [i for i in n.inputs if i in step]
        if not s_in:
            if n.op == "Scan":
                return None
            bp.nodes.append(Node(n.op, [get(i) for i in n.inputs], [get(o) for o in n.outputs], dict(n.params)))
            continue
        o0 = n.outputs[0]
        if n.op in _BATCH_ALIAS and len(n.inputs) == 1:
            step.add(o0)
            m[o0] = get(n.inputs[0])
        elif n.op == "Elemwise":
            step.update(n.outputs)
            ins = [get(i) if i in step else lead(i) for i in n.inputs]
            bp.nodes.append(Node("Elemwise", ins, [get(o) for o in n.outputs], dict(n.params)))
        elif n.op == "CAReduce":
            nd = V[n.inputs[0]].ndim
            ax = n.params.get("axis")
            ax = list(range(nd)) if ax is None else [a % nd for a in ax]
            step.add(o0)
            bp.nodes.append(Node("CAReduce", [get(n.inputs[0])], [get(o0)],
                                 dict(n.params, axis=[a + 1 for a in ax])))
        elif n.op == "DimShuffle":
            step.add(o0)
            bp.nodes.append(Node("DimShuffle", [get(n.inputs[0])], [get(o0)],
                                 dict(n.params, new_order=[0] + [e if e == "x" else e + 1
                                                                 for e in n.params["new_order"]])))
        elif n.op == "Shape_i":
            bp.nodes.append(Node("Shape_i", [get(n.inputs[0])], [get(o0)], {"i": int(n.params["i"]) + 1}))
        elif n.op == "Subtensor":
            x, ents = n.inputs[0], entries(n.params["idx_list"], n.inputs[1:])
            if x in step:
                if any(d in step for _e, dyn in ents for d in dyn):
                    return None
                step.add(o0)
                bp.nodes.append(Node("Subtensor", [get(x)] + [get(d) for _e, dyn in ents for d in dyn],
                                     [get(o0)], {"idx_list": [full] + [e for e, _d in ents]}))
            else:
                e0, d0 = ents[0]
                if "index" not in e0 or len(d0) != 1 or d0[0] not in step or V[d0[0]].ndim != 0 or \
                        any(d in step for _e, dyn in ents[1:] for d in dyn):
                    return None
                step.add(o0)
                rows = emit("AdvancedSubtensor1", [get(x), get(d0[0])], V[x].dtype, [None] + list(V[x].shape[1:]))
                if len(ents) == 1:
                    m[o0] = rows
                else:
                    bp.nodes.append(Node("Subtensor", [rows] + [get(d) for _e, dyn in ents[1:] for d in dyn],
                                         [get(o0)], {"idx_list": [full] + [e for e, _d in ents[1:]]}))
        elif n.op == "AdvancedSubtensor1":
            x, iv = n.inputs
            if x in step or V[iv].ndim != 1:
                return None
            step.add(o0)
            # rows of an invariant table by the step's index VECTOR (an embedding lookup per batch
            # item): one gather over the T * B indices, unfolded to [T, B, ...]
            flat = emit("Reshape", [get(iv), emit("MakeVector", [i64(-1)], "int64", [1], {"dtype": "int64"})],
                        V[iv].dtype, [None], {"ndim": 1})
            rows = emit("AdvancedSubtensor1", [get(x), flat], V[x].dtype, [None] + list(V[x].shape[1:]))
            dims = [T_(), emit("Shape_i", [get(iv)], "int64", [], {"i": 1})] + \
                [emit("Shape_i", [get(x)], "int64", [], {"i": d}) for d in range(1, V[x].ndim)]
            shp = emit("MakeVector", dims, "int64", [len(dims)], {"dtype": "int64"})
            bp.nodes.append(Node("Reshape", [rows, shp], [get(o0)], {"ndim": len(dims)}))
        elif n.op == "IncSubtensor":
            x, y = n.inputs[:2]
            ents = entries(n.params["idx_list"], n.inputs[2:])
            dyn_step = [d for _e, dyn in ents for d in dyn if d in step]
            n_int = sum(1 for e, _d in ents if "index" in e)
            if y in step and V[y].ndim != V[x].ndim - n_int:
                return None          # (a value that broadcasts from the left would misalign under [T, ...])
            step.add(o0)
            if not dyn_step:
                if x not in step:
                    return None
                bp.nodes.append(Node("IncSubtensor", [get(x), get(y)] + [get(d) for _e, dyn in ents for d in dyn],
                                     [get(o0)], dict(n.params, idx_list=[full] + [e for e, _d in ents], inplace=False)))
            else:
                e0, d0 = ents[0]
                if len(ents) != 1 or "index" not in e0 or len(d0) != 1 or V[d0[0]].ndim != 0:
                    return None
                if x in step:
                    B = get(x)
                else:
                    dims = [T_()] + [emit("Shape_i", [get(x)], "int64", [], {"i": d}) for d in range(V[x].ndim)]
                    B = emit("Alloc", [lead(x)] + dims, V[x].dtype, [None] + list(V[x].shape))
                ar = emit("ARange", [i64(0), T_(), i64(1)], "int64", [None], {"dtype": "int64"})
                bp.nodes.append(Node("AdvancedIncSubtensor", [B, get(y), ar, get(d0[0])], [get(o0)],
                                     {"set_instead_of_inc": bool(n.params["set_instead_of_inc"]), "inplace": False}))
        elif n.op == "Gemv":
            y, alpha, A, x, beta = n.inputs
            beta0 = _cfloat(plan, beta) == 0.0
            if A in step or alpha in step or beta in step or x not in step or V[A].ndim != 2 or \
                    not (beta0 or y in step):
                return None
            step.add(o0)
            at_ = emit("DimShuffle", [get(A)], V[A].dtype, [V[A].shape[1], V[A].shape[0]], {"new_order": [1, 0]})
            if beta0:
                bp.nodes.append(Node("Dot22Scalar", [get(x), at_, get(alpha)], [get(o0)], {}))
            else:
                bp.nodes.append(Node("Gemm", [get(y), get(alpha), get(x), at_, get(beta)], [get(o0)],
                                     {"inplace": False}))
        elif n.op == "SpecifyShape":
            if any(i in step for i in n.inputs[1:]):
                return None
            step.add(o0)
            nd = V[n.inputs[0]].ndim
            bp.nodes.append(Node("SpecifyShape", [get(i) for i in n.inputs], [get(o0)],
                                 {"dims": [d + 1 for d in n.params.get("dims", range(len(n.inputs) - 1))],
                                  "ndim": int(n.params.get("ndim", nd)) + 1}))
        elif n.op == "Reshape":
            x, sv = n.inputs
            if sv in step or V[sv].dtype != "int64" or V[sv].ndim != 1:
                return None
            step.add(o0)
            t1 = emit("MakeVector", [T_()], "int64", [1], {"dtype": "int64"})
            k = V[sv].shape[0]
            shp = emit("Join", [i64(0), t1, get(sv)], "int64", [None if k is None else k + 1])
            bp.nodes.append(Node("Reshape", [get(x), shp], [get(o0)], {"ndim": int(n.params["ndim"]) + 1}))
        elif n.op == "Alloc":
            if any(i in step for i in n.inputs[1:]) or V[n.inputs[0]].ndim != V[o0].ndim:
                return None
            step.add(o0)
            bp.nodes.append(Node("Alloc", [get(n.inputs[0]), T_()] + [get(i) for i in n.inputs[1:]], [get(o0)],
                                 dict(n.params)))
        else:
            return None
    outs = []
    for o in plan.outputs:
        if o in step:
            outs.append(get(o))
        else:                              # the same value every step
            dims = [T_()] + [emit("Shape_i", [get(o)], "int64", [], {"i": d}) for d in range(V[o].ndim)]
            outs.append(emit("Alloc", [lead(o)] + dims, V[o].dtype, [None] + list(V[o].shape)))
    bp.outputs = outs
    return {"plan": bp, "outs": len(outs)}


_GLUE_TARGETS = ("Subtensor", "AdvancedSubtensor1", "IncSubtensor")


def _sequence_glue_out(plan: Plan, node: Node, L: ScanSlots, replaced: dict):
    """:func:`push_out_sequence_glue` for one Scan node"""
    p, inner, n_seqs = node.params, L.inner, L.n_seqs
    if not n_seqs or not (L.n_mm or L.n_ms or L.n_ss or L.n_sh):
        # (a Scan without recurrence is restated as a whole, in blocks of rows when its
        # intermediates are large: ScanMixin._scan_all_rows)
        return None
    V = inner.vars
    seq_vars, inv_vars = list(inner.inputs[:n_seqs]), list(inner.inputs[L.iin_inv0:])
    rec_inputs = set(inner.inputs[n_seqs:L.iin_inv0])
    prod = inner.producers()
    # 0: invariant / constant, 1: sequence-only, 2: touches the recurrence
    cls = {v: 0 for v in inv_vars}
    cls.update({v: 1 for v in seq_vars})
    cls.update({v: 2 for v in rec_inputs})
    for n_ in inner.nodes:
        k = max([cls.get(i, 0) for i in n_.inputs] or [0])
        if n_.op == "Scan":
            k = 2
        for o in n_.outputs:
            cls[o] = k
    targets = [n_ for n_ in inner.nodes if n_.op in _GLUE_TARGETS and cls[n_.outputs[0]] == 1]
    take, stack = set(), list(targets)
    while stack:                      # the targets and everything (not recurrent) they are computed from
        n_ = stack.pop()
        if id(n_) in take:
            continue
        take.add(id(n_))
        stack.extend(prod[i] for i in n_.inputs if i in prod)
    sub_nodes = [n_ for n_ in inner.nodes if id(n_) in take]
    rest = [n_ for n_ in inner.nodes if id(n_) not in take]
    if not targets or any(n_.op in _GLUE_TARGETS + ("ScalarFromTensor", "AdvancedIncSubtensor1", "Scan") for n_ in rest):
        # index nodes that DO depend on the recurrence stay: the loop keeps its host reads and
        # its place on the launch list whatever leaves it — nothing to gain
        return None
    used = {i for n_ in rest for i in n_.inputs} | set(inner.outputs)
    outs = [o for n_ in sub_nodes for o in n_.outputs if o in used and cls[o] == 1]
    if not outs or any(o in used and cls[o] == 0 for n_ in sub_nodes for o in n_.outputs):
        return None                   # (an invariant intermediate is shared with the step: leave it)
    r = batch_map_step(Plan(inner.name + "_glue", dict(V), seq_vars + inv_vars, list(outs), sub_nodes), n_seqs)
    if r is None:
        return None
    bp = r["plan"]
    # splice the whole-sequence plan in front of the Scan
    n_steps_v = node.inputs[0]
    o_seqs = list(node.inputs[L.in_seq(0):L.in_seq(n_seqs)])
    out = []
    emit = _Emit(plan, out)
    m = dict(zip(bp.inputs[n_seqs:], node.inputs[L.in_non0:]))
    for bv, ov in zip(bp.inputs[:n_seqs], o_seqs):
        src = plan.vars[ov]
        m[bv] = emit("Subtensor", [ov, n_steps_v], src.dtype, [None] + list(src.shape[1:]),
                     {"idx_list": [{"slice": [None, "in", None]}]})

    def mv(v):
        if v not in m:
            src = bp.vars[v]
            m[v] = plan.new_var(src.dtype, list(src.shape), src.name, src.const)
        return m[v]
    for n_ in bp.nodes:
        out.append(Node(n_.op, [mv(i) for i in n_.inputs], [mv(o) for o in n_.outputs], dict(n_.params)))
    new_inner = Plan(inner.name + "_noglue", V, seq_vars + outs + list(inner.inputs[n_seqs:]),
                     list(inner.outputs), rest)
    out.append(Node("Scan", [n_steps_v] + o_seqs + [mv(o) for o in bp.outputs] + list(node.inputs[L.in_seq(n_seqs):]),
                    list(node.outputs), dict(p, n_seqs=n_seqs + len(outs), inner=new_inner)))
    return out


def push_out_sequence_glue(plan: Plan) -> Plan:
    """Index glue on SEQUENCE rows inside a recurrent step — ``E[idx_t]`` of an embedding table by the
    step's index (a scalar or a vector of a batch), ``set_subtensor(zeros[i_t], 1)``, with the index
    arithmetic that feeds them — does not take part in the recurrence.  Inside the loop it costs a
    host read of the index per step (``Subtensor`` is host-side view arithmetic here) and keeps the
    loop off the persistent kernels; it is taken out as the reference's ``scan_pushout_seqs_ops``
    (scan/rewriting.py) takes Elemwise on sequences out: the glue nodes and their sequence-only
    ancestors are restated over whole sequences (:func:`batch_map_step`: one gather for all steps)
    IN FRONT of the Scan, on the first ``n_steps`` rows of the sequences, and their results enter
    the Scan as additional sequences.  What is left of the step (dots, Elemwise) is what the
    sequence hoists and the persistent kernels already handle."""
    return _rewrite_scans(plan, _sequence_glue_out)


def hoist_sequence_dots(plan: Plan, seq_inputs: List[int], invariant: set):
    """Matrix products of a Scan step that involve only a *sequence* row and loop-invariant
    matrices (``x_t @ W`` of an RNN gate) do not depend on the recurrence: they are removed from
    the step and computed for ALL steps by one GEMM before the loop (T x K @ K x M fills the
    chip; T separate K x M GEMVs cannot), the step then reads row t of the result.  The
    reference's ``scan_pushout`` rewrites (scan/rewriting.py) move Elemwise work on sequences out
    of the loop the same way but leave the dots inside.

    Returns ``(loop_plan, hoists)``; each hoist = {"kind": "gemv" | "dot", "seq": inner input id,
    "mat": invariant id, "alpha": float, "out": var id (appended to the plan inputs)}."""
    seqs = set(seq_inputs)
    keep, hoists = [], []
    for n in plan.nodes:
        h = None
        if n.op == "Gemv":
            y, alpha, A, x, beta = n.inputs
            if A in invariant and x in seqs and _cfloat(plan, alpha) is not None:
                if _cfloat(plan, beta) == 0.0:
                    h = {"kind": "gemv", "seq": x, "mat": A, "alpha": _cfloat(plan, alpha)}
                elif _cfloat(plan, beta) is not None and y in seqs:
                    # a chain  W1 x_t + W2 h_t  (the gate pre-activations a gradient Scan
                    # recomputes from stored states): accumulates onto an earlier hoisted product
                    h = {"kind": "gemv", "seq": x, "mat": A, "alpha": _cfloat(plan, alpha),
                         "beta": _cfloat(plan, beta), "acc": y}
        elif n.op in ("Dot22", "Dot"):
            a, b = n.inputs
            if a in seqs and b in invariant and plan.vars[b].ndim == 2:
                h = {"kind": "dot", "seq": a, "mat": b, "alpha": 1.0}
            elif (n.op == "Dot" and a in invariant and b in seqs and plan.vars[a].ndim == 2
                  and plan.vars[b].ndim == 1):
                h = {"kind": "gemv", "seq": b, "mat": a, "alpha": 1.0}
        if h is not None and plan.vars[n.outputs[0]].dtype in ("float32", "float64"):
            h["out"] = n.outputs[0]
            hoists.append(h)
            seqs.add(n.outputs[0])       # row t of the result is a sequence operand from here on
        else:
            keep.append(n)
    if not hoists:
        return plan, []
    loop = Plan(plan.name + "_seqdots", plan.vars, list(plan.inputs) + [h["out"] for h in hoists],
                list(plan.outputs), keep)
    return loop, hoists
