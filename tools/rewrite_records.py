"""Rewrite records of every golden plan, for refactors of the Scan plan rewrites: what each
plan-to-plan rewrite makes of every case of ``tests/golden/cases.json``, one JSON line per result:
[case name, rewrite, ``Plan.dumps(sort_keys=True)`` or the rewrite's other results].

    python tools/rewrite_records.py OUT.jsonl

Per plan: the four rewrites of ``PlanExecutor.__init__`` in its order; per Scan node of the result
(nested ones included): the single-node ``push_out_product_accumulators`` form of
``ScanMixin._op_Scan`` with its need / same / le2 lists, ``batch_map_step``, the chain
``split_column_slices`` -> ``split_invariant`` -> ``hoist_sequence_only`` -> ``hoist_sequence_dots``
and ``merge_shared_left_dots`` of a stacked lifted plan.  Run it on two checkouts; byte-identical
files mean the same plans with the same variable ids.  Prints how often each rewrite changed
something."""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from aesara_amd import exec_common as ec       # noqa: E402
from aesara_amd.plan import Plan                # noqa: E402

count = collections.Counter()


def dump(x):
    if isinstance(x, Plan):
        try:
            return x.dumps(sort_keys=True)
        except TypeError as e:                  # (a host callback cannot be serialised)
            return "TypeError: %s" % e
    if isinstance(x, dict):
        return {k: dump(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [dump(v) for v in x]
    return x


def scans(plan):
    for node in plan.nodes:
        if node.op == "Scan":
            yield node
            yield from scans(node.params["inner"])


def walk(plan, emit):
    """``plan`` as a PlanExecutor is handed it: its constructor rewrites, then every Scan node"""
    for key, fn in (("glue", ec.push_out_sequence_glue), ("accumulators", ec.push_out_accumulators),
                    ("product accumulators (constructor)", ec.push_out_product_accumulators),
                    ("assembled columns", ec.split_assembled_columns)):
        new = fn(plan)
        count[key] += new is not plan
        plan = new
    emit("constructor", plan)
    zeros, last = ec.zero_filled_vars(plan), ec.read_last_row_only(plan)
    for node in scans(plan):
        p, inner = node.params, node.params["inner"]
        need, same, le2 = [], [], []
        wrap = Plan("scan_%d_sunk" % node.outputs[0], dict(plan.vars), list(node.inputs), list(node.outputs), [node])
        wrap2 = ec.push_out_product_accumulators(wrap, need, same, zeros=zeros, last_only=last, need_le2=le2)
        count["product accumulators (per node)"] += wrap2 is not wrap
        emit("sunk", {"plan": wrap2, "need": need, "same": same, "le2": le2})
        r = ec.batch_map_step(inner, p["n_seqs"])       # (whatever the Scan's class: more rules are walked)
        count["batch_map_step"] += r is not None
        emit("batch_map_step", r)
        n_var = len(inner.inputs) - p["n_non_seqs"]
        cols = ec.split_column_slices(inner, set(inner.inputs[n_var:]))
        count["split_column_slices"] += cols is not inner
        pre, loop, hoisted = ec.split_invariant(cols, cols.inputs[n_var:])
        count["split_invariant"] += pre is not None
        seq_ids, inv_set = list(loop.inputs[:p["n_seqs"]]), set(loop.inputs[n_var:])
        loop, lifted = ec.hoist_sequence_only(loop, seq_ids, inv_set)
        count["hoist_sequence_only"] += lifted is not None
        loop, seqdots = ec.hoist_sequence_dots(loop, seq_ids, inv_set)
        count["hoist_sequence_dots"] += bool(seqdots)
        emit("chain", {"pre": pre, "hoisted": hoisted, "lifted": lifted, "seqdots": seqdots, "loop": loop})
        if lifted is not None and lifted.get("stacked"):
            wide = ec.merge_shared_left_dots(lifted["plan"])
            count["merge_shared_left_dots"] += wide is not lifted["plan"]
            emit("merge_shared_left_dots", wide)


def main(path):
    with open(os.path.join(ROOT, "tests", "golden", "cases.json")) as f:
        cases = json.load(f)["cases"]
    n_lines = 0
    with open(path, "w") as out:
        for c in cases:
            def emit(what, x, name=c["name"]):
                nonlocal n_lines
                n_lines += 1
                out.write(json.dumps([name, what, dump(x)], sort_keys=True) + "\n")
            walk(Plan.from_json(c["plan"]), emit)
    print(f"{len(cases)} cases, {n_lines} records; changed:", dict(sorted(count.items())))


if __name__ == "__main__":
    main(sys.argv[1])
