"""Launch records of every committed plan, for host-path refactors: a dry run of each case with
``PlanExecutor._launch`` patched at class level (the inner executors of Scan / IfElse included), one
JSON line per case: [case name, [[entry point, decoded arguments], ...]] — or the exception a dry
run raised (it cannot follow data-dependent control flow).

    python tools/launch_records.py OUT.jsonl

Run it on two checkouts; byte-identical files mean the same C-ABI calls with the same arguments in
the same order.  Dry-run buffer addresses come from a process-wide counter, so equal pointers also
mean equal allocation order."""
import collections
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conv_util, fft_util, linalg_util, mrg_util, pool_util      # noqa: E401,E402
from golden_inputs import make_input                                # noqa: E402
from aesara_amd.exec_common import _FakeBuf                         # noqa: E402
from aesara_amd.executor import PlanExecutor                        # noqa: E402
from aesara_amd.plan import Plan                                    # noqa: E402


def decode(a):
    if hasattr(a, "_obj"):                          # byref(x)
        return decode(a._obj)
    if isinstance(a, C.Array):
        return [decode(e) for e in a]
    if isinstance(a, C.Structure):
        return bytes(a).hex()
    if isinstance(a, C.c_void_p) and a.value is not None and a.value >= _FakeBuf._next:
        return "host"                               # host memory (ahip_arange's first / delta)
    if isinstance(a, C._SimpleCData):               # c_void_p, c_float, ...
        return a.value
    return a                                        # int / None (a kernel handle of a dry run)


def cases():
    with open(os.path.join(ROOT, "tests", "golden", "cases.json")) as f:
        for c in json.load(f)["cases"]:
            yield c["name"], Plan.from_json(c["plan"]), [make_input(s) for s in c["inputs"]]
    for c in conv_util.load_conv_cases():
        if c["kind"] == "op":
            v = {k: make_input(s) for k, s in c["specs"].items()}
            for op in conv_util.OPS:
                yield f"conv/{c['name']}/{op}", conv_util.case_plan(c, op), conv_util.op_inputs(op, v["x"], v["w"], v["dy"])
        else:
            yield "conv/" + c["name"], conv_util.case_plan(c), conv_util.case_inputs(c)
    for c in fft_util.load_fft_cases():
        if c["kind"] == "graph":
            yield "fft/" + c["name"], fft_util.case_plan(c), fft_util.case_inputs(c)
    for dt in pool_util.DTYPES:
        for name in pool_util.OP_CASES:
            g = pool_util.geometry(name)
            v = dict(pool_util.case_values(name, dt), maxout=np.zeros(g.out_shape, dt))
            for op in pool_util.case_ops(name):
                yield f"pool/{name}/{dt}/{op}", pool_util.op_plan(name, op, dt), [v[k] for k in pool_util.OPS[op][1]]
        for name in linalg_util.CASES:
            yield f"linalg/{name}/{dt}", linalg_util.op_plan(name, dt), linalg_util.operands(name, dt)
        for name, (_, size, opt) in mrg_util.UNIFORM_CASES.items():
            sym = opt.get("symbolic")
            plan = mrg_util.uniform_plan(len(size), dt, None if sym else size, opt.get("inplace", False))
            yield f"mrg/{name}/{dt}", plan, [mrg_util.case_state(name)] + ([np.asarray(size, "int64")] if sym else [])
        for op, table, inputs in (("MultinomialFromUniform", mrg_util.MULTINOMIAL_CASES, mrg_util.multinomial_inputs),
                                  ("ChoiceFromUniform", mrg_util.CHOICE_CASES, mrg_util.choice_inputs)):
            for name, (_, _, _, od) in table.items():
                p, u, n = inputs(name, dt)
                yield f"mrg/{name}/{dt}", mrg_util.op_plan(op, dt, dt, od, n=n), [p, u]


def main(path):
    rec = []
    PlanExecutor._launch = lambda self, name, args, _orig=PlanExecutor._launch: (
        rec.append([name, [decode(a) for a in args]]), _orig(self, name, args))[1]
    count = collections.Counter()
    with open(path, "w") as out:
        for n_case, (name, plan, inputs) in enumerate(cases(), 1):
            del rec[:]
            try:
                PlanExecutor(plan, dry_run=True)(*inputs)
                line = [name, rec]
            except Exception as e:
                line = [name, rec, type(e).__name__, str(e)]
            count.update(name for name, _ in rec)
            out.write(json.dumps(line) + "\n")
    print(f"{n_case} cases, {sum(count.values())} launches:", dict(count.most_common()))


if __name__ == "__main__":
    main(sys.argv[1])
