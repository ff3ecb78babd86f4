#!/usr/bin/env python
"""Timing probe of maps over small matrices (MI355X): ``aesara.map`` of ``det`` and of ``matrix_inverse`` over T =
4096 matrices at n = 8, 32, 64, float32 and float64: the plan the reference's front end lowers the map to (the
packed overlay, like tests/test_gpu_linalg_function.py), run by PlanExecutor on device tensors.

Three figures per case, IN THE SAME RUN:

* ``batched_us``: the map restated over the whole stack (scan_rewrite.batch_map_step): one ``ahip_lu_tile`` launch;
* ``launch_list_us``: the same plan run with the switch ``AESARA_HIP_MAP_LINALG=0``: the step loop on the
  launch list, the single-matrix launches once per matrix;
* ``copy_us``: the project's strided copy (``ahip_copy_strided``) of the bytes the batched call moves — the stack
  read once, the result written once (``T n^2`` elements for the inverse; for the determinant the read dominates
  and the same count is used).

Timing: device events around ``iters`` replayed calls after a warm-up (linalg_probe.timed).  Writes JSON lines.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

import ref_overlay
from convolve_probe import copy_yardstick
from linalg_probe import TORCH, timed

SIZES = (8, 32, 64)
T = 4096


def plan_of(ae, op, dtype):
    """The plan of the map of ``op`` over a tensor3."""
    import aesara
    import aesara.tensor as at
    from aesara.compile.mode import Mode
    from aesara.tensor import nlinalg
    from aesara_amd.linker import HIP_QUERY, HipLinker
    As = at.tensor3("As", dtype=dtype)
    ys, _ = aesara.map(getattr(nlinalg, op), [As])
    mode = Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY)
    return ae.function([As], ys, mode=mode).maker.linker.plan


def measure(sizes, t, out):
    ae = ref_overlay.import_reference()
    from aesara_amd.executor import PlanExecutor
    for op in ("det", "matrix_inverse"):
        for n in sizes:
            for dtype in ("float32", "float64"):
                gen = torch.Generator(device="cuda").manual_seed(n)
                A = torch.randn((t, n, n), dtype=TORCH[dtype], device="cuda", generator=gen) / n ** 0.5 \
                    + 2.0 * torch.eye(n, dtype=TORCH[dtype], device="cuda")
                row = {"op": op, "T": t, "n": n, "dtype": dtype}
                res = {}
                for key, on, iters in (("batched", True, 50), ("launch_list", False, 3)):
                    # (the switch is read when the Scan first runs: in the first call below)
                    os.environ["AESARA_HIP_MAP_LINALG"] = str(int(on))
                    ex = PlanExecutor(plan_of(ae, op, dtype), use_graph=True, borrow=True)
                    res[key] = ex(A)[0].clone()
                    modes = set(ex.scan_modes.values())
                    assert modes == {"all-rows"} if on else all(m.startswith("launch-list") for m in modes), modes
                    row[key + "_us"] = round(timed(lambda: ex(A), iters, 2), 1)
                    row[key + "_iters"] = iters
                    row[key + "_replayed"] = bool(ex._graphs) and not ex._no_replay
                a, b = (r.double() for r in res.values())
                row["max_rel_difference"] = float(((a - b).abs().max() / b.abs().max()).item())
                row["copy_us"] = round(copy_yardstick(t * n * n, dtype, 50, 5), 1)
                row["launch_list_over_batched"] = round(row["launch_list_us"] / row["batched_us"], 1)
                row["batched_over_copy"] = round(row["batched_us"] / row["copy_us"], 2)
                out(row)
    os.environ.pop("AESARA_HIP_MAP_LINALG", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_linalg_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="T = 64, n = 8 and 64 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "batched_linalg_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure((8, 64) if args.small else SIZES, 64 if args.small else T, out)


if __name__ == "__main__":
    main()
