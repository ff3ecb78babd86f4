#!/usr/bin/env python
"""MatrixPinv timing probe (MI355X): ``hermitian=False`` at 64 x 64, 512 x 512, 2048 x 2048 and 16384 x 64,
float32 and float64, on a random matrix through PlanExecutor (the one-node plan the Op lowers to).  Up to
64 columns every timed call replays the recorded launch list; above it the plan runs eagerly (one host
read a sweep), and that is what is timed.

Timing: wall time per call (host clock around ``iters`` calls with a device synchronisation at both
ends, after a warm-up: the eager path's host reads are part of the call).  One more eager call with a
pair of HIP events around every launch gives each entry point's share of the device time; its status
record gives the sweeps (the tile solver's own count up to 64 columns).

The yardsticks are taken IN THE SAME RUN: for the square cases ``MatrixInverse`` at the same n, and the
project's own ``ahip_gemm`` on ``sweeps * 8 k^2 rows`` flops (per sweep 2 k^2 rows for the Gram matrices
and 2 k^2 rows each for A J and, with k rows, V J — counted as 8 k^2 rows with the two-sided work on the
tiles) as C[k, k] = A[k, K] B[K, k].  Writes JSON lines.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from aesara_amd._lib import check, lib
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan
from eig_probe import wall_us
from linalg_probe import TORCH, events, gemm_yardstick

CASES = ((64, 64), (512, 512), (2048, 2048), (16384, 64))


def plan_of(op, dtype):
    plan = Plan(f"{op}_{dtype}", {}, [], [], [])
    a, out = plan.new_var(dtype, [None, None]), plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = [a], [out]
    plan.nodes.append(Node(op, [a], [out], {"hermitian": False} if op == "MatrixPinv" else {}))
    return plan


def dissect(dtype, A):
    """(us of every entry point by name, us of the whole call, sweeps) of one eager call."""
    ex = PlanExecutor(plan_of("MatrixPinv", dtype), use_graph=False)
    ex(A)                                              # (first use: module load, LDS attribute)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    marks, launch = [], ex._launch

    def watched(name, args):
        e0, e1 = events()
        check(lib.ahip_event_record(e0, stream))
        launch(name, args)
        check(lib.ahip_event_record(e1, stream))
        marks.append((name, e0, e1))
    ex._launch = watched
    whole = events()
    check(lib.ahip_event_record(whole[0], stream))
    ex(A)
    check(lib.ahip_event_record(whole[1], stream))
    torch.cuda.synchronize()
    ms, us = C.c_float(), {}
    for name, e0, e1 in marks:
        check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
        us[name] = us.get(name, 0.0) + ms.value * 1e3
    check(lib.ahip_event_elapsed_ms(whole[0], whole[1], C.byref(ms)))
    status = ex.svd_status.numpy()
    return us, ms.value * 1e3, int(status[1] or status[3])


def measure(cases, out):
    for m, n in cases:
        k = min(m, n)
        iters, warmup = (100, 10) if k <= 64 else (3, 1)
        for dtype in ("float32", "float64"):
            A = torch.randn((m, n), dtype=TORCH[dtype], device="cuda")
            ex = PlanExecutor(plan_of("MatrixPinv", dtype), use_graph=True, borrow=True)
            us = wall_us(lambda: ex(A), iters, warmup + 1)
            part, eager_us, sweeps = dissect(dtype, A)
            row = {"op": "MatrixPinv", "m": m, "n": n, "dtype": dtype, "iters": iters,
                   "replayed": bool(ex._graphs) and not ex._no_replay, "wall_us_per_call": round(us, 1),
                   "sweeps": sweeps, "eager_call_device_us": round(eager_us, 1),
                   "shares": {name: round(t / eager_us, 3) for name, t in sorted(part.items(), key=lambda kv: -kv[1])
                              if t / eager_us >= 0.005}}
            if m == n:
                inv = PlanExecutor(plan_of("MatrixInverse", dtype), use_graph=True, borrow=True)
                row["matrix_inverse_us_same_run"] = round(wall_us(lambda: inv(A), iters, warmup + 1), 1)
                flops = 8.0 * k * k * max(m, n) * sweeps
                K, gemm_us, gemm_rate = gemm_yardstick(k, flops, dtype, 3, 1)
                row.update({"flops": flops, "gemm_K_same_flops": K, "gemm_us_same_run": round(gemm_us, 1),
                            "fraction_of_the_gemm_rate": round(flops / (us * 1e-6) / gemm_rate, 5)})
            out(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pinv_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="64 x 64 and 130 x 130 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pinv_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure(((64, 64), (130, 130)) if args.small else CASES, out)


if __name__ == "__main__":
    main()
