#!/usr/bin/env python
"""Eigvalsh timing probe (MI355X): the standard problem (``b`` absent, ``lower``) at n in {8, 64, 512,
2048}, float32 and float64, on a random symmetric matrix through PlanExecutor (the one-node plan the Op
lowers to).  Up to 64 rows every timed call replays the recorded launch list; above it the plan runs
eagerly (one host read a sweep), and that is what is timed.

Timing: wall time per call (host clock around ``iters`` calls with a device synchronisation at both
ends, after a warm-up: the eager path's host reads are part of the call).  One more eager call with a
pair of HIP events around every ``ahip_syev_tile`` and ``ahip_syev_apply`` launch gives their shares;
its status record gives the sweeps: the outer sweeps of the tournament (0 up to 64 rows) and the
largest sweep count of any tile.

The yardstick is the project's own ``ahip_gemm`` IN THE SAME RUN on ``12 n^3 sweeps`` flops (4 n^3 a
sweep for each of A J, J^T A and V J) as C[n, n] = A[n, K] B[K, n]; up to 64 rows it is the cheapest
launch of the library instead.  Writes JSON lines.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from aesara_amd._lib import check, lib
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan
from linalg_probe import TORCH, empty_launch, events, gemm_yardstick

SIZES = (8, 64, 512, 2048)
WATCHED = ("ahip_syev_tile", "ahip_syev_apply")


def plan_of(dtype):
    plan = Plan(f"Eigvalsh_{dtype}", {}, [], [], [])
    a, w = plan.new_var(dtype, [None, None]), plan.new_var(dtype, [None])
    plan.inputs, plan.outputs = [a], [w]
    plan.nodes.append(Node("Eigvalsh", [a], [w], {"lower": True}))
    return plan


def wall_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def dissect(dtype, A):
    """(us of the watched launches by name, us of the whole call, outer sweeps, tile sweeps) of one eager call."""
    ex = PlanExecutor(plan_of(dtype), use_graph=False)
    ex(A)                                              # (first use: module load, LDS attribute)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    marks, launch = [], ex._launch

    def watched(name, args):
        if name not in WATCHED:
            return launch(name, args)
        e0, e1 = events()
        check(lib.ahip_event_record(e0, stream))
        launch(name, args)
        check(lib.ahip_event_record(e1, stream))
        marks.append((name, e0, e1))
    ex._launch = watched
    del ex.trace[:]
    whole = events()
    check(lib.ahip_event_record(whole[0], stream))
    ex(A)
    check(lib.ahip_event_record(whole[1], stream))
    torch.cuda.synchronize()
    ms, us = C.c_float(), dict.fromkeys(WATCHED, 0.0)
    for name, e0, e1 in marks:
        check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
        us[name] += ms.value * 1e3
    check(lib.ahip_event_elapsed_ms(whole[0], whole[1], C.byref(ms)))
    outer = max(ex.trace.count("ahip_syev_off") - 1, 0)
    return us, ms.value * 1e3, outer, int(ex.eig_status.numpy()[1])


def measure(sizes, out):
    for n in sizes:
        iters, warmup = (200, 10) if n <= 64 else (3, 1)
        for dtype in ("float32", "float64"):
            G = torch.randn((n, n), dtype=TORCH[dtype], device="cuda")
            A = (G + G.t()) / 2
            ex = PlanExecutor(plan_of(dtype), use_graph=True, borrow=True)
            us = wall_us(lambda: ex(A), iters, warmup + 1)
            part, eager_us, outer, inner = dissect(dtype, A)
            row = {"op": "Eigvalsh", "n": n, "dtype": dtype, "iters": iters,
                   "replayed": bool(ex._graphs) and not ex._no_replay, "wall_us_per_call": round(us, 1),
                   "outer_sweeps": outer, "most_sweeps_of_a_tile": inner,
                   "eager_call_device_us": round(eager_us, 1),
                   "tile_share": round(part["ahip_syev_tile"] / eager_us, 3),
                   "apply_share": round(part["ahip_syev_apply"] / eager_us, 3)}
            if n <= 64:
                row["empty_launch_us_same_run"] = round(empty_launch(iters, warmup), 2)
            else:
                flops = 12.0 * n ** 3 * outer
                K, gemm_us, gemm_rate = gemm_yardstick(n, flops, dtype, 3, 1)
                row.update({"flops": flops, "gemm_K_same_flops": K, "gemm_us_same_run": round(gemm_us, 1),
                            "fraction_of_the_gemm_rate": round(flops / (us * 1e-6) / gemm_rate, 5)})
            out(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="n = 8 and 130 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eig_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure((8, 130) if args.small else SIZES, out)


if __name__ == "__main__":
    main()
