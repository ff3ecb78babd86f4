#!/usr/bin/env python
"""Dense-solve timing probe (MI355X): ``Solve`` (assume_a="gen") and ``SolveTriangular`` (lower) with
their default props at n in {64, 512, 2048, 4096}, float32 and float64, one right-hand side (a vector)
and n of them, through PlanExecutor (the one-node plans the Ops lower to; every timed call replays the
recorded launch list or hipGraph).

Timing: HIP events on the launch stream around ``iters`` calls after a warm-up; the operands are the
same buffers in every call (these sizes are bound by latency and arithmetic, not by HBM).

Flops are the algorithm's: ``Solve`` 2/3 n^3 + 2 n^2 m, ``SolveTriangular`` n^2 m.  The yardstick is the
project's own ``ahip_gemm`` IN THE SAME RUN on the same flop count at the same n: C[n, n] = A[n, K] B[K, n]
with K = flops / (2 n^2) (at least 1); every row carries its rate as a fraction of that product's.  At
n = 64 the row also carries the time of the cheapest launch of the library (a one-element fill).
At n = 4096 the 64 launches of the one-workgroup panel kernel are also timed alone, back to back
on a scratch matrix, and reported as a share of the ``Solve`` time.  Writes JSON lines.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from aesara_amd._lib import DTYPE_CODES, check, lib
from aesara_amd.exec_linalg import NB
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan

SIZES = (64, 512, 2048, 4096)
TORCH = {"float32": torch.float32, "float64": torch.float64}


def plan_of(op, dtype, vec):
    plan = Plan(f"{op}_{dtype}", {}, [], [], [])
    A, b = plan.new_var(dtype, [None, None]), plan.new_var(dtype, [None] if vec else [None, None])
    out = plan.new_var(dtype, [None] if vec else [None, None])
    plan.inputs, plan.outputs = [A, b], [out]
    params = {"assume_a": "gen", "lower": False, "check_finite": True} if op == "Solve" else \
        {"lower": True, "trans": 0, "unit_diagonal": False, "check_finite": True}
    plan.nodes.append(Node(op, [A, b], [out], params))
    return plan


def events():
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib.ahip_event_create(C.byref(e0)))
    check(lib.ahip_event_create(C.byref(e1)))
    return e0, e1


def timed(fn, iters, warmup):
    """Microseconds per call of ``fn()`` by device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = events()
    check(lib.ahip_event_record(e0, stream))
    for _ in range(iters):
        fn()
    check(lib.ahip_event_record(e1, stream))
    torch.cuda.synchronize()
    ms = C.c_float()
    check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value * 1e3 / iters


def gemm_yardstick(n, flops, dtype, iters, warmup):
    K = max(1, int(round(flops / (2.0 * n * n))))
    dt = TORCH[dtype]
    A, B, Cm = (torch.randn(s, dtype=dt, device="cuda") for s in ((n, K), (K, n), (n, n)))
    ct = C.c_float if dtype == "float32" else C.c_double
    one, zero = ct(1.0), ct(0.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def gemm():
        check(lib.ahip_gemm(DTYPE_CODES[dtype], n, n, K, C.byref(one), vp(A), K, 1, vp(B), n, 1, C.byref(zero),
                            vp(Cm), n, 1, vp(Cm), n, 1, stream))
    us = timed(gemm, iters, warmup)
    return K, us, 2.0 * n * n * K / (us * 1e-6)


def empty_launch(iters, warmup):
    t = torch.zeros(1, dtype=torch.float32, device="cuda")
    zero = C.c_uint64(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return timed(lambda: check(lib.ahip_fill(DTYPE_CODES["float32"], C.byref(zero), C.c_void_p(t.data_ptr()), 1,
                                             stream)), iters, warmup)


def panels_alone(n, dtype, iters):
    """The panel launches of one factorisation of an n x n matrix, back to back (us per factorisation)."""
    scratch = torch.randn((n, n), dtype=TORCH[dtype], device="cuda")
    src = scratch.clone()
    piv = torch.zeros(n, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    item = scratch.element_size()

    def run():
        scratch.copy_(src)
        for k in range(0, n, NB):
            e = min(k + NB, n)
            check(lib.ahip_getrf_panel(DTYPE_CODES[dtype], n - k, e - k,
                                       C.c_void_p(scratch.data_ptr() + (k * n + k) * item), n, 1,
                                       C.c_void_p(piv.data_ptr()), k, None, stream))
    copy_us = timed(lambda: scratch.copy_(src), iters, 1)
    return timed(run, iters, 1) - copy_us


def measure(sizes, out):
    for n in sizes:
        iters, warmup = (50, 5) if n <= 512 else (5, 1)
        for dtype in ("float32", "float64"):
            dt = TORCH[dtype]
            A = torch.randn((n, n), dtype=dt, device="cuda")
            T = torch.tril(A) / float(np.sqrt(n)) + 2.0 * torch.eye(n, dtype=dt, device="cuda")
            for vec in (True, False):
                m = 1 if vec else n
                b = torch.randn((n,) if vec else (n, n), dtype=dt, device="cuda")
                for op, M in (("Solve", A), ("SolveTriangular", T)):
                    flops = (2.0 / 3.0) * n ** 3 + 2.0 * n * n * m if op == "Solve" else float(n) * n * m
                    ex = PlanExecutor(plan_of(op, dtype, vec), use_graph=True, borrow=True)
                    us = timed(lambda: ex(M, b), iters, warmup + 1)
                    K, gemm_us, gemm_rate = gemm_yardstick(n, flops, dtype, iters, warmup)
                    row = {"op": op, "n": n, "m": m, "dtype": dtype, "iters": iters,
                           "replayed": bool(ex._graphs) and not ex._no_replay,
                           "launches": {k: ex.trace.count(k) // 2 for k in sorted(set(ex.trace))},
                           "us_per_call": round(us, 1), "flops": flops, "gflops": round(flops / us * 1e-3, 2),
                           "gemm_K_same_flops": K, "gemm_us_same_run": round(gemm_us, 1),
                           "gemm_gflops_same_run": round(gemm_rate * 1e-9, 2),
                           "fraction_of_the_gemm_rate": round(flops / (us * 1e-6) / gemm_rate, 5)}
                    if n == 64:
                        row["empty_launch_us_same_run"] = round(empty_launch(iters, warmup), 2)
                    if n == 4096 and op == "Solve":
                        p_us = panels_alone(n, dtype, 3)
                        row["panel_launches_alone_us"] = round(p_us, 1)
                        row["panel_share_of_the_solve"] = round(p_us / us, 3)
                    out(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linalg_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="n = 64 and 130 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "linalg_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure((64, 130) if args.small else SIZES, out)


if __name__ == "__main__":
    main()
