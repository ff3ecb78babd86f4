#!/usr/bin/env python
"""Convolve timing probe (MI355X): float32 and float64 through PlanExecutor (the one-node plan the Op lowers
to; every timed call replays the recorded launch list), Gaussian operands.

  full,  m = 2^24, n = 3, 64, 1024       one output tile a workgroup, no tap split
  valid, n = 2^20, m = n + 7             eight outputs: one tile, the taps split over 2048 workgroups

Timing: device events around ``iters`` calls after a warm-up.  The yardsticks are taken IN THE SAME RUN: for the
``full`` cases the project's strided copy (``ahip_copy_strided``) of ``m + n - 1`` contiguous elements — what the
call must at least read and write; for the ``valid`` case the project's ``ahip_gemv`` on the same flops, an
``8 x n`` matrix against the taps, which reads eight times the bytes the convolution needs.  ``flops`` counts
``2 n`` per output of ``valid`` and the exact number of products times two for ``full``.  Writes JSON lines.
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

from aesara_amd._lib import DTYPE_CODES, check, lib
from aesara_amd.exec_convolve import window
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan
from linalg_probe import TORCH, timed

CASES = (("full", 1 << 24, 3), ("full", 1 << 24, 64), ("full", 1 << 24, 1024), ("valid", (1 << 20) + 7, 1 << 20))


def plan_of(dtype, mode):
    plan = Plan(f"Convolve_{dtype}_{mode}", {}, [], [], [])
    a, v, out = (plan.new_var(dtype, [None]) for _ in range(3))
    plan.inputs, plan.outputs = [a, v], [out]
    plan.nodes.append(Node("Convolve", [a, v], [out], {"mode": mode}))
    return plan


def vp(t):
    return C.c_void_p(t.data_ptr())


def copy_yardstick(count, dtype, iters, warmup):
    src, dst = (torch.randn(count, dtype=TORCH[dtype], device="cuda") for _ in range(2))
    shape, one = (C.c_int64 * 1)(count), (C.c_int64 * 1)(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return timed(lambda: check(lib.ahip_copy_strided(DTYPE_CODES[dtype], 1, shape, vp(src), one, vp(dst), one, 0,
                                                     stream)), iters, warmup)


def gemv_yardstick(rows, cols, dtype, iters, warmup):
    A, x, y = (torch.randn(s, dtype=TORCH[dtype], device="cuda") for s in ((rows, cols), (cols,), (rows,)))
    ct = C.c_float if dtype == "float32" else C.c_double
    one, zero = ct(1.0), ct(0.0)
    need = int(lib.ahip_gemv_ws_bytes(DTYPE_CODES[dtype], rows, cols))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return timed(lambda: check(lib.ahip_gemv(DTYPE_CODES[dtype], rows, cols, C.byref(one), vp(A), cols, 1, vp(x), 1,
                                             C.byref(zero), vp(y), 1, vp(y), 1, vp(ws), need, stream)), iters, warmup)


def measure(cases, out):
    for mode, m, n in cases:
        lo, length = window(mode, m, n)
        # products: every (j, k) with 0 <= j - k < m inside the window; `full` has all m n of them
        flops = 2.0 * (m * n if mode == "full" else length * n)
        for dtype in ("float32", "float64"):
            item = 4 if dtype == "float32" else 8
            a, v = (torch.randn(k, dtype=TORCH[dtype], device="cuda") for k in (m, n))
            iters, warmup = (20, 3) if flops > 1e9 else (100, 10)
            ex = PlanExecutor(plan_of(dtype, mode), use_graph=True, borrow=True)
            us = timed(lambda: ex(a, v), iters, warmup + 1)
            row = {"op": "Convolve", "mode": mode, "m": m, "n": n, "dtype": dtype, "iters": iters,
                   "replayed": bool(ex._graphs) and not ex._no_replay, "device_us_per_call": round(us, 1),
                   "ws_bytes": int(lib.ahip_convolve_ws_bytes(DTYPE_CODES[dtype], m, n, lo, length)),
                   "flops": flops, "gflops": round(flops / us * 1e-3, 1),
                   "bytes": (m + n + length) * item, "gbytes_per_s": round((m + n + length) * item / us * 1e-3, 1)}
            if mode == "full":
                copy_us = copy_yardstick(length, dtype, iters, warmup)
                row.update({"copy_us_same_run": round(copy_us, 1), "times_copy_same_bytes": round(us / copy_us, 2)})
            else:
                gemv_us = gemv_yardstick(length, n, dtype, iters, warmup)
                row.update({"gemv_rows": length, "gemv_us_same_run": round(gemv_us, 1),
                            "times_gemv_same_flops": round(us / gemv_us, 2)})
            out(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convolve_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="m = 2^16 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "convolve_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure((("full", 1 << 16, 64), ("valid", (1 << 12) + 7, 1 << 12)) if args.small else CASES, out)


if __name__ == "__main__":
    main()
