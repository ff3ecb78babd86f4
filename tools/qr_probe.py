#!/usr/bin/env python
"""QR timing probe (MI355X): ``nlinalg.qr(A)`` ('reduced': Q and R) at 64^2, 1024^2, 4096^2 and
16384 x 256, float32 and float64, through PlanExecutor (the one-node plan the Op lowers to; every timed
call replays the recorded launch list or hipGraph).

Timing: HIP events on the launch stream around ``iters`` calls after a warm-up; the operand is the same
buffer in every call.

Flops are the algorithm's: 2 N^2 (M - N / 3) for the factorisation and the same again for Q.  The
yardstick is the project's own ``ahip_gemm`` IN THE SAME RUN on the same flop count: C[M, N] = A[M, K]
B[K, N] with K = flops / (2 M N) (at least 1); every row carries its rate as a fraction of that
product's.  The launches of the one-workgroup panel kernel are also timed alone, back to back on a
scratch matrix in the workspace's layout, and reported as a share of the call.  Writes JSON lines.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from aesara_amd._lib import DTYPE_CODES, check, lib
from aesara_amd.exec_linalg import NB
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan

from linalg_probe import TORCH, timed

SHAPES = ((64, 64), (1024, 1024), (4096, 4096), (16384, 256))


def plan_of(dtype):
    plan = Plan(f"qr_{dtype}", {}, [], [], [])
    A = plan.new_var(dtype, [None, None])
    Q, R = plan.new_var(dtype, [None, None]), plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = [A], [Q, R]
    plan.nodes.append(Node("QR", [A], [Q, R], {"mode": "reduced"}))
    return plan


def gemm_yardstick(m, n, flops, dtype, iters, warmup):
    K = max(1, int(round(flops / (2.0 * m * n))))
    dt = TORCH[dtype]
    A, B, Cm = (torch.randn(s, dtype=dt, device="cuda") for s in ((m, K), (K, n), (m, n)))
    ct = C.c_float if dtype == "float32" else C.c_double
    one, zero = ct(1.0), ct(0.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731

    def gemm():
        check(lib.ahip_gemm(DTYPE_CODES[dtype], m, n, K, C.byref(one), vp(A), K, 1, vp(B), n, 1, C.byref(zero),
                            vp(Cm), n, 1, vp(Cm), n, 1, stream))
    us = timed(gemm, iters, warmup)
    return K, us, 2.0 * m * n * K / (us * 1e-6)


def panels_alone(src, dtype, iters):
    """The panel launches of one factorisation of ``src`` (M x N), back to back on a copy held like
    the executor's workspace: an (N, M) buffer, element (r, c) at c * M + r (us per factorisation)."""
    m, n = src.shape
    k_all = min(m, n)
    src_t = src.t().contiguous()
    scratch = src_t.clone()
    V = torch.zeros((NB, m), dtype=TORCH[dtype], device="cuda")
    tau = torch.zeros(k_all, dtype=TORCH[dtype], device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    item = scratch.element_size()

    def run():
        scratch.copy_(src_t)
        for k in range(0, k_all, NB):
            e = min(k + NB, k_all)
            check(lib.ahip_geqr2_panel(DTYPE_CODES[dtype], m - k, e - k,
                                       C.c_void_p(scratch.data_ptr() + (k * m + k) * item), 1, m,
                                       C.c_void_p(tau.data_ptr() + k * item),
                                       C.c_void_p(V.data_ptr() + k * item), 1, m, stream))
    copy_us = timed(lambda: scratch.copy_(src_t), iters, 1)
    return timed(run, iters, 1) - copy_us


def measure(shapes, out):
    for m, n in shapes:
        iters, warmup = (200, 10) if m * n <= 4096 else (20, 3) if m * n <= 1 << 20 else (5, 1)
        for dtype in ("float32", "float64"):
            dt = TORCH[dtype]
            A = torch.randn((m, n), dtype=dt, device="cuda") / float(max(m, n)) ** 0.5 \
                + 2.0 * torch.eye(m, n, dtype=dt, device="cuda")
            fact = 2.0 * n * n * (m - n / 3.0)
            flops = 2.0 * fact
            ex = PlanExecutor(plan_of(dtype), use_graph=True, borrow=True)
            us = timed(lambda: ex(A), iters, warmup + 1)
            K, gemm_us, gemm_rate = gemm_yardstick(m, n, flops, dtype, iters, warmup)
            p_us = panels_alone(A, dtype, min(iters, 10))
            out({"op": "QR", "mode": "reduced", "m": m, "n": n, "dtype": dtype, "iters": iters,
                 "replayed": bool(ex._graphs) and not ex._no_replay,
                 "launches": {k: ex.trace.count(k) // 2 for k in sorted(set(ex.trace))},
                 "us_per_call": round(us, 1), "flops": flops, "gflops": round(flops / us * 1e-3, 2),
                 "gemm_K_same_flops": K, "gemm_us_same_run": round(gemm_us, 1),
                 "gemm_gflops_same_run": round(gemm_rate * 1e-9, 2),
                 "fraction_of_the_gemm_rate": round(flops / (us * 1e-6) / gemm_rate, 5),
                 "panel_launches_alone_us": round(p_us, 1), "panel_share_of_the_call": round(p_us / us, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qr_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="64^2 and 130 x 66 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "qr_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure(((64, 64), (130, 66)) if args.small else SHAPES, out)


if __name__ == "__main__":
    main()
