#!/usr/bin/env python
"""Expm / ExpmGrad timing probe (MI355X): n = 8, 64, 65, 512 and 2048, float32 and float64, forward and
gradient, on a Gaussian matrix with entries ``2 / sqrt(n)`` times a standard normal, through PlanExecutor (the
one-node plans the Ops lower to).  Up to 64 rows in float32 and 48 in float64 (half of that for the gradient,
which works on the 2n x 2n block matrix) every timed call replays the recorded launch list; above, the plan
runs eagerly (one host read), and that is what is timed.

Timing: wall time per call (host clock around ``iters`` calls with a device synchronisation at both ends,
after a warm-up: the eager path's host read is part of the call).

The yardsticks are taken IN THE SAME RUN: ``MatrixInverse`` at the size of the matrix that is exponentiated
(N = n, or 2n for the gradient), and the project's own ``ahip_gemm`` on the same flops — ``(products + s)
2 N^3`` for the Pade products (2, 3, 4, 5, 6 for m = 3, 5, 7, 9, 13) and the squarings, plus ``8/3 N^3`` for
the LU and its two substitutions on N right-hand sides — as C[N, N] = A[N, K] B[K, N].  ``m`` and ``s`` are the
kernels' own: the status record of ``ahip_expm_norm1``, or of one direct ``ahip_expm_tile`` call.  Writes
JSON lines.
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
from aesara_amd.exec_common import dtype_code
from aesara_amd.exec_expm import TILE_ROWS
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan
from eig_probe import wall_us
from linalg_probe import TORCH, gemm_yardstick

SIZES = (8, 64, 65, 512, 2048)
PRODUCTS = {0: 0, 3: 2, 5: 3, 7: 4, 9: 5, 13: 6}


def plan_of(op, dtype):
    plan = Plan(f"{op}_{dtype}", {}, [], [], [])
    ins = [plan.new_var(dtype, [None, None]) for _ in range(2 if op == "ExpmGrad" else 1)]
    out = plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = list(ins), [out]
    plan.nodes.append(Node(op, list(ins), [out], {}))
    return plan


def degree_and_scaling(ex, M, dtype):
    """(m, s) of the call: the blocked path's status record, else that of one direct tile launch on ``M``."""
    N = M.shape[0]
    if N > TILE_ROWS[dtype]:
        status = ex.expm_status.numpy()
    else:
        out, st = torch.empty_like(M), torch.zeros(3, dtype=torch.int64, device="cuda")
        vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
        check(lib.ahip_expm_tile(dtype_code(dtype), 1, N, vp(M), 0, N, 1, vp(out), 0, N, 1, vp(st),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        status = st.cpu().numpy()
    return int(status[1]), int(status[2])


def measure(sizes, out):
    for n in sizes:
        for dtype in ("float32", "float64"):
            gen = torch.Generator(device="cuda").manual_seed(n)
            A = torch.randn((n, n), dtype=TORCH[dtype], device="cuda", generator=gen) * (2.0 / n ** 0.5)
            G = torch.randn((n, n), dtype=TORCH[dtype], device="cuda", generator=gen)
            for op, ins in (("Expm", (A,)), ("ExpmGrad", (A, G))):
                N = n * len(ins)
                iters, warmup = (100, 10) if N <= TILE_ROWS[dtype] else (5, 2) if N <= 1024 else (3, 1)
                ex = PlanExecutor(plan_of(op, dtype), use_graph=True, borrow=True)
                us = wall_us(lambda: ex(*ins), iters, warmup + 1)
                Z = torch.zeros_like(A)
                M = A if op == "Expm" else torch.cat((torch.cat((A.t(), G), 1), torch.cat((Z, A.t()), 1)), 0).contiguous()
                m, s = degree_and_scaling(ex, M, dtype)
                flops = (PRODUCTS[m] + s) * 2.0 * N ** 3 + 8.0 / 3.0 * N ** 3
                inv = PlanExecutor(plan_of("MatrixInverse", dtype), use_graph=True, borrow=True)
                inv_us = wall_us(lambda: inv(M), iters, warmup + 1)
                K, gemm_us, gemm_rate = gemm_yardstick(N, flops, dtype, max(3, iters // 10), 1)
                out({"op": op, "n": n, "rows_exponentiated": N, "dtype": dtype, "iters": iters,
                     "replayed": bool(ex._graphs) and not ex._no_replay, "m": m, "s": s,
                     "wall_us_per_call": round(us, 1), "matrix_inverse_us_same_run": round(inv_us, 1),
                     "times_matrix_inverse": round(us / inv_us, 2), "flops": flops, "gemm_K_same_flops": K,
                     "gemm_us_same_run": round(gemm_us, 1), "times_gemm_same_flops": round(us / gemm_us, 2),
                     "fraction_of_the_gemm_rate": round(flops / (us * 1e-6) / gemm_rate, 5)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expm_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="n = 8 and 65 only (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "expm_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure((8, 65) if args.small else SIZES, out)


if __name__ == "__main__":
    main()
