#!/usr/bin/env python
"""Sparse timing probe (MI355X): the gather product ``StructuredDot`` (sparse x dense) through
PlanExecutor — the one-node plans the Op lowers to, every call one replayed launch list — and the
densify-and-multiply route on the same operands as the comparison.

Gather product: a 2^18 x 2^16 matrix with 2^24 stored entries, float32 and float64, csr and csc, with
1, 64 and 256 dense columns, for two patterns: ``uniform`` (every compressed row the same length,
columns uniform) and ``powerlaw`` (the same number of entries, row lengths proportional to
rank^-0.8, rows not sorted).  A csc value goes through the orientation flip on every call; its share
is timed on its own (the stable argsort of the indices plus ``ahip_csr_flip_finish``, eagerly).

Comparison: 16384 x 16384 at 1 % density with 256 dense columns, float32: ``StructuredDot`` against
``DenseFromSparse`` followed by the dense product (``ahip_gemm``) on the same operands in the same run.

Timing: HIP events on the launch stream around ``iters`` calls after a warm-up.  Bytes are the
algorithm's — data + indices + indptr + B once + the output — over the event time as a fraction of
the 8.0 TB/s HBM peak (the dense operand is re-read per entry from the caches; nothing rotates: the
operands of the large shape are larger than the 256 MiB Infinity Cache together).  Writes JSON lines.
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

from aesara_amd._lib import check, lib
from aesara_amd.device import DevArray
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan

HBM_PEAK = 8.0e12


def sparse_inputs(plan, dtype):
    new = plan.new_var
    return [new(dtype, [None]), new("int32", [None]), new("int32", [None]), new("int64", []), new("int64", [])]


def product_plan(fmt, dtype, densify=False):
    """``StructuredDot`` as lower_sparse.py emits it, or ``DenseFromSparse`` followed by ``Dot``."""
    plan = Plan(f"{'densify' if densify else 'sdot'}_{fmt}_{dtype}", {}, [], [], [])
    sp = sparse_inputs(plan, dtype)
    b = plan.new_var(dtype, [None, None])
    out = plan.new_var(dtype, [None, None])
    plan.inputs, plan.outputs = sp + [b], [out]
    named = {"format": fmt, "name": "x"}
    if densify:
        d = plan.new_var(dtype, [None, None])
        plan.nodes.append(Node("DenseFromSparse", sp, [d], named))
        plan.nodes.append(Node("Dot", [d, b], [out], {}))
    else:
        plan.nodes.append(Node("StructuredDot", sp + [b], [out], dict(named, sparse_first=True)))
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


def pattern(kind, major, minor, nnz, gen):
    """(indices, indptr) on the device for ``major`` compressed rows over ``minor``."""
    if kind == "uniform":
        per = nnz // major
        idx = torch.randint(0, minor, (major, per), device="cuda", generator=gen, dtype=torch.int32)
        idx = torch.sort(idx, dim=1).values.reshape(-1).contiguous()
        lens = torch.full((major,), per, dtype=torch.int64)
    else:
        w = torch.arange(1, major + 1, dtype=torch.float64) ** -0.8
        lens = torch.floor(w * (nnz / w.sum())).to(torch.int64)
        lens[0] += nnz - int(lens.sum())                 # (what flooring lost goes to the longest row)
        lens = lens[torch.randperm(major, generator=torch.Generator().manual_seed(3))]
        idx = torch.randint(0, minor, (nnz,), device="cuda", generator=gen, dtype=torch.int32)
    indptr = torch.zeros(major + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lens, 0)
    return idx, indptr.to(torch.int32).cuda(), int(lens.max())


def gather_product(rows, cols, nnz, widths, iters, warmup, out, dtypes=("float32", "float64")):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    for kind in ("uniform", "powerlaw"):
        for fmt in ("csr", "csc"):
            major, minor = (rows, cols) if fmt == "csr" else (cols, rows)
            indices, indptr, longest = pattern(kind, major, minor, nnz, gen)
            ext = [np.asarray(rows, "int64"), np.asarray(cols, "int64")]
            for dtype in dtypes:
                tdt = torch.float32 if dtype == "float32" else torch.float64
                data = torch.randn(nnz, dtype=tdt, device="cuda", generator=gen)
                ex = PlanExecutor(product_plan(fmt, dtype), use_graph=True, borrow=True)
                flip_us = None
                if fmt == "csc":
                    di, dp = DevArray.from_torch(indices), DevArray.from_torch(indptr)
                    flip_us = timed(lambda: ex._sp_flip(di, dp, major, minor), iters, warmup)
                for n in widths:
                    B = torch.randn(cols, n, dtype=tdt, device="cuda", generator=gen)
                    args = [data, indices, indptr] + ext + [B]
                    us = timed(lambda: ex(*args), iters, warmup)
                    isz = data.element_size()
                    nbytes = nnz * (isz + 4) + (major + 1) * 4 + cols * n * isz + rows * n * isz
                    rec = {"op": "StructuredDot", "pattern": kind, "format": fmt, "dtype": dtype, "shape": [rows, cols],
                           "nnz": nnz, "longest_compressed_row": longest, "dense_columns": n, "iters": iters,
                           "replayed": bool(ex._graphs) and not ex._no_replay, "launches": sorted(set(ex.trace)),
                           "us_per_call": round(us, 1), "algorithmic_bytes": nbytes,
                           "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}
                    if flip_us is not None:
                        rec.update(flip_us=round(flip_us, 1), flip_share=round(flip_us / us, 3))
                    out(rec)
                    del B
                del data, ex
            del indices, indptr
            torch.cuda.empty_cache()


def comparison(n, density, width, iters, warmup, out):
    """``StructuredDot`` against ``DenseFromSparse`` + the dense product, float32 csr, same operands."""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    nnz = int(n * n * density) // n * n
    indices, indptr, _ = pattern("uniform", n, n, nnz, gen)
    data = torch.randn(nnz, dtype=torch.float32, device="cuda", generator=gen)
    B = torch.randn(n, width, dtype=torch.float32, device="cuda", generator=gen)
    args = [data, indices, indptr, np.asarray(n, "int64"), np.asarray(n, "int64"), B]
    sparse = PlanExecutor(product_plan("csr", "float32"), use_graph=True, borrow=True)
    dense = PlanExecutor(product_plan("csr", "float32", densify=True), use_graph=True, borrow=True)
    a, b = sparse(*args)[0].clone(), dense(*args)[0].clone()
    worst = float((a - b).abs().max() / b.abs().max())
    us_s = timed(lambda: sparse(*args), iters, warmup)
    us_d = timed(lambda: dense(*args), iters, warmup)
    out({"op": "StructuredDot vs DenseFromSparse + Dot", "dtype": "float32", "format": "csr", "shape": [n, n],
         "density": density, "nnz": nnz, "dense_columns": width, "iters": iters,
         "sparse_us_per_call": round(us_s, 1), "densify_and_multiply_us_per_call": round(us_d, 1),
         "sparse_over_dense_time": round(us_s / us_d, 3), "max_abs_difference_over_max": worst,
         "dense_launches": sorted(set(dense.trace))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_probe.jsonl"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sparse_probe.py measures on the GPU only"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(rec):
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        if args.small:
            gather_product(1 << 8, 1 << 6, 1 << 12, (1, 64), args.iters, args.warmup, out)
            comparison(256, 0.05, 16, args.iters, args.warmup, out)
        else:
            gather_product(1 << 18, 1 << 16, 1 << 24, (1, 64, 256), args.iters, args.warmup, out)
            comparison(16384, 0.01, 256, args.iters, args.warmup, out)


if __name__ == "__main__":
    main()
