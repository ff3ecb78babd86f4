#!/usr/bin/env python
"""Row-FFT timing probe (MI355X): ``RFFT`` of 65536 x 1024 float32 and 16384 x 1024 float64 through
PlanExecutor (the plan a ``fft.rfft_op(x, x.shape[1:])`` lowers to: ``s`` stays on the host, so the
call is one replayed launch list — twiddle-table kernel + transform kernel).

Timing: HIP events on the launch stream around ``iters`` calls after a warm-up.  The inputs rotate
over enough buffers that a buffer has left the 256 MiB Infinity Cache before it is read again
(MALL-cold), the output buffer is function-owned (``borrow=True``).  The rate is the ALGORITHMIC
traffic — the real rows read once, n/2 + 1 complex bins written once — over the event time, as a
fraction of the 8.0 TB/s HBM3E peak (the yardstick of DESIGN.md's kernel table).  Also reports the
relative L2 error against NumPy in float64 / longdouble on a slice of the rows, at n and at a
Bluestein length next to it.  Writes JSON lines.
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
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan, Var

HBM_PEAK = 8.0e12
MALL_BYTES = 256 << 20


def rfft_plan(dtype):
    vs = {0: Var(0, dtype, [None, None]), 1: Var(1, "int64", []), 2: Var(2, "int64", [1]),
          3: Var(3, dtype, [None, None, 2])}
    return Plan("rfft_rows", vs, [0], [3], [
        Node("Shape_i", [0], [1], {"i": 1}),
        Node("MakeVector", [1], [2], {"dtype": "int64"}),
        Node("RFFT", [0, 2], [3], {})])


def events():
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib.ahip_event_create(C.byref(e0)))
    check(lib.ahip_event_create(C.byref(e1)))
    return e0, e1


def rel_l2(got, exact):
    exact = np.asarray(exact, dtype=np.longdouble)
    d = np.asarray(got, dtype=np.longdouble) - exact
    return float(np.sqrt((d * d).sum() / (exact * exact).sum()))


def accuracy(dtype, n, rows=64):
    x = np.random.default_rng(n).standard_normal((rows, n)).astype(dtype)
    (got,) = PlanExecutor(rfft_plan(dtype))(x)
    hi = np.float64 if dtype == "float32" else np.longdouble
    A = np.fft.rfft(x.astype(hi), axis=1)
    return rel_l2(got.cpu().numpy(), np.stack([A.real, A.imag], axis=-1))


def measure(dtype, rows, n, iters, warmup):
    tdt = getattr(torch, dtype)
    item = torch.empty(0, dtype=tdt).element_size()
    in_bytes, out_bytes = rows * n * item, rows * (n // 2 + 1) * 2 * item
    nbuf = max(2, -(-2 * MALL_BYTES // in_bytes) + 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = [torch.randn(rows, n, dtype=tdt, device="cuda", generator=g) for _ in range(nbuf)]
    ex = PlanExecutor(rfft_plan(dtype), use_graph=True, borrow=True)
    for k in range(max(warmup, 2 * nbuf)):
        ex(xs[k % nbuf])
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = events()
    check(lib.ahip_event_record(e0, stream))
    for k in range(iters):
        ex(xs[k % nbuf])
    check(lib.ahip_event_record(e1, stream))
    torch.cuda.synchronize()
    ms = C.c_float()
    check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
    us = ms.value * 1e3 / iters
    return {"op": "RFFT", "dtype": dtype, "rows": rows, "n": n, "iters": iters, "input_buffers": nbuf,
            "replayed": bool(ex._graphs) and not ex._no_replay,
            "us_per_call": round(us, 2), "algorithmic_bytes": in_bytes + out_bytes,
            "tb_per_s": round((in_bytes + out_bytes) / us / 1e6, 3),
            "hbm_peak_fraction": round((in_bytes + out_bytes) / (us * 1e-6) / HBM_PEAK, 3),
            "rel_l2_error_n": accuracy(dtype, n), "rel_l2_error_n_minus_24": accuracy(dtype, n - 24)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fft_rows.jsonl"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fft_probe.py measures on the GPU only"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for dtype, rows, n in (("float32", 65536, 1024), ("float64", 16384, 1024)):
            rec = measure(dtype, rows, n, args.iters, args.warmup)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
