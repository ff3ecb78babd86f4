#!/usr/bin/env python
"""Pooling timing probe (MI355X): ``Pool`` and its gradient in float32 at x (64, 64, 112, 112) for
``max`` 2x2 stride 2, ``max`` 3x3 stride 2 pad 1 and ``average_exc_pad`` 2x2 stride 2, through
PlanExecutor (the plans the Ops lower to, ws / stride / pad constant: every call is one replayed
launch list of one kernel).

Timing: HIP events on the launch stream around ``iters`` calls after a warm-up.  Every large operand
(image, maxout, gz) rotates over enough buffers that a buffer has left the 256 MiB Infinity Cache
before it is read again (MALL-cold); the output buffer is function-owned (``borrow=True``).

Bytes are the algorithm's: forward — x read once, z written once; ``MaxPoolGrad`` — x, maxout and gz
read, gx written; ``AvgPoolGrad`` — gz read, gx written (x gives its shape only).  They are reported
over the event time as a fraction of the 8.0 TB/s HBM peak.  The yardstick is the project's own
strided copy kernel (``ahip_copy_strided``) on a float32 tensor with the byte count of the image,
cold in the same way, measured IN THE SAME RUN just before each group: a pooling kernel cannot beat
a copy of the same traffic, so every line also carries its fraction relative to the copy's.  Writes
JSON lines.
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
from aesara_amd.exec_pool import pool_geometry
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan

HBM_PEAK = 8.0e12
MALL_BYTES = 256 << 20
CONFIGS = [("max", (2, 2), (2, 2), (0, 0)), ("max", (3, 3), (2, 2), (1, 1)),
           ("average_exc_pad", (2, 2), (2, 2), (0, 0))]


def pool_plan(kind, mode, ws, stride, pad, dtype="float32"):
    """``kind``: "fwd" (x) / "grad" (x, maxout, gz for max; x, gz else) — what lower_pool.py emits."""
    op = "Pool" if kind == "fwd" else ("MaxPoolGrad" if mode == "max" else "AvgPoolGrad")
    plan = Plan(f"{op}_{mode}", {}, [], [], [])
    n_data = 1 if kind == "fwd" else (3 if mode == "max" else 2)
    data = [plan.new_var(dtype, [None] * 4) for _ in range(n_data)]
    geo = [plan.add_const(np.asarray(v, "int64")) for v in (ws, stride, pad)]
    out = plan.new_var(dtype, [None] * 4)
    plan.inputs, plan.outputs = list(data), [out]
    plan.nodes.append(Node(op, data + geo, [out], {"mode": mode, "ignore_border": True, "ndim": 2}))
    return plan


def events():
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib.ahip_event_create(C.byref(e0)))
    check(lib.ahip_event_create(C.byref(e1)))
    return e0, e1


def timed(fn, calls, iters, warmup):
    """Microseconds per call of ``fn(*calls[k % len(calls)])`` by device events."""
    for k in range(warmup):
        fn(*calls[k % len(calls)])
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = events()
    check(lib.ahip_event_record(e0, stream))
    for k in range(iters):
        fn(*calls[k % len(calls)])
    check(lib.ahip_event_record(e1, stream))
    torch.cuda.synchronize()
    ms = C.c_float()
    check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value * 1e3 / iters


def copy_yardstick(xs, iters, warmup):
    """The strided copy kernel on the rotating images (read once, written once)."""
    dst = torch.empty_like(xs[0])
    i64 = lambda v: (C.c_int64 * len(v))(*v)          # noqa: E731
    shape, strides = i64(list(xs[0].shape)), i64(list(xs[0].stride()))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy(x):
        check(lib.ahip_copy_strided(DTYPE_CODES["float32"], x.dim(), shape, C.c_void_p(x.data_ptr()), strides,
                                    C.c_void_p(dst.data_ptr()), strides, 0, stream))
    us = timed(copy, [(x,) for x in xs], iters, warmup)
    nbytes = 2 * xs[0].numel() * 4
    return {"op": "ahip_copy_strided", "x": list(xs[0].shape), "dtype": "float32", "us_per_call": round(us, 1),
            "algorithmic_bytes": nbytes, "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 4)}


def measure(shape, iters, warmup, out):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    rnd = lambda s: torch.randn(*s, dtype=torch.float32, device="cuda", generator=gen)     # noqa: E731
    image_bytes = int(np.prod(shape)) * 4
    nbuf = min(32, max(2, -(-2 * MALL_BYTES // image_bytes) + 1))      # (32: the tiny rehearsal shape)
    xs = [rnd(shape) for _ in range(nbuf)]
    warm = max(warmup, 2 * nbuf)
    for mode, ws, stride, pad in CONFIGS:
        g = pool_geometry(shape, np.asarray(ws), np.asarray(stride), np.asarray(pad), 2, True, mode)
        yard = copy_yardstick(xs, iters, warm)
        out(yard)
        fwd = PlanExecutor(pool_plan("fwd", mode, ws, stride, pad), use_graph=True, borrow=True)
        zs = [fwd(x)[0].clone() for x in xs]
        gzs = [rnd(g.out_shape) for _ in range(nbuf)]
        out_bytes = int(np.prod(g.out_shape)) * 4
        for kind in ("fwd", "grad"):
            ex = fwd if kind == "fwd" else PlanExecutor(pool_plan("grad", mode, ws, stride, pad),
                                                        use_graph=True, borrow=True)
            if kind == "fwd":
                calls, nbytes = [(x,) for x in xs], image_bytes + out_bytes
            elif mode == "max":
                calls, nbytes = list(zip(xs, zs, gzs)), 2 * image_bytes + 2 * out_bytes
            else:
                calls, nbytes = [(xs[0], gz) for gz in gzs], image_bytes + out_bytes
            us = timed(ex, calls, iters, warm)
            frac = nbytes / (us * 1e-6) / HBM_PEAK
            out({"op": ex.plan.nodes[-1].op, "mode": mode, "ws": list(ws), "stride": list(stride), "pad": list(pad),
                 "dtype": "float32", "x": list(shape), "out": list(g.out_shape), "iters": iters,
                 "input_buffers": nbuf, "replayed": bool(ex._graphs) and not ex._no_replay,
                 "launches": sorted(set(ex.trace)), "us_per_call": round(us, 1), "algorithmic_bytes": nbytes,
                 "hbm_peak_fraction": round(frac, 4), "copy_us_same_run": yard["us_per_call"],
                 "copy_hbm_peak_fraction_same_run": yard["hbm_peak_fraction"],
                 "fraction_of_the_copy": round(frac / yard["hbm_peak_fraction"], 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_probe.jsonl"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tiny shape (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pool_probe.py measures on the GPU only"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(rec):
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        measure((2, 4, 8, 8) if args.small else (64, 64, 112, 112), args.iters, args.warmup, out)


if __name__ == "__main__":
    main()
