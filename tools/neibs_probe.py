#!/usr/bin/env python
"""Images2Neibs timing probe (MI355X): float32 and float64 through PlanExecutor (the one-node plan the Op lowers to,
patch shape and step as constants; every timed call replays the recorded launch list), ``valid`` mode on a
64 x 64 x 256 x 256 image:

  3 x 3 patches at step 1      nine times the image is written (less the border)
  2 x 2 patches at step 2      disjoint patches: a permutation of the image

Timing: device events around ``iters`` calls after a warm-up.  The yardstick is taken IN THE SAME RUN: the project's
strided copy (``ahip_copy_strided``) of as many contiguous elements as the call writes.  ``bytes`` counts the image
once and the result once.  Writes JSON lines.
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

import numpy as np
import torch

from aesara_amd._lib import DTYPE_CODES, check, lib
from aesara_amd.exec_neibs import band_split, neibs_geometry
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan
from linalg_probe import TORCH, timed

CASES = (((3, 3), (1, 1)), ((2, 2), (2, 2)))


def plan_of(dtype, patch, step):
    plan = Plan(f"Images2Neibs_{dtype}", {}, [], [], [])
    x, out = plan.new_var(dtype, [None] * 4), plan.new_var(dtype, [None, None])
    vecs = [plan.add_const(np.asarray(v, "int64")) for v in (patch, step)]
    plan.inputs, plan.outputs = [x], [out]
    plan.nodes.append(Node("Images2Neibs", [x] + vecs, [out], {"mode": "valid"}))
    return plan


def copy_yardstick(count, dtype, iters, warmup):
    src, dst = (torch.zeros(count, dtype=TORCH[dtype], device="cuda") for _ in range(2))
    shape, one = (C.c_int64 * 1)(count), (C.c_int64 * 1)(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return timed(lambda: check(lib.ahip_copy_strided(DTYPE_CODES[dtype], 1, shape, C.c_void_p(src.data_ptr()), one,
                                                     C.c_void_p(dst.data_ptr()), one, 0, stream)), iters, warmup)


def measure(shape, iters, warmup, out):
    for patch, step in CASES:
        for dtype in ("float32", "float64"):
            item = 4 if dtype == "float32" else 8
            g = neibs_geometry(shape, patch, step, "valid")
            count = g.out_shape[0] * g.out_shape[1]
            x = torch.randn(shape, dtype=TORCH[dtype], device="cuda")
            ex = PlanExecutor(plan_of(dtype, patch, step), use_graph=True, borrow=True)
            us = timed(lambda: ex(x), iters, warmup + 1)
            band, tile, pitch = band_split(item, *patch, *step, *g.grid)
            row = {"op": "Images2Neibs", "mode": "valid", "shape": list(shape), "patch": list(patch), "step": list(step),
                   "dtype": dtype, "iters": iters, "replayed": bool(ex._graphs) and not ex._no_replay,
                   "band": band, "tile": tile, "pitch": pitch, "device_us_per_call": round(us, 1),
                   "out_elements": count, "bytes": (x.numel() + count) * item,
                   "gbytes_per_s": round((x.numel() + count) * item / us * 1e-3, 1)}
            del ex, x
            torch.cuda.empty_cache()
            copy_us = copy_yardstick(count, dtype, iters, warmup)
            torch.cuda.empty_cache()
            row.update({"copy_us_same_run": round(copy_us, 1), "times_copy_same_out_bytes": round(us / copy_us, 2)})
            out(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neibs_probe.jsonl"))
    ap.add_argument("--small", action="store_true", help="a 4 x 4 x 64 x 64 image (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "neibs_probe.py measures on the GPU only"
    with open(args.out, "w") as f:
        def out(row):
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")
        measure((4, 4, 64, 64) if args.small else (64, 64, 256, 256), *((3, 1) if args.small else (10, 2)), out)


if __name__ == "__main__":
    main()
