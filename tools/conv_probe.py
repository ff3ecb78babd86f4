#!/usr/bin/env python
"""Convolution timing probe (MI355X): ``Conv2d``, ``Conv2dGradW`` and ``Conv2dGradI`` in float32 at
x (64, 64, 56, 56), w (64, 64, 3, 3), border_mode "half", through PlanExecutor (the plans the three
abstract Ops lower to; the gradients' ``shape`` is MakeVector of Shape_i, so every call is one
replayed launch list).

Timing: HIP events on the launch stream around ``iters`` calls after a warm-up.  The large operands
(image, topgrad) rotate over enough buffers that a buffer has left the 256 MiB Infinity Cache before
it is read again (MALL-cold); the output buffer is function-owned (``borrow=True``).  Each Op is
timed three times: whole, with the GEMM launches left out ("movement": im2col / col2im and the
small kernel copies) and with the im2col / col2im launches left out ("products": the GEMMs on
whatever the workspace holds) — the split is by launch list, not by a profiler, so the two parts
need not add up to the whole exactly.  Rates: 2 * N * O * OH * OW * (C/G) * kh * kw flop over the
event time as a fraction of the 157.3 TFLOP/s fp32 MFMA peak, for the products alone and for the
whole Op; and the bytes im2col / col2im move through ``col`` relative to the image.  Writes JSON lines.
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

import torch

from aesara_amd import knobs
from aesara_amd._lib import check, lib
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Node, Plan, Var

FP32_MFMA_PEAK = 157.3e12
MALL_BYTES = 256 << 20
PARAMS = {"border_mode": "half", "subsample": [1, 1], "filter_dilation": [1, 1], "filter_flip": True,
          "num_groups": 1}
MOVEMENT = ("ahip_im2col2d", "ahip_col2im2d")
PRODUCTS = ("ahip_gemm", "ahip_gemm_batched")


def conv_plan(op, dtype="float32"):
    t4 = [None] * 4
    if op == "Conv2d":
        vs = {0: Var(0, dtype, t4), 1: Var(1, dtype, t4), 2: Var(2, dtype, t4)}
        return Plan(op, vs, [0, 1], [2], [Node(op, [0, 1], [2], dict(PARAMS))])
    vs = {0: Var(0, dtype, t4), 1: Var(1, dtype, t4), 2: Var(2, dtype, t4), 3: Var(3, "int64", []),
          4: Var(4, "int64", []), 5: Var(5, "int64", [2]), 6: Var(6, dtype, t4)}
    return Plan(op, vs, [0, 1, 2], [6], [
        Node("Shape_i", [2], [3], {"i": 2}), Node("Shape_i", [2], [4], {"i": 3}),
        Node("MakeVector", [3, 4], [5], {"dtype": "int64"}), Node(op, [0, 1, 5], [6], dict(PARAMS))])


class Without(PlanExecutor):
    """A PlanExecutor that leaves out the launches named in ``skip`` (timing a part of an Op)."""
    skip = ()

    def _launch(self, name, args):
        if name not in self.skip:
            super()._launch(name, args)


def launch_counts(op, shape_x, shape_w):
    """C-ABI calls of one evaluation, by name (a dry run: host logic only)."""
    import numpy as np
    x, w = np.zeros(shape_x, "float32"), np.zeros(shape_w, "float32")
    dy = np.zeros((shape_x[0], shape_w[0]) + tuple(shape_x[2:]), "float32")
    ex = PlanExecutor(conv_plan(op), dry_run=True)
    ex(*{"Conv2d": (x, w), "Conv2dGradW": (x, dy, w), "Conv2dGradI": (w, dy, x)}[op])
    return {n: ex.trace.count(n) for n in sorted(set(ex.trace))}


def events():
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib.ahip_event_create(C.byref(e0)))
    check(lib.ahip_event_create(C.byref(e1)))
    return e0, e1


def timed(ex, calls, iters, warmup):
    for k in range(warmup):
        ex(*calls[k % len(calls)])
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = events()
    check(lib.ahip_event_record(e0, stream))
    for k in range(iters):
        ex(*calls[k % len(calls)])
    check(lib.ahip_event_record(e1, stream))
    torch.cuda.synchronize()
    ms = C.c_float()
    check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value * 1e3 / iters, bool(ex._graphs) and not ex._no_replay


def measure(op, shape_x, shape_w, iters, warmup):
    N, Cc, H, W = shape_x
    O, Cg, kh, kw = shape_w
    OH, OW = H, W                                       # "half" with an odd kernel, subsample 1
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float32, device="cuda", generator=g)     # noqa: E731
    image_bytes = N * Cc * H * W * 4
    nbuf = min(32, max(2, -(-2 * MALL_BYTES // image_bytes) + 1))      # (32: the tiny rehearsal shape)
    xs = [rnd(N, Cc, H, W) for _ in range(nbuf)]
    w = rnd(O, Cg, kh, kw)
    if op == "Conv2d":
        calls = [(x, w) for x in xs]
    else:
        dys = [rnd(N, O, OH, OW) for _ in range(nbuf)]
        calls = [(x, dy, w) for x, dy in zip(xs, dys)] if op == "Conv2dGradW" else \
            [(w, dy, xs[0]) for dy in dys]
    rec = {"op": op, "dtype": "float32", "x": list(shape_x), "w": list(shape_w), "border_mode": "half",
           "iters": iters, "input_buffers": nbuf, "launches": launch_counts(op, shape_x, shape_w)}
    for key, skip in (("us_per_call", ()), ("us_movement", PRODUCTS), ("us_products", MOVEMENT)):
        ex = Without(conv_plan(op), use_graph=True, borrow=True)
        ex.skip = skip
        us, replayed = timed(ex, calls, iters, max(warmup, 2 * nbuf))
        rec[key] = round(us, 1)
        rec["replayed"] = rec.get("replayed", True) and replayed
    flop = 2.0 * N * O * OH * OW * Cg * kh * kw
    col_bytes = N * Cc * kh * kw * OH * OW * 4
    rec.update({
        "flop": flop, "tflops_whole": round(flop / rec["us_per_call"] / 1e6, 2),
        "mfma_peak_fraction_whole": round(flop / (rec["us_per_call"] * 1e-6) / FP32_MFMA_PEAK, 4),
        "mfma_peak_fraction_products": round(flop / (rec["us_products"] * 1e-6) / FP32_MFMA_PEAK, 4),
        "image_bytes": image_bytes, "col_bytes": col_bytes, "col_over_image": round(col_bytes / image_bytes, 2),
        "col_tb_per_s_movement": round(col_bytes / rec["us_movement"] / 1e6, 3),
        "conv_ws_mb": float(knobs.get("CONV_WS_MB"))})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_probe.jsonl"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a tiny shape (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "conv_probe.py measures on the GPU only"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    shapes = ((2, 4, 8, 8), (4, 4, 3, 3)) if args.small else ((64, 64, 56, 56), (64, 64, 3, 3))
    with open(args.out, "w") as f:
        for op in ("Conv2d", "Conv2dGradW", "Conv2dGradI"):
            rec = measure(op, *shapes, args.iters, args.warmup)
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
