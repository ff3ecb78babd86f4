#!/usr/bin/env python
"""MRG31k3p timing probe (MI355X): ``ahip_mrg_uniform`` in float32 and float64 at 2^24 and 2^20 samples
with the reference's default 15 360 streams — one piece per stream (``parts = 1``) against the
executor's choice and two neighbours — and with 2^20 streams; ``ahip_multinomial_from_uniform`` at
65 536 x 1000 float32.  The C-ABI entry points are called directly, so ``parts`` is what the row says.

Timing: after a warm-up, ``reps`` HIP-event timings of ``iters`` back-to-back calls each; the row
carries their median (and the spread).  The sample buffers rotate over more than the 256 MiB Infinity
Cache.  The yardstick is ``ahip_fill``, the write-only kernel the library already had, over the same
bytes and buffers IN THE SAME RUN just before each group: a generator that writes n bytes cannot beat
a fill of n bytes, so every row carries its time as a multiple of the fill's.  Writes JSON lines.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from aesara_amd._lib import DTYPE_CODES, check, lib
from aesara_amd.exec_rng import M2, mrg_jump_table, mrg_parts

MALL_BYTES = 256 << 20
TORCH = {"float32": torch.float32, "float64": torch.float64}


def events():
    e0, e1 = C.c_void_p(), C.c_void_p()
    check(lib.ahip_event_create(C.byref(e0)))
    check(lib.ahip_event_create(C.byref(e1)))
    return e0, e1


def timed(fn, nbuf, iters, warmup, reps):
    """(median, min, max) microseconds per call of ``fn(k % nbuf)`` over ``reps`` event timings."""
    for k in range(warmup):
        fn(k % nbuf)
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e0, e1 = events()
    ms, us = C.c_float(), []
    for _ in range(reps):
        check(lib.ahip_event_record(e0, stream))
        for k in range(iters):
            fn(k % nbuf)
        check(lib.ahip_event_record(e1, stream))
        torch.cuda.synchronize()
        check(lib.ahip_event_elapsed_ms(e0, e1, C.byref(ms)))
        us.append(ms.value * 1e3 / iters)
    return statistics.median(us), min(us), max(us)


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fill_yardstick(bufs, dtype, args):
    val = (C.c_float if dtype == "float32" else C.c_double)(0.5)
    n = bufs[0].numel()

    def fill(k):
        check(lib.ahip_fill(DTYPE_CODES[dtype], C.byref(val), C.c_void_p(bufs[k].data_ptr()), n, stream_ptr()))
    return timed(fill, len(bufs), args.iters, max(args.warmup, 2 * len(bufs)), args.reps)


def uniform_rows(n_streams, n_elements, dtype, parts_list, args, out):
    nbytes = n_elements * (4 if dtype == "float32" else 8)
    nbuf = min(16, max(2, -(-2 * MALL_BYTES // nbytes) + 1))
    bufs = [torch.empty(n_elements, dtype=TORCH[dtype], device="cuda") for _ in range(nbuf)]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    state = torch.randint(1, M2, (n_streams, 6), dtype=torch.int32, device="cuda", generator=gen)
    new = torch.empty_like(state)
    fill_us = fill_yardstick(bufs, dtype, args)
    chosen = mrg_parts(n_streams, n_elements)
    j_max = -(-n_elements // n_streams)
    for parts in parts_list:
        c = -(-j_max // parts)
        table = torch.from_numpy(mrg_jump_table(parts, c)).cuda() if parts > 1 else None

        def draw(k):
            check(lib.ahip_mrg_uniform(DTYPE_CODES[dtype], C.c_void_p(state.data_ptr()), C.c_void_p(new.data_ptr()),
                                       n_streams, C.c_void_p(bufs[k].data_ptr()), n_elements, parts,
                                       C.c_void_p(table.data_ptr()) if table is not None else C.c_void_p(),
                                       stream_ptr()))
        us = timed(draw, nbuf, args.iters, max(args.warmup, 2 * nbuf), args.reps)
        out({"op": "MrgUniform", "dtype": dtype, "n_streams": n_streams, "n_elements": n_elements, "parts": parts,
             "chosen_parts": chosen, "steps_per_lane": c, "lanes": n_streams * parts, "sample_buffers": nbuf,
             "iters": args.iters, "reps": args.reps, "us_per_call": round(us[0], 2), "us_min": round(us[1], 2),
             "us_max": round(us[2], 2), "bytes_written": nbytes, "fill_us_same_run": round(fill_us[0], 2),
             "times_the_fill": round(us[0] / fill_us[0], 2), "fraction_of_fill": round(fill_us[0] / us[0], 4)})


def multinomial_row(nb_multi, nb_outcomes, args, out):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(2)
    pvals = torch.rand(nb_multi, nb_outcomes, dtype=torch.float32, device="cuda", generator=gen)
    pvals /= pvals.sum(dim=1, keepdim=True)
    unis = torch.rand(nb_multi, dtype=torch.float32, device="cuda", generator=gen)
    outs = [torch.empty(nb_multi, nb_outcomes, dtype=torch.int64, device="cuda") for _ in range(2)]
    val = C.c_int64(0)

    def fill(k):
        check(lib.ahip_fill(DTYPE_CODES["int64"], C.byref(val), C.c_void_p(outs[k].data_ptr()), outs[k].numel(),
                            stream_ptr()))

    def draw(k):
        check(lib.ahip_multinomial_from_uniform(
            DTYPE_CODES["float32"], DTYPE_CODES["float32"], DTYPE_CODES["int64"], C.c_void_p(pvals.data_ptr()),
            nb_outcomes, 1, C.c_void_p(unis.data_ptr()), 1, nb_multi, nb_outcomes, 1, C.c_void_p(outs[k].data_ptr()),
            stream_ptr()))
    iters = max(2, args.iters // 5)
    fill_us = timed(fill, 2, iters, 2, args.reps)
    us = timed(draw, 2, iters, 2, args.reps)
    out({"op": "MultinomialFromUniform", "dtype": "float32", "odtype": "int64", "nb_multi": nb_multi,
         "nb_outcomes": nb_outcomes, "n": 1, "iters": iters, "reps": args.reps, "us_per_call": round(us[0], 1),
         "us_min": round(us[1], 1), "us_max": round(us[2], 1), "bytes_written": outs[0].numel() * 8,
         "bytes_read": pvals.numel() * 4, "fill_us_same_run": round(fill_us[0], 1),
         "times_the_fill": round(us[0] / fill_us[0], 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mrg_probe.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="tiny shapes (rehearsal of the script)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mrg_probe.py measures on the GPU only"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def out(rec):
            print(json.dumps(rec), flush=True)
            f.write(json.dumps(rec) + "\n")
        sizes = (1 << 12, 1 << 10) if args.small else (1 << 24, 1 << 20)
        many = 1 << 8 if args.small else 1 << 20
        few = 60 if args.small else 15360
        for dtype in ("float32", "float64"):
            for n in sizes:
                chosen = mrg_parts(few, n)
                parts = sorted({1, max(2, chosen // 2), chosen, 2 * chosen})
                uniform_rows(few, n, dtype, parts, args, out)
                uniform_rows(many, n, dtype, [1], args, out)
        multinomial_row(*((256, 50) if args.small else (65536, 1000)), args, out)


if __name__ == "__main__":
    main()
