#!/usr/bin/env python
"""Benchmark of the HIP linker hot path (driver contract: see the repo prompt / DESIGN.md §5).

Headline (``value``) = BASELINE.json configs[1]: the fused Elemwise chain
``exp(-(x-mu)**2 / (2*sigma**2)).sum()`` on a float64 4096x4096 matrix — the plan is the one the
HIP linker lowers from the reference's FAST_RUN graph (tests/golden: cfg2_gauss_sum; shapes are
dynamic, so the same plan runs at 4096x4096).  One "step" = one evaluation of the compiled
function: one launch-list replay (a single host call into libaesara_hip.so) that issues the ONE
fused Elemwise+Sum kernel (in-kernel deterministic finalize), with ``x`` resident in HBM.

A plain run (``--gpus 1 --steps K --warmup W``) does only that: set up, warm up, time K steps,
print the line (``--dump-outputs DIR``: and write what the last timed step returned to
``DIR/gauss_sum.npy``).  Everything else below runs with ``--full`` only.

With ``--full`` the same JSON line carries ``"secondary"``: every other BASELINE config at its full
shape, each with its own ``roofline`` timed by HIP events in this run and a correctness assert
against an fp64 restatement on the same data:

* cfg3b  Gemm fp32 4096^3 (the ``check_blas.py:54-57`` update ``C <- 0.4*C + 0.8*dot(A,B)``), MFMA-bound
* cfg3a  Gemv fp64 4096^2 (``M.dot(v) + a``, BASELINE configs[2]'s graph), HBM-bound
* cfg1b  matrix add fp64 4096^2, HBM-bound
* cfg4   Scan GRU T=512 H=1024 fp32, B=1 (vector state) and B=64 (matrix state)
* cfg5   logistic-regression logp + grad, N=2^24 x 256 fp32 (16 GiB of X) — row-sharded over the
         ranks for N>1 (strong scaling: 2^24/N rows per rank, ONE all-reduce of the 258 fp64 partials)

N>1: the headline stays config 2 under weak scaling (every rank evaluates its own 4096x4096 row
block; the CAReduce partial is summed with one bucketed asynchronous RCCL all-reduce), so the
driver's N=1,2,4,8 series is one workload; config 5's strong-scaling figure rides in ``secondary``.

The timed region ROTATES over ``--rotate`` (8) distinct 128 MiB inputs (1 GiB > the 256 MiB
memory-side Infinity Cache), so every eval streams its matrix from HBM: ``roofline`` is the
MALL-cold figure; the same-buffer (cache-assisted) figure of earlier rounds rides in
``config.warm``.  cfg3a does the same.

Prints ONE JSON line (rank 0).  ``roofline`` is measured live with HIP events on the launch
stream.  ``cpu_baseline`` (``--full``, rank 0, N=1 only): the REFERENCE itself — its ``Mode("cvm","fast_run")``
C linker on this host (``oracle/time_reference.py`` in a child process, ``kind: "reference"``) when
the reference front end is available (``/root/reference`` or the packed overlay ``oracle/_ref/``),
else the oracle's C port of the same loops (``kind: "port"``).  With the front end available the
line also carries ``through_function`` (top level): the headline itself is then driven through the real
``aesara.function(..., mode="HIP")`` -> ``Function.__call__`` instead of the bare executor.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (guide: 8.0 TB/s; ~6.3 TB/s achievable)
MFMA_F32_PEAK = 157.3          # TFLOP/s, v_mfma_f32_16x16x4_f32 dense (guide)
ROWS, COLS = int(os.environ.get("AESARA_BENCH_ROWS", "4096")), 4096   # (rows: size sweeps of tools/ only)
ALGO_BYTES = ROWS * COLS * 8   # x read once (134 217 728 B per eval)


class DevTimer:
    """HIP events on the launch stream (torch.cuda.Event only sees torch's current stream —
    here they coincide, but the events are created through the C-ABI like the launches)."""

    def __init__(self, C, lib, check, torch):
        self.C, self.lib, self.check, self.torch = C, lib, check, torch
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        check(lib.ahip_event_create(C.byref(self.e0)))
        check(lib.ahip_event_create(C.byref(self.e1)))

    def stream(self):
        return self.C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def time(self, fn, iters, warmup=3):
        """(device ms per call, wall ms per call) over `iters` back-to-back calls."""
        for _ in range(warmup):
            fn()
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.check(self.lib.ahip_event_record(self.e0, self.stream()))
        for _ in range(iters):
            fn()
        self.check(self.lib.ahip_event_record(self.e1, self.stream()))
        self.torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / iters
        ms = self.C.c_float()
        self.check(self.lib.ahip_event_elapsed_ms(self.e0, self.e1, self.C.byref(ms)))
        return ms.value / iters, wall * 1e3


def roof(bound, work, dev_ms, peak, **extra):
    if bound == "hbm":
        ach, unit = work / (dev_ms * 1e-3) / 1e9, "GB/s"
    else:
        ach, unit = work / (dev_ms * 1e-3) / 1e12, "TFLOP/s"
    r = {"bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
         "kernel_ms": dev_ms, "algorithmic": work}
    r.update(extra)
    return r


HANDOFF_FLOOR_US = 0.89  # ONE all-to-all hand-off of a 1024-float vector between 256 co-resident workgroups,
#                          measured in isolation with the kernel's own exchange (tagged 8-byte granules, 4 polling
#                          wavefronts, first poll held back 15 x 64 cycles, s_sleep 1 between polls) and nothing
#                          else in the step: tools/handoff_floor.py -> profiles/r05_handoff_floor.json (0.886 us;
#                          0.857 with 8 polling wavefronts; 1.63 with the polls issued back to back, the form the
#                          guide's "allgather" row prices at 2.4-3.0 us).  A step of config 4 B = 1 has two of
#                          them plus the row dots and LDS staging between them, so the ratio below reads ~1.9


def latency_row(dev_ms, T, restreamed_bytes, handoffs_per_step, resident_bound_bytes):
    """Config 4 with a vector state is bound by dependent hand-offs, not by bytes: the row
    reports us/step against the hand-off floor.  ``vs_restreamed_bound`` (SURVEY §8d context) is
    what the time would be worth if the weights were re-streamed from HBM every step, as the
    reference's per-step GEMVs do — it is NOT an achieved HBM fraction (the kernel moves ~69 MB)."""
    us = dev_ms * 1e3 / T
    floor = handoffs_per_step * HANDOFF_FLOOR_US
    return {"bound": "latency", "unit": "us/step", "us_per_step": us, "kernel_ms": dev_ms,
            "handoffs_per_step": handoffs_per_step, "handoff_floor_us_per_step": floor,
            "us_per_step_vs_handoff_floor": us / floor,
            "vs_restreamed_bound": restreamed_bytes / (dev_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "restreamed_bytes": restreamed_bytes, "resident_bound_bytes": resident_bound_bytes,
            "note": "latency-bound by construction: weights stay on chip, each step is "
                    "`handoffs_per_step` dependent vector exchanges; no HBM/MFMA fraction applies "
                    "(floor = the same exchange measured in isolation, tools/handoff_floor.py)"}


def pick_transport(world, torch, dist):
    """The exchange transport of an N > 1 run: the C-ABI communicator by default (ahip_comm_*:
    RCCL enqueued by the shim on the launch stream — a sharded evaluation, rounds + all-reduces,
    is ONE recorded launch list, no Python between the rounds); torch.distributed (backend nccl =
    RCCL, one Python call per collective) when AESARA_BENCH_COMM=torch, when the process group is
    not RCCL (the one-device gloo hooks: RCCL refuses two ranks on one device) or when
    ahip_comm_init_rank fails on any rank.  Returns (group, kind, description)."""
    if world == 1:
        return None, "none", None
    from aesara_amd.dist import HipComm
    kind = os.environ.get("AESARA_BENCH_COMM", "abi")
    if dist.get_backend() != "nccl":
        kind = "torch"
    err = None
    if kind == "abi":
        group, ok = None, torch.ones(1, device="cuda")
        try:
            group = HipComm(bootstrap_group=dist.group.WORLD)
        except Exception as e:              # noqa: BLE001
            err = "%s: %s" % (type(e).__name__, e)
            ok.zero_()
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)        # every rank takes the same transport
        if ok.item() == 1.0:
            return group, "abi", ("C-ABI communicator (ahip_comm_*: RCCL on the launch stream, "
                                  "all-reduces recorded into the launch lists), %d ranks" % group.world)
        if group is not None:
            group.close(force=True)
        err = err or "another rank failed"
    return dist.group.WORLD, "torch", "torch.distributed (%s)%s" % (
        dist.get_backend(), "; C-ABI communicator unavailable: " + err if err else "")


def wait_for_stream(C, lib, check, torch, seconds):
    """True when everything enqueued on the launch stream so far finishes within ``seconds`` — an
    event polled from the host (``ahip_event_query``), never a blocking synchronize: a collective
    whose peers never arrive would block that forever."""
    ev = C.c_void_p()
    check(lib.ahip_event_create(C.byref(ev)))
    check(lib.ahip_event_record(ev, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    t_end = time.perf_counter() + seconds
    done = False
    while time.perf_counter() < t_end:
        r = lib.ahip_event_query(ev)
        if r == 0:
            done = True
            break
        if r < 0:
            break
        time.sleep(0.005)
    if done:
        lib.ahip_event_destroy(ev)       # (a pending event is leaked on purpose: destroying it could block)
    return done


TRANSPORT_GUARD_S = float(os.environ.get("AESARA_BENCH_TRANSPORT_GUARD_S", "60"))


def guard_first_exchange(first_exchange, group, C, lib, check, torch, dist, rank):
    """Run the FIRST sharded evaluation of the C-ABI transport under a wall-clock guard (VERDICT r5
    weak 7: a recorded all-reduce that hangs or mis-pairs with N real ranks — a path no box of this
    project has executed — would otherwise cost the run its whole timeout with no line printed).
    Returns None when the exchange completed on every rank, else a description: the communicator has
    then been aborted (ncclCommAbort terminates the stuck collective) and the caller continues on
    torch.distributed."""
    err = None
    try:
        first_exchange()
        if not wait_for_stream(C, lib, check, torch, TRANSPORT_GUARD_S):
            err = "first sharded evaluation did not complete within %.0f s" % TRANSPORT_GUARD_S
    except Exception as e:                               # noqa: BLE001
        err = "%s: %s" % (type(e).__name__, str(e)[:200])
    if err is not None:
        try:
            group.abort()
        except Exception:                                # noqa: BLE001
            pass
    # every rank takes the same decision (torch.distributed has its own communicator and stream)
    ok = torch.tensor([0.0 if err else 1.0], device="cuda")
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if ok.item() == 1.0:
        return None
    if err is None:
        err = "another rank's first sharded evaluation failed"
        try:
            group.abort()
        except Exception:                                # noqa: BLE001
            pass
    if rank == 0:
        print(json.dumps({"transport_error": err, "transport": "C-ABI communicator (ahip_comm_*)",
                          "fallback": "torch.distributed"}), file=sys.stderr, flush=True)
    return err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true",
                    help="headline only (used by the rocprofv3 passes of tools/profile_bench.sh)")
    ap.add_argument("--only-secondary", default="",
                    help="comma list of secondary workloads to run (default: all)")
    ap.add_argument("--cfg5-log2n", type=int, default=24, help="config 5 rows = 2**k (total)")
    ap.add_argument("--eager", action="store_true", help="no launch-list replay (per-node launches)")
    ap.add_argument("--no-warm", action="store_true",
                    help="skip the same-buffer and through-Function legs (rocprofv3 passes: every "
                         "profiled eval of the headline kernel is then a MALL-cold one)")
    ap.add_argument("--executor-level", action="store_true",
                    help="time the bare PlanExecutor even when the reference front end is present")
    ap.add_argument("--no-clock-warmup", action="store_true",
                    help="skip the untimed clock warm-up in front of the timed region")
    ap.add_argument("--rotate", type=int, default=8,
                    help="distinct input buffers the timed region cycles through (1 = same buffer)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything besides the headline: the fp64 check of the benchmarked "
                         "path, the sustained / same-buffer / executor-level / read-only-ceiling legs, "
                         "the secondary configs and the CPU baseline with its reference comparison")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy")
    args = ap.parse_args()

    import ctypes as C

    import numpy as np
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain ``python bench.py --gpus N``: become the launcher the contract names (one rank per
        # GPU of this node over RCCL), same arguments, loopback rendezvous on a free port
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        if os.environ.get("AESARA_BENCH_DRY_LAUNCH"):       # (tests: show the launch line, run nothing)
            print(json.dumps({"launch": cmd}))
            return
        sys.stdout.flush()
        os.execv(sys.executable, cmd)
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run "
                         "--nproc-per-node %d" % (args.gpus, world, args.gpus))
    # test hooks (single-GPU boxes): AESARA_BENCH_BACKEND=gloo + AESARA_BENCH_ONE_DEVICE=1 run
    # the N>1 control flow (ring slots, bucketed async all-reduce) with every rank on cuda:0
    backend = os.environ.get("AESARA_BENCH_BACKEND", "nccl")
    if os.environ.get("AESARA_BENCH_ONE_DEVICE"):
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from golden_util import CASES, case_plan
    from aesara_amd._lib import check, lib
    from aesara_amd.executor import PlanExecutor

    G = not args.eager
    group, comm_kind, transport = pick_transport(world, torch, dist)

    def plan_of(name):
        return case_plan(next(c for c in CASES if c["name"] == name))

    def randn(shape, dtype, seed):
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        return torch.randn(*shape, dtype=dtype, device="cuda", generator=g)

    timer = DevTimer(C, lib, check, torch)
    f64, f32 = torch.float64, torch.float32

    ex = PlanExecutor(plan_of("cfg2_gauss_sum"), use_graph=G, borrow=True)

    ref_warm = None

    # synthetic input of the named shape, generated on device (rank-specific row block);
    # NROT distinct buffers: consecutive evals never find their matrix in the 256 MiB MALL
    NROT = max(1, args.rotate)
    xs = [randn((ROWS, COLS), f64, 1 + rank + 100 * k) for k in range(NROT)]
    x = xs[0]
    mu = torch.tensor(0.1, dtype=f64, device="cuda")
    sigma = torch.tensor(1.3, dtype=f64, device="cuda")

    from aesara_amd.dist import ShardedFunction, plan_split_outputs

    kinds = plan_split_outputs(plan_of("cfg2_gauss_sum"), 0)   # ["allreduce"]: Sum over the split rows
    # ring of result slots: the fused kernel of eval i writes its partial straight into
    # ring[i % R] (executor out=), and every BUCKET evals ONE asynchronous RCCL all-reduce sums
    # a bucket of partials over the ranks (bucketed: the 8-byte payload is latency-bound on xGMI),
    # so consecutive evals pipeline behind the collective
    R, BUCKET = 32, 8
    ring = torch.zeros(R, dtype=f64, device="cuda")
    slots = [ring[i] for i in range(R)]
    state = {"i": 0}
    reducer = ShardedFunction(lambda bucket: [bucket], kinds, group=group if comm_kind == "abi" else None)

    # N = 1 with the reference front end present (the packed overlay travels to the GPU box): the
    # timed step is ``f(x, mu, sigma)`` of ``f = aesara.function([x, mu, sigma], expr, mode="HIP")``
    # — Function.__call__ with its own input filtering (no trust_input), device tensor in, device
    # tensor out: the "compiled-fn evals/sec" of the metric.  The bare executor rides in
    # ``config.executor_level``; ``--executor-level`` (and N > 1: ring slots need ``out=``) times it.
    fn, fn_info = (None, None)
    if world == 1 and not args.executor_level:
        fn, fn_info = make_function(xs[0], torch, np)

    def step():
        i = state["i"]
        state["i"] = i + 1
        if world == 1:
            if fn is not None:
                state["last"] = fn(xs[i % NROT])
            else:
                state["last"] = ex(xs[i % NROT], mu, sigma)[0]
            return None
        ex(xs[i % NROT], mu, sigma, out=[slots[i % R]])
        state["last"] = slots[i % R]
        if (i + 1) % BUCKET == 0:
            lo = (i + 1 - BUCKET) % R
            _, hs = reducer(ring[lo:lo + BUCKET], async_op=True)
            return hs[0]
        return None

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # correctness of the benchmarked path against an fp64 restatement on the same data
    if args.full:
        for xk in (xs[0], xs[-1]):
            (out,) = ex(xk, mu, sigma)
            want = torch.exp(-(xk - 0.1) ** 2 / (2 * 1.3 ** 2)).sum()
            rel = abs(out.item() - want.item()) / abs(want.item())
            assert rel < 1e-9, f"benchmark result mismatch: rel err {rel}"
        del want

    transport_error = None
    if world > 1 and comm_kind == "abi":
        def first_exchange():
            for _ in range(BUCKET):
                step()
        transport_error = guard_first_exchange(first_exchange, group, C, lib, check, torch, dist, rank)
        if transport_error is not None:
            group, comm_kind = dist.group.WORLD, "torch"
            transport = "torch.distributed (%s); C-ABI communicator gave up: %s" % (dist.get_backend(),
                                                                                   transport_error)
            reducer = ShardedFunction(lambda bucket: [bucket], kinds, group=None)
            state["i"] = 0

    stream = timer.stream()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    check(lib.ahip_event_create(C.byref(ev0)))
    check(lib.ahip_event_create(C.byref(ev1)))

    h = None
    for _ in range(args.warmup):
        h = step()
    if h is not None:
        h.wait()
    # clock warm-up (untimed, on top of the W warm-up steps): the driver's region is K = 20 evals
    # (0.6 ms) — measured right behind an idle period it runs 1.5-3 us per eval slower than the
    # same step sustained (r04 sweep: 30.4-33 vs 28.1 us), because the chip has not ramped its
    # clocks yet.  ~60 ms of the same step first; the timed region itself is unchanged
    # (barrier + synchronize, exactly K steps, barrier + synchronize).
    CLOCK_WARMUP = 0 if args.no_clock_warmup else 2048
    # (no garbage-collector pause inside or IN FRONT OF a 0.6 ms region: collected and switched off
    # before the clock warm-up, as ``timeit`` does — a full collection between the warm-up and the
    # timed region walks every object the golden plans loaded, tens of ms in which the chip idles
    # and drops its clocks again: r04, 28 -> 37-42 us per eval once the golden set had grown)
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()
    for _ in range(CLOCK_WARMUP):
        h = step()
        if h is not None:
            h.wait()
    if CLOCK_WARMUP and world == 1:
        # ... and the region's own shape a few times (drain, then K steps from an idle queue): the
        # first K-step window behind the long warm-up read 0.5-1 us per eval slower than the ones
        # after it (r04, AESARA_BENCH_REGIONS=8: 28.8-29.0 vs 27.5-28.6 us)
        for _ in range(3):
            barrier()
            for _ in range(args.steps):
                step()
    state["i"] = ((state["i"] + BUCKET - 1) // BUCKET) * BUCKET if world > 1 else state["i"]

    barrier()
    t0 = time.perf_counter()
    check(lib.ahip_event_record(ev0, stream))
    handles = []
    for _ in range(args.steps):
        h = step()
        if h is not None:
            handles.append(h)
            if len(handles) > 2:   # <= 3 buckets (24 evals) in flight: ring slots never reused early
                handles.pop(0).wait()
    check(lib.ahip_event_record(ev1, stream))
    for h in handles:
        h.wait()
    barrier()
    t1 = time.perf_counter()
    gc.enable()
    ms = C.c_float()
    check(lib.ahip_event_elapsed_ms(ev0, ev1, C.byref(ms)))
    if os.environ.get("AESARA_BENCH_REGIONS"):
        # (diagnostic) the same K-step region again, several times: spread of the short window
        reg = []
        for _r in range(int(os.environ["AESARA_BENCH_REGIONS"])):
            barrier()
            ta = time.perf_counter()
            check(lib.ahip_event_record(ev0, stream))
            for _ in range(args.steps):
                step()
            check(lib.ahip_event_record(ev1, stream))
            barrier()
            tb = time.perf_counter()
            m2 = C.c_float()
            check(lib.ahip_event_elapsed_ms(ev0, ev1, C.byref(m2)))
            reg.append((round(m2.value / args.steps * 1e3, 2), round((tb - ta) / args.steps * 1e6, 2)))
        print("regions (event us/eval, wall us/eval): first %.2f / %.2f, then %s"
              % (ms.value / args.steps * 1e3, (t1 - t0) / args.steps * 1e6, reg), file=sys.stderr)

    elapsed = torch.tensor([t1 - t0], dtype=f64, device="cuda")
    if world > 1:
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = elapsed.item()

    if args.dump_outputs and rank == 0:
        # what the last timed step returned (a borrowed output buffer is overwritten by the legs
        # below, so it is copied out now)
        os.makedirs(args.dump_outputs, exist_ok=True)
        last = torch.as_tensor(state["last"]).detach().to("cpu", torch.float64).numpy()
        np.save(os.path.join(args.dump_outputs, "gauss_sum.npy"), last)

    # the driver's --steps may be small (20 evals = 0.55 ms): a longer untimed-by-contract run
    # of the same step gives the sustained figure next to it
    sustained = warm = through = exec_level = None
    if world == 1 and not args.full:
        through = fn_info
    elif world == 1:
        n_long = max(args.steps, 2000)
        state["i"] = 0
        d_ms, w_ms = timer.time(step, n_long, warmup=NROT)
        sustained = {"evals": n_long, "kernel_ms": d_ms, "evals_per_s": 1e3 / max(d_ms, w_ms),
                     "frac": ALGO_BYTES / (d_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                     "note": "same rotation over %d buffers, longer run" % NROT}
        if fn is not None:
            # the same rotation through the bare executor (no Function.__call__ around it)
            est = {"i": 0}

            def estep():
                est["i"] += 1
                ex(xs[est["i"] % NROT], mu, sigma)
            d2, w2 = timer.time(estep, n_long, warmup=NROT)
            exec_level = {"evals": n_long, "kernel_ms": d2, "evals_per_s": 1e3 / max(d2, w2),
                          "frac": ALGO_BYTES / (d2 * 1e-3) / 1e9 / HBM_PEAK_GBS,
                          "note": "PlanExecutor called directly (borrowed outputs), same rotation"}
            # host cost of one call alone: the same calls with nothing to wait for in between
            t0h = time.perf_counter()
            for _ in range(200):
                step()
            host_us = (time.perf_counter() - t0h) / 200 * 1e6
            torch.cuda.synchronize()
            through = dict(fn_info, evals_per_s=sustained["evals_per_s"], kernel_ms=sustained["kernel_ms"],
                           frac=sustained["frac"], host_us_per_call=host_us)
        elif fn_info is not None:
            through = fn_info
        # the figure of rounds 1-2: ONE 128 MiB buffer re-read every eval, i.e. partly served by the
        # 256 MiB memory-side cache (MALL) — an L2-fabric number, not an HBM number
        if not args.no_warm:
            d_ms, w_ms = timer.time(lambda: ex(x, mu, sigma), n_long, warmup=20)
            warm = {"evals": n_long, "kernel_ms": d_ms, "evals_per_s": 1e3 / max(d_ms, w_ms),
                    "frac": ALGO_BYTES / (d_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "note": "same buffer every eval (MALL-assisted); not the roofline figure"}

    # what the hardware allows at this size with this launch shape: the same rotation through a
    # kernel that only loads and sums (no exp, no division) — the read-only ceiling of the headline
    ceiling = None
    if world == 1 and args.full:
        from aesara_amd.plan import Plan
        exs = PlanExecutor(Plan.from_json(SUM_PLAN), use_graph=G, borrow=True)
        (o,) = exs(xs[0])
        want = xs[0].sum().item()
        assert abs(o.item() - want) <= 1e-9 * abs(want) + 1e-6, "sum kernel mismatch"
        cstate = {"i": 0}

        def cstep():
            i = cstate["i"]
            cstate["i"] = i + 1
            exs(xs[i % NROT])
        d_ms, w_ms = timer.time(cstep, max(args.steps, 2000), warmup=NROT)
        ceiling = {"kernel_ms": d_ms, "frac": ALGO_BYTES / (d_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                   "achieved_GBs": ALGO_BYTES / (d_ms * 1e-3) / 1e9,
                   "note": "x.sum() of the same matrices, same rotation, same launch shape: loads + "
                           "adds only (no ALU work to hide), in-kernel finalize included"}
        del exs

    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        # compiles the reference's C modules in the background while the secondary rows run — started
        # only now, behind every leg that is paced by host calls of a few microseconds: a few hundred
        # gcc processes next to the headline's 0.6 ms timed region cost it 4 us per eval (r04: 32.8 vs
        # 28.5 us on the same box), next to the executor-level and read-only-ceiling legs half their
        # rate (0.27 / 0.29 instead of 0.62 / 0.67)
        ref_warm = start_reference_warm()

    secondary = []
    if args.full and not args.no_secondary:
        only = [s for s in args.only_secondary.split(",") if s]
        ctx = dict(torch=torch, np=np, dist=dist, timer=timer, plan_of=plan_of, randn=randn,
                   PlanExecutor=PlanExecutor, G=G, rank=rank, world=world, args=args,
                   group=group, comm_kind=comm_kind, transport=transport)
        for name, fn in SECONDARY:
            if only and name not in only:
                continue
            if world > 1 and name == "cfg4":
                # config 4 with a matrix state shards along the batch: strong scaling,
                # no collective on the data path.  Guarded: an extra row must never cost the line.
                # (no collective inside the guarded part: a rank that fails must not leave the
                # others waiting; the two all-reduces below are reached by every rank)
                try:
                    r, dw = sec_cfg4_sharded(ctx), None
                    dw = [r["ms_per_eval"], 1e3 / r["evals_per_s"]]
                except Exception as e:              # noqa: BLE001
                    r = {"config": "cfg4 Scan GRU B=64 batch-sharded", "error": "%s: %s" % (type(e).__name__, e)}
                ok = torch.tensor([0.0 if dw is None else 1.0], dtype=torch.float64, device="cuda")
                dist.all_reduce(ok, op=dist.ReduceOp.MIN)
                t = torch.tensor(dw or [0.0, 0.0], dtype=torch.float64, device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                if ok.item() == 1.0:
                    d_, w_ = t.tolist()
                    r["ms_per_eval"], r["evals_per_s"] = d_, 1e3 / max(d_, w_)
                    r["roofline"] = roof("mfma", r["roofline"]["algorithmic"], d_, MFMA_F32_PEAK,
                                         us_per_step=d_ * 1e3 / 512,
                                         note="per-rank flops; kernel_ms is the max over the ranks")
                elif "error" not in r:
                    r = {"config": r["config"], "error": "another rank failed"}
                if rank == 0:
                    secondary.append(r)
                torch.cuda.empty_cache()
                continue
            if world > 1 and name not in ("cfg5", "placed"):
                continue              # replicas only: measured at N=1
            if name == "placed":
                # guarded like the sharded config-4 row: an extra row must never cost the line
                # (its two collectives — barrier, max of the times — are reached by every rank
                # only when the guarded part succeeded everywhere)
                try:
                    r, ms_ = fn(ctx), None
                    ms_ = r["ms_per_eval"]
                except Exception as e:              # noqa: BLE001
                    r = {"config": "placed outputs", "error": "%s: %s" % (type(e).__name__, e)}
                if world > 1:
                    t = torch.tensor([0.0 if ms_ is None else 1.0, ms_ or 0.0], dtype=torch.float64,
                                     device="cuda")
                    tmin, tmax = t.clone(), t.clone()
                    dist.all_reduce(tmin, op=dist.ReduceOp.MIN)
                    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
                    if tmin[0].item() == 1.0:
                        r["ms_per_eval"] = tmax[1].item()
                        r["evals_per_s"] = 1e3 / r["ms_per_eval"]
                    elif "error" not in r:
                        r = {"config": r["config"], "error": "another rank failed"}
                if rank == 0:
                    secondary.append(r)
                torch.cuda.empty_cache()
                continue
            r = fn(ctx)
            if rank == 0:
                secondary.extend(r if isinstance(r, list) else [r])
            torch.cuda.empty_cache()

    if rank == 0:
        dev_ms_per_eval = ms.value / args.steps          # device time per eval on the stream
        achieved = ALGO_BYTES / (dev_ms_per_eval * 1e-3) / 1e9
        traffic, traffic_src = measured_traffic()
        res = {
            "metric": "compiled-fn evals/sec + achieved HBM GB/s (elemwise) / MFMA % (gemm), 1->8 GPU",
            "value": args.steps * world / elapsed,
            "unit": "evals/s",
            "n_gpus": world,
            "ranks_seen": dist.get_world_size() if world > 1 else 1,   # what the process group reports
            "transport": transport,                                    # which exchange path ran (N > 1)
            "ranks_seen": world if world == 1 else (group.world if comm_kind == "abi" else dist.get_world_size()),
            "transport_error": transport_error,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: fused Elemwise exp(-(x-mu)^2/2sigma^2).sum(), "
                                   "fp64 4096x4096 per GPU, inputs resident in HBM (rotating over %d "
                                   "distinct 128 MiB matrices: MALL-cold), launch-list replay, "
                                   "outputs borrowed (Out(borrow=True): function-owned buffers)" % NROT,
                       "rows_per_gpu": ROWS, "cols": COLS, "rotate": NROT,
                       "clock_warmup_evals": CLOCK_WARMUP,
                       # north_star: >= 60 % of the HBM roofline on this graph.  Met on a cache-warm
                       # input (config.warm), NOT on MALL-cold inputs (DESIGN §5 says why)
                       "target_frac": 0.60, "target_met_cold": bool(achieved / HBM_PEAK_GBS >= 0.60),
                       "warm": warm, "executor_level": exec_level, "read_only_ceiling": ceiling,
                       "headline_path": "aesara.function(mode='HIP') -> Function.__call__ (untrusted: its own "
                                        "input filter, device tensors in / out)" if fn is not None
                                        else "PlanExecutor (no reference front end here, N > 1, or "
                                             "--executor-level)",
                       "parallelism": "row-sharded x%d, bucketed async RCCL all-reduce of the CAReduce "
                                      "partials (8 evals per collective)" % world
                                      if world > 1 else "single GPU",
                       "sustained": sustained},
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "kernel_ms": dev_ms_per_eval, "algorithmic_bytes": ALGO_BYTES},
        }
        if through is not None:
            res["through_function"] = through    # top level: the driver's record keeps top-level keys
        if secondary:
            res["secondary"] = secondary
        if world == 1 and args.full and not args.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(np, ref_warm, secondary)
            vs = res["cpu_baseline"].pop("vs_reference", None)
            if vs is not None:
                res["vs_reference"] = vs        # top level: the driver's record keeps top-level keys
        print(json.dumps(res))
    if world > 1:
        if comm_kind == "abi":
            group.close(force=True)
        dist.destroy_process_group()


SUM_PLAN = {"version": 1, "name": "sum_all_f64",
            "vars": [{"id": 0, "dtype": "float64", "shape": [None, None], "name": "x"},
                     {"id": 1, "dtype": "float64", "shape": []}],
            "inputs": [0], "outputs": [1],
            "nodes": [{"op": "CAReduce", "inputs": [0], "outputs": [1],
                       "params": {"scalar_op": "add", "axis": None, "acc_dtype": "float64"}}]}


# ---------------------------------------------------------------------------------------------
# secondary workloads: the other BASELINE configs at full shape
# ---------------------------------------------------------------------------------------------

def sec_cfg3b(c):
    """Gemm fp32 4096^3 through the plan the linker lowers for check_blas.py:54-57's update."""
    torch = c["torch"]
    f32 = torch.float32
    ex = c["PlanExecutor"](c["plan_of"]("cfg3b_gemm_update"), use_graph=c["G"], borrow=True)
    Cm = c["randn"]((4096, 4096), f32, 1)
    A, B = c["randn"]((4096, 4096), f32, 3), c["randn"]((4096, 4096), f32, 4)
    (out,) = ex(Cm, A, B)
    ref = 0.4 * Cm.double() + 0.8 * (A.double() @ B.double())
    rel = (torch.linalg.norm(out.double() - ref) / torch.linalg.norm(ref)).item()
    assert rel <= 1e-6, f"cfg3b Frobenius rel err {rel}"
    del ref
    rows = []
    for name, a, b in (("NN", A, B), ("NT", A, B.t()), ("TN", A.t(), B), ("TT", A.t(), B.t())):
        # 40 untimed evals (~45 ms) first: the first MFMA-heavy launches after the light config-2
        # run are 7 % slower (1.18 vs 1.10 ms, tools/gemm_layout_order.py: whichever layout is
        # measured first pays it) — the timed region is the steady state
        d, w = c["timer"].time(lambda: ex(Cm, a, b), 30, warmup=40)
        rows.append({"config": "cfg3b Gemm fp32 4096^3 0.4*C+0.8*A@B (%s)" % name, "dtype": "f32",
                     "evals_per_s": 1e3 / max(d, w),
                     "roofline": roof("mfma", 2 * 4096 ** 3, d, MFMA_F32_PEAK,
                                      kernel="gemm.hip 128x128 v_mfma_f32_16x16x4_f32"),
                     "check": {"frobenius_rel_err_vs_fp64": rel, "bar": 1e-6} if name == "NN" else None})
    return rows


GEMM_SHAPES = (
    # (row key = time_reference.py config, kind, shape, what)
    ("bdot_64x512", "BatchedDot", (64, 512, 512, 512), "64 x (512x512x512)"),
    ("bdot_1024x64", "BatchedDot", (1024, 64, 64, 64), "1024 x (64x64x64)"),
    ("dot22_tall", "Dot22", (16384, 64, 1024), "16384x64x1024"),
    ("dot22_wide", "Dot22", (64, 16384, 1024), "64x16384x1024"),
)


def sec_gemmshapes(c):
    """BatchedDot (tensor/blas.py:2179) and Dot22 (:1659) away from the square headline: fp32, the
    shapes VERDICT r5 names.  Each row is priced against the roof that bounds it: the MFMA peak
    when the operands are re-used (2 M N K / 157.3 TFLOP/s), the HBM peak when the products are so
    small that the operand bytes dominate (1024 x 64^3: 10.7 flop per byte < 157.3 / 8 = 19.7)."""
    torch = c["torch"]
    f32 = torch.float32
    from aesara_amd.dist import subplan_for_outputs
    rows = []
    for key, kind, shp, what in GEMM_SHAPES:
        if kind == "BatchedDot":
            Bn, M, N, K = shp
            plan = c["plan_of"]("batched_dot_f32")
            A, B = c["randn"]((Bn, M, K), f32, 11), c["randn"]((Bn, K, N), f32, 12)
            flops, byts = 2.0 * Bn * M * N * K, 4.0 * Bn * (M * K + K * N + M * N)
            ref = torch.bmm(A.double(), B.double())
        else:
            M, N, K = shp
            plan = subplan_for_outputs(c["plan_of"]("dot22_f32"), [0])
            A, B = c["randn"]((M, K), f32, 13), c["randn"]((K, N), f32, 14)
            flops, byts = 2.0 * M * N * K, 4.0 * (M * K + K * N + M * N)
            ref = A.double() @ B.double()
        ex = c["PlanExecutor"](plan, use_graph=c["G"], borrow=True)
        (out,) = ex(A, B)
        rel = (torch.linalg.norm(out.double() - ref) / torch.linalg.norm(ref)).item()
        assert rel <= 1e-6, f"{kind} {what}: Frobenius rel err {rel}"
        del ref
        d, w = c["timer"].time(lambda: ex(A, B), 50, warmup=20)
        mfma_ms = flops / (MFMA_F32_PEAK * 1e12) * 1e3
        hbm_ms = byts / (HBM_PEAK_GBS * 1e9) * 1e3
        if hbm_ms > mfma_ms:
            r = roof("hbm", byts, d, HBM_PEAK_GBS, kernel="gemm.hip", mfma_frac=flops / (d * 1e-3) / 1e12 / MFMA_F32_PEAK,
                     note="operand bytes bound this shape: %.1f flop per byte < %.1f = MFMA peak / HBM peak"
                          % (flops / byts, MFMA_F32_PEAK * 1e3 / HBM_PEAK_GBS))
        else:
            r = roof("mfma", flops, d, MFMA_F32_PEAK, kernel="gemm.hip",
                     hbm_frac=byts / (d * 1e-3) / 1e9 / HBM_PEAK_GBS)
        rows.append({"config": "%s fp32 %s" % (kind, what), "key": key, "dtype": "f32",
                     "evals_per_s": 1e3 / max(d, w), "roofline": r,
                     "check": {"frobenius_rel_err_vs_fp64": rel, "bar": 1e-6}})
        del ex, A, B, out
        torch.cuda.empty_cache()
    return rows



def sec_cfg3a(c):
    torch = c["torch"]
    f64 = torch.float64
    # BASELINE configs[2]'s graph: ``M.dot(v) + a`` as the linker lowers it (golden cfg3a_gemv,
    # second output: AllocEmpty -> Gemv(beta = 0) -> Elemwise add of the broadcast scalar) — the
    # plan tests/refcheck.py checks against the reference is the plan that is timed
    from aesara_amd.dist import subplan_for_outputs
    plan = subplan_for_outputs(c["plan_of"]("cfg3a_gemv"), [1])
    ex = c["PlanExecutor"](plan, use_graph=c["G"], borrow=True)
    M = c["randn"]((4096, 4096), f64, 2)
    v, a = c["randn"]((4096,), f64, 3), torch.tensor(2.0, dtype=f64, device="cuda")
    (out,) = ex(M, v, a)
    ref = M @ v + a
    err = ((out - ref).abs().max() / ref.abs().max()).item()
    assert err <= 1e-10, f"cfg3a rel err {err}"
    dw, _ = c["timer"].time(lambda: ex(M, v, a), 200)
    # rotate over 8 distinct matrices (1 GiB > the 256 MiB MALL): the HBM figure
    Ms = [M] + [c["randn"]((4096, 4096), f64, 20 + k) for k in range(7)]
    st = {"i": 0}

    def step():
        st["i"] += 1
        ex(Ms[st["i"] & 7], v, a)
    d, w = c["timer"].time(step, 200, warmup=16)
    work = 4096 * 4096 * 8 + 2 * 4096 * 8
    return {"config": "cfg3a Gemv fp64 4096^2 M.dot(v) + a (rotating over 8 matrices: MALL-cold)",
            "dtype": "f64", "evals_per_s": 1e3 / max(d, w),
            "roofline": roof("hbm", work, d, HBM_PEAK_GBS,
                             warm={"kernel_ms": dw, "frac": work / (dw * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                   "note": "same matrix every eval (MALL-assisted)"}),
            "check": {"max_rel_err_vs_fp64": err, "bar": 1e-10}}


def sec_cfg1b(c):
    torch = c["torch"]
    f64 = torch.float64
    ex = c["PlanExecutor"](c["plan_of"]("cfg1b_matrix_add"), use_graph=c["G"], borrow=True)
    x, y = c["randn"]((4096, 4096), f64, 0), c["randn"]((4096, 4096), f64, 1)
    (out,) = ex(x, y)
    assert torch.equal(out, x + y)
    d, w = c["timer"].time(lambda: ex(x, y), 200)
    return {"config": "cfg1b matrix add fp64 4096^2", "dtype": "f64", "evals_per_s": 1e3 / max(d, w),
            "roofline": roof("hbm", 3 * 4096 * 4096 * 8, d, HBM_PEAK_GBS), "check": {"exact": True}}


def _gru_ref(torch, x, h0, Ws, all_steps=False):
    """fp64 restatement of the GRU step of tests/golden cfg4 (oracle/gen_golden.py), all T steps."""
    Wz, Uz, Wr, Ur, Wh, Uh = [W.double() for W in Ws]
    h = h0.double()
    xd = x.double()
    xz, xr, xh = xd @ Wz, xd @ Wr, xd @ Wh
    hs = []
    for t in range(x.shape[0]):
        z = torch.sigmoid(xz[t] + h @ Uz)
        r = torch.sigmoid(xr[t] + h @ Ur)
        hh = torch.tanh(xh[t] + (r * h) @ Uh)
        h = (1 - z) * h + z * hh
        if all_steps:
            hs.append(h)
    return torch.stack(hs) if all_steps else h


def sec_cfg4(c):
    torch, np = c["torch"], c["np"]
    f32 = torch.float32
    T, H = 512, 1024
    rows = []
    Ws = [c["randn"]((H, H), f32, 5 + k) / np.sqrt(H) for k in range(6)]
    for B, case in ((1, "cfg4_gru_b1_f32"), (64, "cfg4_gru_b8_f32")):
        ex = c["PlanExecutor"](c["plan_of"](case), use_graph=c["G"], borrow=True)
        shp = (T, H) if B == 1 else (T, B, H)
        x = c["randn"](shp, f32, 4) * 0.1
        h0 = torch.zeros((H,) if B == 1 else (B, H), dtype=f32, device="cuda")
        t0 = time.perf_counter()
        outs = ex(x, h0, *Ws)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        hT = outs[-1].double()
        ref = _gru_ref(torch, x, h0, Ws)
        err = ((hT - ref).abs().max() / ref.abs().max()).item()
        assert err <= 1e-5, f"cfg4 B={B} h_T rel err {err}"
        d, w = c["timer"].time(lambda: ex(x, h0, *Ws), 5, warmup=1)
        kind = getattr(ex, "scan_modes", None)
        if B == 1:
            # two bounds: weights re-streamed every step vs kept on chip
            rl = latency_row(d, T, restreamed_bytes=T * 6 * H * H * 4, handoffs_per_step=2,
                             resident_bound_bytes=6 * H * H * 4 + 2 * T * H * 4)
        else:
            rl = roof("mfma", T * 6 * 2 * B * H * H, d, MFMA_F32_PEAK, us_per_step=d * 1e3 / T)
        rows.append({"config": "cfg4 Scan GRU T=512 H=1024 fp32 B=%d" % B, "dtype": "f32",
                     "evals_per_s": 1e3 / max(d, w), "first_call_s": first, "scan_path": kind,
                     "roofline": rl, "check": {"hT_max_rel_err_vs_fp64_all_steps": err, "bar": 1e-5}})
        del ex
    # the same recurrence under aesara.grad (not a BASELINE config, reported next to
    # config 4 because it is the Scan gradient path on the same kernels): loss + 7 gradients
    for B, case in ((1, "gru_bptt_b1_f32"), (64, "gru_bptt_b4_f32")):
        ex = c["PlanExecutor"](c["plan_of"](case), use_graph=c["G"], borrow=True)
        shp = (T, H) if B == 1 else (T, B, H)
        x = c["randn"](shp, f32, 4) * 0.1
        h0 = torch.zeros((H,) if B == 1 else (B, H), dtype=f32, device="cuda")
        outs = ex(x, h0, *Ws)
        hs = _gru_ref(torch, x, h0, Ws, all_steps=True)
        ref = ((hs[-1] ** 2).sum() + hs.mean()).item()
        err = abs(outs[0].item() - ref) / abs(ref)
        assert err <= 1e-4, f"cfg4 training step B={B}: loss rel err {err}"
        d, w = c["timer"].time(lambda: ex(x, h0, *Ws), 5, warmup=1)
        rows.append({"config": "cfg4 + aesara.grad: GRU training step T=512 H=1024 fp32 B=%d "
                               "(loss + 7 gradients; extra, not a BASELINE config)" % B,
                     "dtype": "f32", "evals_per_s": 1e3 / max(d, w), "ms_per_eval": d,
                     "scan_path": getattr(ex, "scan_modes", None),
                     "roofline": (roof("mfma", 3 * T * 6 * 2 * B * H * H, d, MFMA_F32_PEAK,
                                       us_per_step=d * 1e3 / T,
                                       note="flops = forward + gate recomputation + backward / weight-"
                                            "gradient products (3 x the forward count)") if B > 1 else
                                  latency_row(d, T, restreamed_bytes=3 * T * 6 * H * H * 4,
                                              handoffs_per_step=2 + 3, resident_bound_bytes=None)),
                     "check": {"loss_rel_err_vs_fp64": err, "bar": 1e-4,
                               "gradients": "tests/test_gpu_fullsize.py::test_gru_bptt_against_torch_autograd"}})
        del ex
    return rows


def sec_cfg4_sharded(c):
    """Config 4, B = 64, split along the batch over the ranks (aesara_amd/dist.py: the step is
    row-local, every rank runs the persistent loop on its B / N rows; no exchange).  Strong
    scaling: `evals_per_s` is whole-job (one eval = all 64 sequences)."""
    torch, np, dist = c["torch"], c["np"], c["dist"]
    from aesara_amd.dist import ShardedPlan, shard_rows
    f32 = torch.float32
    T, H, B = 512, 1024, 64
    world, rank = c["world"], c["rank"]
    lo, hi = shard_rows(B, world, rank)
    Ws = [c["randn"]((H, H), f32, 5 + k) / np.sqrt(H) for k in range(6)]
    x = c["randn"]((T, B, H), f32, 4)[:, lo:hi].contiguous() * 0.1
    h0 = torch.zeros((hi - lo, H), dtype=f32, device="cuda")
    sp = ShardedPlan(c["plan_of"]("cfg4_gru_b8_f32"), split_inputs={0: 1, 1: 0}, use_graph=c["G"], borrow=True,
                     group=dist.group.WORLD)
    outs = sp(x, h0, *Ws)
    ref = _gru_ref(torch, x, h0, Ws)
    err = ((outs[-1].double() - ref).abs().max() / ref.abs().max()).item()
    assert err <= 1e-5, f"cfg4 sharded: h_T rel err {err}"
    d, w = c["timer"].time(lambda: sp(x, h0, *Ws), 5, warmup=1)       # local; combined by the caller
    return {"config": "cfg4 Scan GRU T=512 H=1024 fp32 B=64 batch-sharded, %d rank(s) x %d rows, strong scaling"
                      % (world, hi - lo), "dtype": "f32", "n_gpus": world, "scaling": "strong",
            "evals_per_s": 1e3 / max(d, w), "ms_per_eval": d, "collective": "none on the data path",
            "roofline": roof("mfma", T * 6 * 2 * (hi - lo) * H * H, d, MFMA_F32_PEAK, us_per_step=d * 1e3 / T,
                             note="per-rank flops; kernel_ms is the max over the ranks"),
            "check": {"hT_max_rel_err_vs_fp64_local_rows": err, "bar": 1e-5}}


def sec_cfg5(c):
    """Config 5 at full shape, row-sharded over the ranks (strong scaling): every rank runs the
    single-pass row program on its 2^k/N rows, ONE all-reduce sums the 258 accumulator-dtype
    partials (aesara_amd/dist.py), the casts to the output dtype happen after it."""
    torch, dist = c["torch"], c["dist"]
    f32 = torch.float32
    world, rank = c["world"], c["rank"]
    N, D = 1 << c["args"].cfg5_log2n, 256
    n_loc = N // world
    g = torch.Generator(device="cuda")
    g.manual_seed(6 + 1000 * rank)
    X = torch.empty((n_loc, D), dtype=f32, device="cuda")
    blk = 1 << 20
    for i in range(0, n_loc, blk):
        X[i:i + blk] = torch.randn((min(blk, n_loc - i), D), dtype=f32, device="cuda", generator=g)
    gw_ = torch.Generator(device="cuda")
    gw_.manual_seed(7)
    wv = torch.randn((D,), dtype=f32, device="cuda", generator=gw_) / 16
    b = torch.tensor(0.1, dtype=f32, device="cuda")
    yv = (torch.rand(n_loc, device="cuda", generator=g) < 0.5).to(f32)

    from aesara_amd.dist import HipComm, ShardedPlan
    group, comm_kind = c["group"], c["comm_kind"]
    sp = ShardedPlan(c["plan_of"]("cfg5_logistic"), split_inputs={0: 0, 3: 0}, use_graph=c["G"], borrow=True,
                     group=group)
    outs = sp(X, wv, b, yv)
    torch.cuda.synchronize()
    logp, gw, gb = [o.clone() for o in outs]
    # fp64 restatement in row blocks (local rows), summed over the ranks
    acc = torch.zeros(D + 2, dtype=torch.float64, device="cuda")
    for i in range(0, n_loc, 1 << 21):
        Xd = X[i:i + (1 << 21)].double()
        yd = yv[i:i + (1 << 21)].double()
        z = Xd @ wv.double() + 0.1
        acc[0] += -(yd * torch.nn.functional.softplus(-z) + (1 - yd) * torch.nn.functional.softplus(z)).sum()
        r = yd - torch.sigmoid(z)
        acc[1] += r.sum()
        acc[2:] += Xd.t() @ r
        del Xd, yd, z, r
    if world > 1:
        dist.all_reduce(acc)
    e_logp = abs(logp.item() - acc[0].item()) / abs(acc[0].item())
    e_gb = abs(gb.item() - acc[1].item()) / max(abs(acc[1].item()), 1.0)
    e_gw = (torch.linalg.norm(gw.double() - acc[2:]) / torch.linalg.norm(acc[2:])).item()
    assert e_logp <= 1e-6 and e_gw <= 1e-5, (e_logp, e_gb, e_gw)

    iters = 20
    for _ in range(3):
        sp(X, wv, b, yv)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    d, w = c["timer"].time(lambda: sp(X, wv, b, yv), iters, warmup=0)
    t = torch.tensor([max(d, w)], dtype=torch.float64, device="cuda")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ms_job = t.item()
    local_bytes = n_loc * D * 4 + n_loc * 4
    return {"config": "cfg5 logistic logp+grad fp32 N=2^%d D=256, %d rank(s) x %d rows, strong scaling"
                      % (c["args"].cfg5_log2n, world, n_loc),
            "dtype": "f32", "n_gpus": world, "scaling": "strong",
            "evals_per_s": 1e3 / ms_job, "ms_per_eval": ms_job,
            "collective": None if world == 1 else "1 all-reduce(sum) of 258 fp64 per eval",
            "transport": None if world == 1 else (
                c["transport"] + (", %d of %d evals were single-list replays" % (sp.replays, iters + 4)
                                  if comm_kind == "abi" else "")),
            "ranks_seen": world if world == 1 else (group.world if comm_kind == "abi" else dist.get_world_size()),
            "aggregate_GBs": world * local_bytes / (ms_job * 1e-3) / 1e9,
            "roofline": roof("hbm", local_bytes, d, HBM_PEAK_GBS,
                             note="per-rank: local X once + y; kernel_ms includes the collective for N>1"),
            "check": {"logp_rel_err": e_logp, "gb_rel_err": e_gb, "gw_rel_err": e_gw,
                      "bars": [1e-6, 1e-6, 1e-5]}}


def sec_placed(c):
    """north_star: "independent graph outputs shard embarrassingly across the 8 GPUs".  ONE plan
    with 8 independent towers (output k = sum(exp(-0.5 * x_k**2)), x_k fp64 2048x2048 = 32 MiB)
    through ``dist.PlacedPlan``: every rank evaluates only the towers ``place_outputs`` gave it,
    no communication on the data path.  Strong scaling: the job is always the 8 towers."""
    torch, dist = c["torch"], c["dist"]
    from aesara_amd.dist import PlacedPlan
    from aesara_amd.plan import Node, Plan
    f64 = torch.float64
    world, rank = c["world"], c["rank"]
    NT, R = 8, 2048
    p = Plan("towers", {}, [], [], [])
    for k in range(NT):
        x = p.new_var("float64", [None, None], "x%d" % k)
        e = p.new_var("float64", [None, None])
        o = p.new_var("float64", [])
        p.inputs.append(x)
        p.outputs.append(o)
        p.nodes.append(Node("Elemwise", [x], [e], {"scalar": {"n_in": 1, "nodes": [
            {"op": "sqr", "in": [["i", 0]], "dtype": "float64"},
            {"op": "mul", "in": [["c", -0.5, "float64"], ["t", 0]], "dtype": "float64"},
            {"op": "exp", "in": [["t", 1]], "dtype": "float64"}], "out": [["t", 2]]}}))
        p.nodes.append(Node("CAReduce", [e], [o], {"scalar_op": "add", "axis": None, "acc_dtype": "float64"}))
    pp = PlacedPlan(p, world, rank, use_graph=c["G"])
    # inputs of towers other ranks own are never read: a placeholder keeps the signature
    xs = [c["randn"]((R, R), f64, 40 + k) if k in pp.mine else torch.zeros((1, 1), dtype=f64, device="cuda")
          for k in range(NT)]
    outs = pp(*xs)
    for k in pp.mine:
        ref = torch.exp(-0.5 * xs[k] ** 2).sum().item()
        assert abs(outs[k].item() - ref) <= 1e-9 * abs(ref), (k, outs[k].item(), ref)
    assert all(outs[k] is None for k in range(NT) if k not in pp.mine)
    torch.cuda.synchronize()
    d, w = c["timer"].time(lambda: pp(*xs), 200, warmup=5)     # local; max over ranks by the caller
    ms_job = max(d, w)
    local_bytes = len(pp.mine) * R * R * 8
    return {"config": "placed outputs: 8 independent fp64 2048^2 exp-sum towers in ONE plan, %d rank(s), "
                      "%s towers on this rank, strong scaling" % (world, len(pp.mine)),
            "dtype": "f64", "n_gpus": world, "scaling": "strong", "collective": "none",
            "placement": pp.placement, "evals_per_s": 1e3 / ms_job, "ms_per_eval": ms_job,
            "roofline": roof("hbm", local_bytes, d, HBM_PEAK_GBS,
                             note="per-rank bytes of the towers it owns; kernel_ms = this rank")}


SECONDARY = [("cfg3b", sec_cfg3b), ("gemmshapes", sec_gemmshapes), ("cfg3a", sec_cfg3a), ("cfg1b", sec_cfg1b), ("cfg4", sec_cfg4),
             ("cfg5", sec_cfg5), ("placed", sec_placed)]


def measured_traffic():
    """HBM bytes per launch of the dominant kernel from rocprofv3 PMC passes of this command
    (separate `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` runs, tools/profile_bench.sh; FETCH_SIZE
    doubled per the gfx950 correction of MI355X_MICROARCH.md §HBM).  Counters cannot be read
    inside an unprofiled run, so the figure comes from the newest committed pass; null if none."""
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_traffic.json")), reverse=True):
        try:
            with open(path) as f:
                return json.load(f)["hbm_bytes_per_launch"], os.path.relpath(path, ROOT)
        except Exception:
            continue
    return None, None


def start_reference_warm():
    """Kick off (in the background) a child that compiles the reference's C modules for every
    config into its compile cache, so the timed child at the end of the run only loads them."""
    try:
        import ref_overlay
        if not ref_overlay.available():
            return None
        import subprocess
        env = dict(os.environ)
        env.pop("AESARA_FLAGS", None)
        # the child only compiles (tiny shapes): one BLAS / OpenMP thread — at their defaults the
        # tiny warm-up evaluations spin 256 threads next to the rows being measured (r04: Gemm rows
        # 0.75 instead of 0.80 while it ran) — and the lowest scheduling priority
        for k in ("OPENBLAS_NUM_THREADS", "OMP_NUM_THREADS", "MKL_NUM_THREADS"):
            env[k] = "1"
        return subprocess.Popen([sys.executable, os.path.join(ROOT, "oracle", "time_reference.py"), "--warm"],
                                stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, env=env,
                                preexec_fn=lambda: os.nice(19))
    except Exception:                                   # noqa: BLE001
        return None


def reference_rows(budget, configs, openmp=False, timeout=420, dump_dir=None, full=False):
    import subprocess
    env = dict(os.environ)
    env.pop("AESARA_FLAGS", None)
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "time_reference.py"), "--budget", str(budget),
           "--configs", ",".join(configs)] + (["--openmp"] if openmp else []) + \
        (["--dump-dir", dump_dir] if dump_dir else []) + (["--full"] if full else [])
    p = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout)
    line = next((ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if line is None:
        raise RuntimeError("time_reference.py gave no result: " + (p.stderr or p.stdout)[-400:])
    return json.loads(line[7:])


def full_shape_reference_check(refcheck):
    """Configs 4 (B = 1 and B = 64, T = 512) and 5 (N = 2^24, 16 GiB of X) ONCE through the
    reference's C linker on this host, then the HIP path on the same seeded inputs.  One child per
    config (bounded: a slow host costs that config's check, not the line); config 5 needs ~40 GiB
    of free host memory (X in the child and again here for the upload) and is skipped below that."""
    import shutil
    import tempfile
    out = {}
    for cfg, limit in (("cfg4_b1", 240), ("cfg4_b64", 420), ("cfg5", 600)):
        if cfg == "cfg5":
            try:
                with open("/proc/meminfo") as f:
                    avail = next(int(ln.split()[1]) for ln in f if ln.startswith("MemAvailable")) >> 20
            except Exception:                           # noqa: BLE001
                avail = 0
            if avail < 40:
                raise RuntimeError("cfg5 at N = 2^24 needs ~40 GiB of free host memory, %d GiB available"
                                   % avail)
        dump = tempfile.mkdtemp(prefix="aesara_ref_full_")
        try:
            r = reference_rows(0.0, [cfg], timeout=limit, dump_dir=dump, full=True)
            row = r["rows"][cfg]
            if "error" in row:
                raise RuntimeError("%s: %s" % (cfg, row["error"]))
            got = refcheck.hip_vs_reference(dump, [cfg], full=True)
            got[cfg]["reference_ms_full_shape"] = row.get("ms_per_eval")
            out.update(got)
        finally:
            shutil.rmtree(dump, ignore_errors=True)
    return out


def make_function(x0, torch, np):
    """The headline workload through the REAL front end: ``aesara.function([x, mu, sigma], expr,
    mode="HIP")``; returns (callable taking the device matrix, info) — the callable is an ordinary
    UNTRUSTED ``Function.__call__`` (types.py:791-1082: its own input filter — a device tensor is
    filtered on the device by ``devcell.DeviceFilterType`` — then HipLinker's VM -> PlanExecutor
    replay -> ``ahip_list_run_rebased``; mu / sigma are host scalars as a user passes them; the
    result is a fresh device tensor).  (None, why) when the front end is not available here."""
    try:
        import ref_overlay
        if not ref_overlay.available():
            return None, None
        ae = ref_overlay.import_reference()
        import aesara.tensor as at
        import aesara_amd
        aesara_amd.get_mode()
        x, mu, sg = at.dmatrix("x"), at.dscalar("mu"), at.dscalar("sigma")
        f = ae.function([x, mu, sg], at.exp(-(x - mu) ** 2 / (2 * sg ** 2)).sum(), mode="HIP")
        assert f.trust_input is False
        m, s_ = np.asarray(0.1), np.asarray(1.3)
        out = f(x0, m, s_)
        want = torch.exp(-(x0 - 0.1) ** 2 / (2 * 1.3 ** 2)).sum()
        rel = abs(out.item() - want.item()) / abs(want.item())
        assert rel < 1e-9, rel
        info = {"path": "aesara.function(mode='HIP') -> Function.__call__ (trust_input=False: "
                        "DeviceFilterType) -> HipLinker fast VM -> PlanExecutor replay -> "
                        "ahip_list_run_rebased; fresh outputs",
                "trust_input": False, "rel_err_vs_fp64": rel, "front_end": ref_overlay.source()}
        return (lambda xd: f(xd, m, s_)), info
    except Exception as e:                              # noqa: BLE001  (fall back to the executor)
        return None, {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}


def cpu_baseline(np, ref_warm=None, secondary=None):
    """The reference's own C linker on this host when its front end is available (child process,
    bounded: <= ~6 s of evals per config), else the oracle's C port of the same loops."""
    res = None
    try:
        import ref_overlay
        have = ref_overlay.available()
    except Exception:                                   # noqa: BLE001
        have = False
    if have:
        try:
            if ref_warm is not None:
                ref_warm.wait(timeout=300)
            import tempfile
            dump = tempfile.mkdtemp(prefix="aesara_ref_out_")
            r = reference_rows(4.0, ["cfg2", "cfg1b", "cfg3a", "cfg3b", "cfg4_b1", "cfg4_b64", "cfg5"]
                               + [k for k, *_ in GEMM_SHAPES], dump_dir=dump, timeout=600)
            row = r["rows"]["cfg2"]
            res = {"value": 1e3 / row["ms_per_eval"], "unit": "evals/s", "cores": row["cores"],
                   "kind": "reference", "ms_per_eval": row["ms_per_eval"],
                   "sample": "%d evals of the same %s with the reference's Mode('cvm','fast_run') C linker "
                             "(trust_input, median)" % (row["evals"], row["sample"]),
                   "host_cores_visible": r["host"]["nproc"], "front_end": r["source"],
                   "threads": "Elemwise/CAReduce loops single-threaded (openmp=False, the reference default); "
                              "BLAS rows: bundled OpenBLAS at its default thread count",
                   "graph": row.get("nodes")}
            scale = {"cfg4_b1": 8.0, "cfg4_b64": 8.0, "cfg5": 16.0}
            others = {}
            for k, v in r["rows"].items():
                if k == "cfg2":
                    continue
                if "ms_per_eval" in v:
                    others[k] = {"ms_per_eval_full_config": v["ms_per_eval"] * scale.get(k, 1.0),
                                 "measured_ms": v["ms_per_eval"], "evals": v["evals"], "cores": v["cores"],
                                 "sample": v["sample"]}
                else:
                    others[k] = v
            res["other_configs"] = others
            # the HIP path on the SAME seeded inputs against what the reference's C linker returned
            # (full BASELINE shapes for cfg 1b / 2 / 3a / 3b, the timed samples for cfg 4 / 5):
            # north_star "results equal to the C linker within 1e-6 rel"
            try:
                import shutil
                import refcheck
                vs = refcheck.hip_vs_reference(dump)
                shutil.rmtree(dump, ignore_errors=True)
                sampled = {k: v["max"] for k, v in vs.items() if not v["full_shape"]}
                # configs 4 and 5 are TIMED on samples (T = 64 of 512 steps, 2^20 of 2^24 rows);
                # their RESULTS are checked at BASELINE's full shapes: the reference evaluates each
                # once (SURVEY §8d "run it once"), the HIP path runs the same seeded inputs
                full_note = None
                if not os.environ.get("AESARA_BENCH_NO_FULL_REFERENCE"):
                    try:
                        vs.update(full_shape_reference_check(refcheck))
                    except Exception as e:              # noqa: BLE001
                        full_note = "%s: %s" % (type(e).__name__, str(e)[:300])
                res["vs_reference"] = {"bar": refcheck.BAR, "rel_err": {k: v["max"] for k, v in vs.items()},
                                       "per_output": {k: v["rel_err"] for k, v in vs.items()},
                                       "full_shape": bool(vs) and all(v["full_shape"] for v in vs.values()),
                                       "full_shape_per_config": {k: v["full_shape"] for k, v in vs.items()},
                                       "input_shapes": {k: v["input_shapes"] for k, v in vs.items()},
                                       "sampled_rel_err": sampled,
                                       "bars": {k: v["bars"] for k, v in vs.items()},
                                       "ok": bool(vs) and all(v["ok"] for v in vs.values()),
                                       "what": "||hip - ref||_2 / ||ref||_2 per output, same seeded inputs "
                                               "(oracle/time_reference.make_inputs); ref = the reference's "
                                               "Mode('cvm','fast_run') on this host; every config at "
                                               "BASELINE's full shape (cfg 4: T = 512, cfg 5: N = 2^24 — "
                                               "one reference evaluation each)"}
                if full_note:
                    res["vs_reference"]["full_shape_error"] = full_note
            except Exception as e:                      # noqa: BLE001  (a check row must not cost the line)
                res["vs_reference"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
            # next to every secondary row: the reference's time for the same config on this host
            key = {"cfg3b": "cfg3b", "cfg3a": "cfg3a", "cfg1b": "cfg1b", "cfg5": "cfg5"}
            for srow in secondary or ():
                name = srow.get("config", "")
                k = next((v for p_, v in key.items() if name.startswith(p_)), None)
                if srow.get("key") in others:
                    k = srow["key"]
                if name.startswith("cfg4 Scan GRU") and "B=1" in name:
                    k = "cfg4_b1"
                elif name.startswith("cfg4 Scan GRU") and "B=64" in name:
                    k = "cfg4_b64"
                if k and k in others and "ms_per_eval_full_config" in others[k]:
                    srow["cpu_reference_ms_per_eval"] = others[k]["ms_per_eval_full_config"]
                if k and k in res["vs_reference"].get("rel_err", {}):
                    if not isinstance(srow.get("check"), dict):
                        srow["check"] = {}
                    srow["check"]["vs_reference_rel_err"] = res["vs_reference"]["rel_err"][k]
            try:
                ro = reference_rows(4.0, ["cfg2"], openmp=True, timeout=240)["rows"]["cfg2"]
                res["openmp"] = {"value": 1e3 / ro["ms_per_eval"], "unit": "evals/s", "cores": ro["cores"],
                                 "kind": "reference", "ms_per_eval": ro["ms_per_eval"],
                                 "sample": "%d evals, AESARA_FLAGS=openmp=True OMP_NUM_THREADS=%d"
                                           % (ro["evals"], ro["cores"])}
            except Exception as e:                      # noqa: BLE001
                res["openmp"] = {"error": str(e)[:200]}
        except Exception as e:                          # noqa: BLE001
            res = None
            ref_err = "%s: %s" % (type(e).__name__, str(e)[:300])
    port = cpu_baseline_port(np)
    if res is None:
        res = port
        if have:
            res["reference_error"] = ref_err
    else:
        res["port"] = {k: port[k] for k in ("value", "ms_per_eval", "cores", "sample")}
    return res


def cpu_baseline_port(np):
    """Oracle C port of the reference C linker's loops for the same graph, same shape, on the
    host: bounded sample, single thread like the reference default (openmp=False,
    configdefaults.py:1037).  Fallback when the reference front end is not available."""
    import cport
    xh = np.random.default_rng(1).standard_normal((ROWS, COLS))
    cport.cfg2_eval(xh, 0.1, 1.3)  # warm-up (page faults)
    n, t0 = 0, time.perf_counter()
    while n < 10 and time.perf_counter() - t0 < 4.0:
        cport.cfg2_eval(xh, 0.1, 1.3)
        n += 1
    dt = (time.perf_counter() - t0) / n
    return {"value": 1.0 / dt, "unit": "evals/s", "cores": 1, "kind": "port",
            "sample": "%d evals of the same 4096x4096 fp64 graph (oracle/c_port.c: unfused "
                      "Composite loop + Sum loop as the reference C linker runs them)" % n,
            "ms_per_eval": dt * 1e3, "host_cores_visible": os.cpu_count()}


if __name__ == "__main__":
    main()
