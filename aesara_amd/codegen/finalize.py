"""In-kernel finalize of a full reduction, the wavefront fold it is built on, and the layout of
the reduce workspace that the host side shares with it."""
from __future__ import annotations

from .prelude import CTYPE, RTYPE
from .scalar import is_float, red_combine, red_identity, store_val

TRACE_SLOTS = 8          # 8-byte stamps per workgroup of an EW_TRACE build (after the 4 KiB tail of ws)
TRACE_HALF = 2048        # workgroup slots per half of the trace area (even / odd launch epochs)
REDUCE_ERR_OFF = 128     # error word of the in-kernel finalize: bytes past the shard sums (epoch at +64)
REDUCE_HOSTFLAG_OFF = 192  # 8-byte pointer to a host-mapped (pinned) flag the failing launch also raises


def wave_fold_lines(acc_t, comb, var="acc", indent="    "):
    """Fold `var` over the 64 lanes of a wavefront in a fixed tree, without LDS round trips: four
    DPP steps leave every lane of a 16-lane row with the row's fold, the four row leaders are
    then combined in lane order (uniform reads).  Every lane ends with the wave's fold."""
    out = []
    for ctrl in ("0xB1", "0x4E", "0x141", "0x140"):
        out.append("%s%s = %s;" % (indent, var, comb(var, "dpp_mov_<%s, %s>(%s)" % (acc_t, ctrl, var))))
    rows = ["lane_get_<%s>(%s, %d)" % (acc_t, var, 16 * r) for r in range(4)]
    out.append("%s%s = %s;" % (indent, var, comb(comb(comb(rows[0], rows[1]), rows[2]), rows[3])))
    return out


COLLECT_K = 4            # partials per lane per polling round of the finalize (8 granule loads in flight;
#                          8 per lane would put the kernel above 64 VGPRs = one 1024-thread workgroup per CU)


def reduce_all_finalize(spec, red, L):
    """Deterministic in-kernel finalize of a full reduction (appended after the streaming loop:
    `acc` holds the thread's partial).

    ONE hop on a static tree, no tickets and no fences: every workgroup folds its threads (DPP
    inside a wavefront, the waves in order through LDS) and publishes its partial as two
    epoch-tagged 8-byte granules {hi32 | epoch}, {lo32 | epoch} (agent-scope write-through
    stores, single-copy atomic).  Workgroup 0 then collects: wavefront w takes the partials
    [256 w, 256 w + 256), four per lane and all eight granule loads of a lane in flight at
    once, re-reading until every tag carries this launch's epoch; lanes fold their four in index
    order, the wave folds by DPP, the collecting waves in order through LDS (the other waves of
    workgroup 0 have exited: the barrier counts live waves only).  With the default 1024-thread
    workgroups a launch has <= 512 partials: two wavefronts collect side by side and the critical
    path after the last workgroup has streamed is one store -> load visibility latency.  The
    workspace is zero-initialised once; epoch 0 never matches a live tag; every spin is bounded
    and a partial that never arrives raises the error word (a float result is NaN)."""
    acc_t = RTYPE[red["acc"]]
    sm_t = acc_t if acc_t != "bool" else "unsigned char"
    comb = lambda a_, b_: red_combine(red["op"], red["acc"], a_, b_)  # noqa: E731
    nw = spec.block // 64
    AG = "__ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT"
    K = COLLECT_K
    ident = red_identity(red["op"], red["acc"])
    tr = spec.trace

    L.append("  __shared__ %s sm[%d];" % (sm_t, nw))
    L.append("  unsigned long long* wsp = (unsigned long long*)a.ws;")
    L.append("  unsigned* errp = (unsigned*)((char*)a.ws + a.aux1 + 2048 + %d);" % REDUCE_ERR_OFF)
    L.append("  const unsigned ep = ep0 + 1u;")
    L.append("  const unsigned wv_ = threadIdx.x >> 6, ln_ = threadIdx.x & 63u;")
    # workgroup partial: wave folds, then the waves in order
    L.append("  {")
    L.extend(wave_fold_lines(acc_t, comb))
    if nw > 1:
        L.append("    if (ln_ == 0) sm[wv_] = acc;")
        L.append("    __syncthreads();")
    L.append("    if (threadIdx.x == 0) {")
    if nw > 1:
        L.append("      %s r = sm[0];" % acc_t)
        L.append("      for (int w = 1; w < %d; ++w) r = %s;" % (nw, comb("r", "(%s)sm[w]" % acc_t)))
    else:
        L.append("      %s r = acc;" % acc_t)
    L.append("      union { unsigned long long u; %s v; } cv; cv.u = 0; cv.v = r;" % acc_t)
    L.append("      unsigned long long* slot = wsp + 2 * (size_t)blockIdx.x;")
    L.append("      __hip_atomic_store(slot, ((cv.u >> 32) << 32) | ep, %s);" % AG)
    L.append("      __hip_atomic_store(slot + 1, (cv.u << 32) | ep, %s);" % AG)
    if tr:
        L.append("      tr_s_[4] = wall_clock64();")
        L.append("      unsigned long long* const tr_ = (unsigned long long*)((char*)a.ws + a.aux1 + 4096) + "
                 "%d * ((size_t)blockIdx.x + (ep & 1u) * %d);" % (TRACE_SLOTS, TRACE_HALF))
        L.append("      for (int q = 0; q < 8; ++q) if (q < 5 || q == 7) tr_[q] = tr_s_[q];")
    L.append("    }")
    L.append("  }")
    hj = spec.hjobs
    L.append("  if (%s != 0) return;" % ("lb_" if hj else "blockIdx.x"))
    # ---- workgroup 0 (of the job): collect
    L.append("  const unsigned G_ = %s;" % ("gj_" if hj else "gridDim.x"))
    if hj:
        L.append("  wsp += 2 * (size_t)slot0_;             // this job's partial slots")
    L.append("  const unsigned ncol_ = (G_ + %du) / %du < %du ? (G_ + %du) / %du : %du;   // collecting waves" %
             (64 * K - 1, 64 * K, nw, 64 * K - 1, 64 * K, nw))
    L.append("  const bool one_wave = ncol_ <= 1u;")
    L.append("  if (wv_ >= ncol_) return;")
    if nw > 1:
        L.append("  if (!one_wave) __syncthreads();        // sm[] is reused below (live waves only)")
    L.append("  acc = %s;" % ident)
    L.append("  for (unsigned c0 = wv_ * %du; c0 < G_; c0 += %du) {" % (64 * K, 64 * K * nw))
    L.append("    unsigned long long g0[%d], g1[%d];" % (K, K))
    L.append("    bool seen = false;")
    L.append("    for (int spin = 0; spin < (1 << 24); ++spin) {")
    L.append("      bool all_ = true;")
    L.append("#pragma unroll")
    L.append("      for (int k = 0; k < %d; ++k) {" % K)
    L.append("        const unsigned idx = c0 + (unsigned)k * 64u + ln_;")
    L.append("        if (idx < G_) {")
    L.append("          g0[k] = __hip_atomic_load(wsp + 2 * (size_t)idx, %s);" % AG)
    L.append("          g1[k] = __hip_atomic_load(wsp + 2 * (size_t)idx + 1, %s);" % AG)
    L.append("        }")
    L.append("      }")
    L.append("#pragma unroll")
    L.append("      for (int k = 0; k < %d; ++k) {" % K)
    L.append("        const unsigned idx = c0 + (unsigned)k * 64u + ln_;")
    L.append("        if (idx < G_) all_ = all_ && (unsigned)g0[k] == ep && (unsigned)g1[k] == ep;")
    L.append("      }")
    L.append("      if (all_) { seen = true; break; }")
    L.append("      __builtin_amdgcn_s_sleep(1);")
    L.append("    }")
    # a partial that never arrived (the producing workgroup starved for ~2^24 polls: a device
    # shared with something that never yields) must not become a silently wrong sum: the launch
    # tags the device error word with ITS epoch (so only its own float result becomes NaN: later
    # launches carry other epochs and nothing has to be cleared) and raises a flag in pinned host
    # memory, which the executor looks at after every call without touching the device
    L.append("    if (!seen) {")
    L.append("      __hip_atomic_store(errp, ep, %s);" % AG)
    L.append("      unsigned* hostp = *(unsigned* volatile*)((char*)a.ws + a.aux1 + 2048 + %d);" % REDUCE_HOSTFLAG_OFF)
    L.append("      if (hostp) __hip_atomic_store(hostp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);")
    L.append("    }")
    L.append("#pragma unroll")
    L.append("    for (int k = 0; k < %d; ++k) {" % K)
    L.append("      const unsigned idx = c0 + (unsigned)k * 64u + ln_;")
    L.append("      if (idx < G_) {")
    L.append("        union { unsigned long long u; %s v; } cv; cv.u = ((g0[k] >> 32) << 32) | (g1[k] >> 32);" % acc_t)
    L.append("        acc = %s;" % comb("acc", "cv.v"))
    L.append("      }")
    L.append("    }")
    L.append("  }")
    if tr:
        L.append("  if (threadIdx.x == 0) tr_s_[5] = wall_clock64();")
    L.append("  {")
    L.extend(wave_fold_lines(acc_t, comb))
    if nw > 1:
        L.append("    if (!one_wave) {")
        L.append("      if (ln_ == 0) sm[wv_] = acc;")
        L.append("      __syncthreads();")
        L.append("      acc = sm[0];")
        L.append("      for (unsigned w = 1; w < ncol_; ++w) acc = %s;" % comb("acc", "(%s)sm[w]" % acc_t))
        L.append("    }")
    L.append("    if (threadIdx.x == 0) {")
    L.append("      %s r = acc;" % acc_t)
    if is_float(red["acc"]):
        L.append("      if (__hip_atomic_load(errp, %s) == ep) r = (%s)__builtin_nan(\"\");" % (AG, acc_t))
    L.append("      *(%s*)a.out = %s;" % (CTYPE[red["out"]], store_val("r", red["acc"], red["out"])))
    L.append("      __hip_atomic_store(epochp, ep, %s);" % AG)
    if tr:
        L.append("      tr_s_[6] = wall_clock64();")
        L.append("      unsigned long long* const tr_ = (unsigned long long*)((char*)a.ws + a.aux1 + 4096) + "
                 "%d * ((size_t)blockIdx.x + (ep & 1u) * %d);" % (TRACE_SLOTS, TRACE_HALF))
        L.append("      tr_[5] = tr_s_[5]; tr_[6] = tr_s_[6];")
    L.append("    }")
    L.append("  }")
