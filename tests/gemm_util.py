"""Shared by tests/test_gpu_gemm_routes.py (device) and tests/test_gemm_route_table.py (no device):
the case table that runs every instantiation of aesara_amd/csrc/gemm.hip at its smallest shape, the
operand buffers, the two value regimes and the element-wise bar.

Routes.  ``ahip_gemm_last_route()`` names the instantiation the last call launched:
``big/a{0,1,2}/b{0,1,2}/e{0,1,2}`` (128x128 tile: staging mode of A and of B, edge mode),
``half/a./b./e{0,2}/ks{1,2,4}`` (64x64 tile), ``skinny/nf{1,2,4}/bkc{0,1}/nw{4,8,16}``, ``tn``,
``small``, ``scale``, ``splitk/s{S}/big/...`` and ``none``.  Every case names the route it is meant
to run and the test asserts it; the dispatcher's tuning parameters are forced per case so that no
route depends on the CU count.

Layouts.  "N" is a row-major operand, "T" a transposed view of the row-major transpose.  A "N" is
staging mode a0 (k contiguous), A "T" is a1; B "N" is b1 (n contiguous), B "T" is b0.

Buffers.  A, B, Cin and C are views inside larger buffers: a margin of 128 rows and 128 columns (one
full tile) on every side and a row pitch with padding.  Everything outside the views is NaN, and
so is the C view itself when beta == 0.  After the call every element of the C buffer outside the
M x N view must be bit-identical to before (a store outside the view) and the view must hold no
NaN (an unwritten tile, an over-read that reached a stored output, Cin read at beta == 0).  The
margin keeps a wrong store inside the test's own allocation.

Regime A (bit-exact): A, B, Cin drawn from {-2, -1, 1, 2}, alpha from {1, -0.5, 2}, beta from
{0, 1, -0.5}.  Every partial sum is an integer or half-integer below 2**24 (K <= 33280, |product|
<= 4), exactly representable in float32: any summation order gives the same bits, and every
dropped, duplicated or misplaced product changes the sum (there are no zeros).

Regime B (derived bar): standard-normal operands, alpha from {1, 0.8, -1.5}, beta from {0, 0.4}.
A sum of K products in any order, with or without FMA, then the alpha multiply, the beta multiply
and one add (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1, at
twice gamma_n as in tests/conv_util.py):

    |got - exact| <= (K + 3) * eps(dtype) * (|alpha| * (|A| @ |B|) + |beta| * |Cin|) + tiny(dtype)

float32 is judged against the float64 NumPy result; float64 against NumPy's own float64 result at
twice the bar, because both sides carry the bound.  Nothing here is tuned.
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

MARGIN = 128
DTYPES = ("float32", "float64")
VEC = {"float32": 4, "float64": 2}
BK = {"float32": 32, "float64": 16}
MAX_MN, MAX_K = 1156, 33280

DEFAULTS = {"gemm_small_max_tiles": 64, "gemm_half_max_tiles": 448, "gemm_half_min_tiles": 192,
            "gemm_half_ksplit": -1, "gemm_skinny_nf": 0, "gemm_group": 8}
NEVER = 1 << 40


def big_params(group=8):
    return {"gemm_small_max_tiles": 0, "gemm_half_min_tiles": NEVER, "gemm_group": group}


def half_params(ks, group=8):
    return {"gemm_half_max_tiles": NEVER, "gemm_half_min_tiles": 1, "gemm_half_ksplit": ks,
            "gemm_group": group}


def row16_params(nf=0):
    return {"gemm_half_min_tiles": NEVER, "gemm_skinny_nf": nf}


@dataclass(frozen=True)
class Case:
    id: str
    family: str
    dtype: str
    route: str
    M: int
    N: int
    K: int
    ta: bool = False            # A is a transposed view
    tb: bool = False            # B is a transposed view
    batch: int = 1
    batched_api: bool = False   # ahip_gemm_batched even for batch == 1
    params: dict = field(default_factory=dict, hash=False, compare=False)
    a_how: str = ""             # "", "pitch1" (odd row pitch), "offset1" (base off by one element),
    b_how: str = ""             # "rev" (reversed rows: negative stride)
    a_bs0: bool = False         # A broadcast over the batch (a_bs = 0)
    a_bs_odd: bool = False      # batch stride of A not a multiple of VEC
    cin: str = "own"            # "own", "t" (transposed, ci_rs = 1) or "alias" (Cin is C)
    c_t: bool = False           # C column-major (c_rs = 1)
    alpha: object = None        # forced alpha / beta (None: drawn per regime)
    beta: object = None
    need_beta: bool = False     # draw beta from the non-zero values only
    splitk: str = ""            # "", "ws" (ahip_gemm_splitk with its workspace), "short" (one byte less)


def _lay(ta, tb):
    return ("T" if ta else "N") + ("T" if tb else "N")


def _big(ta, tb, e):
    return "big/a%d/b%d/e%d" % (int(ta), 0 if tb else 1, e)


def _half(ta, tb, e, ks):
    return "half/a%d/b%d/e%d/ks%d" % (int(ta), 0 if tb else 1, e, ks)


LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]


def _cases_for(dt):
    v, bk = VEC[dt], BK[dt]
    d = "f32" if dt == "float32" else "f64"
    out = []

    def add(family, name, route, M, N, K, **kw):
        out.append(Case("%s-%s-%s" % (family, d, name), family, dt, route, M, N, K, **kw))

    # ---- big tile ---------------------------------------------------------------------------
    P = big_params()
    for ta, tb in LAYOUTS:
        L = _lay(ta, tb)
        for nsl in (1, 2, 3, 5):        # one, two, odd, several slabs: the prefetch's special cases
            add("big_e0", "128x256x%dbk-%s" % (nsl, L), _big(ta, tb, 0), 128, 256, nsl * bk, ta=ta,
                tb=tb, params=P)
        add("big_e2", "132x136x2bk-%s" % L, _big(ta, tb, 2), 132, 136, 2 * bk, ta=ta, tb=tb, params=P,
            c_t=(ta and tb), cin="t" if ta else "own")
        add("big_e1", "132x136xbk+vec-%s" % L, _big(ta, tb, 1), 132, 136, bk + v, ta=ta, tb=tb,
            params=P)
        add("big_e1", "128x128x3bk+vec-%s" % L, _big(ta, tb, 1), 128, 128, 3 * bk + v, ta=ta, tb=tb,
            params=P, cin="alias")
    # scalar staging (always e1): the scalar-staged operand made by an odd pitch, a base offset
    # of one element, an odd K (k-contiguous operands only) and reversed rows
    for how in ("pitch1", "offset1"):
        add("big_scalar", "a0b2-%s" % how, "big/a0/b2/e1", 132, 136, 2 * bk, tb=True, b_how=how, params=P)
        add("big_scalar", "a1b2-%s" % how, "big/a1/b2/e1", 132, 136, 2 * bk, ta=True, b_how=how, params=P)
        add("big_scalar", "a2b1-%s" % how, "big/a2/b1/e1", 132, 136, 2 * bk, a_how=how, params=P)
        add("big_scalar", "a2b0-%s" % how, "big/a2/b0/e1", 132, 136, 2 * bk, ta=True, tb=True, a_how=how,
            params=P)
        add("big_scalar", "a2b2-%s" % how, "big/a2/b2/e1", 132, 136, 2 * bk, tb=(how == "pitch1"),
            a_how=how, b_how=how, params=P)
    add("big_scalar", "a2b1-kodd", "big/a2/b1/e1", 132, 136, 2 * bk + 1, params=P)
    add("big_scalar", "a1b2-kodd", "big/a1/b2/e1", 132, 136, 2 * bk + 1, ta=True, tb=True, params=P)
    add("big_scalar", "a2b2-kodd", "big/a2/b2/e1", 132, 136, 2 * bk + 1, tb=True, params=P)
    add("big_scalar", "a2b1-rev", "big/a2/b1/e1", 132, 136, 2 * bk, a_how="rev", params=P)
    add("big_scalar", "a0b2-rev", "big/a0/b2/e1", 132, 136, 2 * bk, tb=True, b_how="rev", params=P)
    if dt == "float32":
        # chunked fold: every 64 slabs the accumulators are folded into C (first fold: + beta * Cin)
        for cin in ("t", "alias"):
            add("big_fold", "128x136x2080-NN-cin_%s" % cin, "big/a0/b1/e2", 128, 136, 2080,
                need_beta=True, cin=cin, params=P)
            add("big_fold", "132x128x4128-TT-cin_%s" % cin, "big/a1/b0/e2", 132, 128, 4128, ta=True,
                tb=True, need_beta=True, cin=cin, params=P)
        add("big_fold", "128x128x2080-NT-e0", "big/a0/b0/e0", 128, 128, 2080, tb=True, need_beta=True,
            params=P)
    # tile walk: 10 x 3 tiles, ragged M; tiles_m is no multiple of the group, the tile count none of 8
    for grp in (1, 2, 8):
        add("big_walk", "1156x384xbk-NN-group%d" % grp, "big/a0/b1/e2", 1156, 384, bk,
            params=big_params(grp))
    add("big_walk", "1156x384xbk-TT-group2", "big/a1/b0/e2", 1156, 384, bk, ta=True, tb=True,
        params=big_params(2))
    add("big_batch", "b3-132x136x2bk-NN", "big/a0/b1/e2", 132, 136, 2 * bk, batch=3, params=P)
    add("big_batch", "b3-128x128x2bk-TN-a_bs0", "big/a1/b1/e0", 128, 128, 2 * bk, ta=True, batch=3,
        a_bs0=True, params=P)
    add("big_batch", "b2-132x136x2bk-NN-a_bs_odd", "big/a2/b1/e1", 132, 136, 2 * bk, batch=2,
        a_bs_odd=True, params=P)

    # ---- half tile --------------------------------------------------------------------------
    for ks in (1, 2, 4):
        for ta, tb in LAYOUTS:
            L = _lay(ta, tb)
            add("half_e0", "64x128x16bk-%s-ks%d" % (L, ks), _half(ta, tb, 0, ks), 64, 128, 16 * bk,
                ta=ta, tb=tb, params=half_params(ks))
            add("half_e2", "68x132x16bk-%s-ks%d" % (L, ks), _half(ta, tb, 2, ks), 68, 132, 16 * bk,
                ta=ta, tb=tb, params=half_params(ks), cin="alias" if tb else "t")
    for ta, tb in LAYOUTS:
        L = _lay(ta, tb)
        add("half_ks1", "64x128xbk-%s" % L, _half(ta, tb, 0, 1), 64, 128, bk, ta=ta, tb=tb,
            params=half_params(1))
        add("half_ks1", "68x132x3bk-%s" % L, _half(ta, tb, 2, 1), 68, 132, 3 * bk, ta=ta, tb=tb,
            params=half_params(1))
    for grp in (1, 8):
        add("half_walk", "580x192x4bk-NN-group%d" % grp, "half/a0/b1/e2/ks1", 580, 192, 4 * bk,
            params=half_params(1, grp))
    add("half_batch", "b3-68x132x16bk-TN-ks2", "half/a1/b1/e2/ks2", 68, 132, 16 * bk, ta=True, batch=3,
        params=half_params(2))

    # ---- 16-row kernels ---------------------------------------------------------------------
    for nf in ((1, 2, 4) if dt == "float32" else (1, 2)):
        R = row16_params(nf)
        for tb in (False, True):
            bkc = int(tb)
            L = _lay(False, tb)
            # K = 1024 + VEC: the last wavefronts of the 16-wave form own an empty K range
            for K, nw in ((v, 4), (200, 4), (520, 8), (1024 + v, 8 if nf == 4 else 16)):
                add("skinny", "20x72x%d-%s-nf%d" % (K, L, nf), "skinny/nf%d/bkc%d/nw%d" % (nf, bkc, nw),
                    20, 72, K, tb=tb, params=R)
            # the all-loads-first short path (K = 256: every wavefront's slice is exactly its
            # limit of 64), and the smallest problem
            for K in (64, 256):
                add("skinny", "16x64x%d-%s-nf%d" % (K, L, nf), "skinny/nf%d/bkc%d/nw4" % (nf, bkc), 16,
                    64, K, tb=tb, params=R)
            add("skinny", "1x4xvec-%s-nf%d" % (L, nf), "skinny/nf%d/bkc%d/nw4" % (nf, bkc), 1, 4, v,
                tb=tb, params=R)
    add("skinny", "b3-20x72x200-NN-nf2", "skinny/nf2/bkc0/nw4", 20, 72, 200, batch=3,
        params=row16_params(2))
    add("skinny", "20x72x520-NT-nf1-a_rev", "skinny/nf1/bkc1/nw8", 20, 72, 520, tb=True, a_how="rev",
        params=row16_params(1))
    R = row16_params()
    add("tn", "20x72x203", "tn", 20, 72, 203, ta=True, params=R)
    add("tn", "64x64x1000", "tn", 64, 64, 1000, ta=True, params=R, cin="t")
    add("small", "19x71x203", "small", 19, 71, 203, params=R)
    add("small", "20x72x200-a_offset1", "small", 20, 72, 200, a_how="offset1", params=R)
    add("small", "1x1x1", "small", 1, 1, 1, params=R)
    for beta in (0.0, -0.5):
        add("scale", "20x72-k0-beta%g" % beta, "scale", 20, 72, 0, beta=beta, params=R)
        add("scale", "20x72x200-alpha0-beta%g" % beta, "scale", 20, 72, 200, alpha=0.0, beta=beta,
            params=R)
    add("none", "m0", "none", 0, 72, 8, params=R, batched_api=True)
    add("none", "n0", "none", 20, 0, 8, params=R)
    add("none", "batch0", "none", 20, 72, 8, batch=0, params=R)

    # ---- split-K ----------------------------------------------------------------------------
    add("splitk", "128x128x8192-NN", "splitk/s8/big/a0/b1/e0", 128, 128, 8192, splitk="ws")
    add("splitk", "132x136x8192-TN", "splitk/s8/big/a1/b1/e2", 132, 136, 8192, ta=True, splitk="ws",
        cin="t")
    add("splitk", "128x128x16384-NT", "splitk/s16/big/a0/b0/e0", 128, 128, 16384, tb=True, splitk="ws")
    if dt == "float32":
        # K / S = 2080: the chunked fold runs inside a slice
        add("splitk", "128x128x33280-NN", "splitk/s16/big/a0/b1/e0", 128, 128, 33280, splitk="ws")
    # a workspace one byte too small: exactly ahip_gemm, result and route
    add("splitk", "128x128x8192-NN-short_ws", "big/a0/b1/e0", 128, 128, 8192, splitk="short", params=P)
    return out


CASES = [c for dt in DTYPES for c in _cases_for(dt)]
FAMILIES = sorted({c.family for c in CASES})


def cases_of(*families):
    return [c for c in CASES if c.family in families]


# ---- operand buffers -------------------------------------------------------------------------
class Operand:
    """A [batch, R, C] view inside a NaN-filled flat host buffer: ``flat`` (the whole buffer),
    ``view`` (the logical operand, a strided NumPy view of ``flat``), ``off`` (element offset of
    view[0, 0, 0]) and the element strides ``bs``, ``rs``, ``cs``."""

    def __init__(self, dtype, batch, R, Cc, trans=False, how="", bs0=False, bs_odd=False):
        isz = np.dtype(dtype).itemsize
        sr, sc = (Cc, R) if trans else (R, Cc)          # extents of the stored row-major matrix
        pitch = (sc + 2 * MARGIN + 3) // 4 * 4 + 8 + (1 if how == "pitch1" else 0)
        rows = sr + 2 * MARGIN
        bstride = rows * pitch + (1 if bs_odd else 0)
        nb = 1 if bs0 else max(batch, 1)
        self.flat = np.full(nb * bstride + 8, np.nan, dtype=dtype)
        off = MARGIN * pitch + MARGIN + (1 if how == "offset1" else 0)
        rstride = pitch
        if how == "rev":
            off += (sr - 1) * pitch if sr else 0
            rstride = -pitch
        stored = np.lib.stride_tricks.as_strided(
            self.flat[off:], shape=(nb, sr, sc), strides=(bstride * isz, rstride * isz, isz))
        self.view = stored.transpose(0, 2, 1) if trans else stored
        self.off = off
        self.bs = 0 if bs0 else bstride
        self.rs, self.cs = (1, rstride) if trans else (rstride, 1)
        self._geom = (off, nb, sr, sc, bstride, rstride, trans)

    def view_of(self, flat):
        """The same view on another flat array of the same length."""
        off, nb, sr, sc, bstride, rstride, trans = self._geom
        isz = flat.dtype.itemsize
        stored = np.lib.stride_tricks.as_strided(
            flat[off:], shape=(nb, sr, sc), strides=(bstride * isz, rstride * isz, isz))
        return stored.transpose(0, 2, 1) if trans else stored


def eps(dtype):
    return float(np.finfo(dtype).eps)


def gemm_bar(dtype, K, alpha, beta, absAB, absCin, against_reference=False):
    """Element-wise bound of the module docstring (an array like ``absAB``)."""
    L = abs(alpha) * np.asarray(absAB, dtype=np.float64) + abs(beta) * np.asarray(absCin, dtype=np.float64)
    return (2 if against_reference else 1) * (K + 3) * eps(dtype) * L + float(np.finfo(dtype).tiny)


def draw_values(case, regime):
    """alpha, beta (rounded to the case's dtype, as the kernel sees them) and the logical A
    [batch, M, K], B [batch, K, N], Cin [batch, M, N] of a case in a regime, from a seed that is a
    function of the case id alone."""
    rng = np.random.default_rng(zlib.crc32(("%s/%s" % (case.id, regime)).encode()))
    dt = case.dtype
    nb = max(case.batch, 1)
    if regime == "A":
        alphas, betas = (1.0, -0.5, 2.0), (0.0, 1.0, -0.5)
        draw = lambda shape: rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size=shape).astype(dt)  # noqa: E731
    else:
        alphas, betas = (1.0, 0.8, -1.5), (0.0, 0.4)
        draw = lambda shape: rng.standard_normal(shape).astype(dt)  # noqa: E731
    if case.need_beta:
        betas = tuple(b for b in betas if b != 0.0)
    alpha = float(rng.choice(alphas)) if case.alpha is None else case.alpha
    beta = float(rng.choice(betas)) if case.beta is None else case.beta
    alpha, beta = float(np.dtype(dt).type(alpha)), float(np.dtype(dt).type(beta))
    A = draw((1 if case.a_bs0 else nb, case.M, case.K))
    B = draw((nb, case.K, case.N))
    Cin = draw((nb, case.M, case.N))
    return alpha, beta, A, B, Cin


def expected(case, regime, alpha, beta, A, B, Cin):
    """(exact result in float64, |A| @ |B|): regime A through the int64 product."""
    if regime == "A":
        prod = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float64)
    else:
        prod = A.astype(np.float64) @ B.astype(np.float64)
    exact = alpha * prod + (beta * Cin.astype(np.float64) if beta != 0.0 else 0.0)
    absAB = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    return exact, absAB


def _bits(a):
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def set_params(params):
    """Force the dispatcher's parameters: the defaults overridden by ``params``."""
    from aesara_amd._lib import check, lib
    for k, val in dict(DEFAULTS, **params).items():
        check(lib.ahip_set_param(k.encode(), int(val)))


def last_route():
    from aesara_amd._lib import lib
    return lib.ahip_gemm_last_route().decode()


def run_case(case, regime):
    """Run one case in one regime on the device and check the route, the guard elements, the NaN
    canary and the values.  Returns the worst |got - exact| / bar (0 in regime A)."""
    import torch
    from aesara_amd._lib import DTYPE_CODES, check, lib

    dt = case.dtype
    isz = np.dtype(dt).itemsize
    M, N, K, batch = case.M, case.N, case.K, case.batch
    nb = max(batch, 1)
    alpha, beta, A, B, Cin = draw_values(case, regime)

    oa = Operand(dt, nb, M, K, trans=case.ta, how=case.a_how, bs0=case.a_bs0, bs_odd=case.a_bs_odd)
    ob = Operand(dt, nb, K, N, trans=case.tb, how=case.b_how)
    # a zero extent still gets a real C buffer: nothing in it may change
    oc = Operand(dt, nb, max(M, 1), max(N, 1), trans=case.c_t)
    oa.view[...] = A
    ob.view[...] = B
    alias = case.cin == "alias"
    if alias:
        oi = oc
        if beta != 0.0 and M and N:
            oc.view[...] = Cin
    else:
        oi = Operand(dt, nb, max(M, 1), max(N, 1), trans=(case.cin == "t"))
        if beta != 0.0 and M and N:
            oi.view[...] = Cin              # beta == 0: Cin stays NaN and must not be read
    before = oc.flat.copy()

    dev = {id(o): torch.from_numpy(o.flat).cuda() for o in (oa, ob, oc, oi)}
    ptr = lambda o: dev[id(o)].data_ptr() + o.off * isz  # noqa: E731
    al, be = np.array([alpha], dtype=dt), np.array([beta], dtype=dt)
    stream = torch.cuda.current_stream().cuda_stream
    code = DTYPE_CODES[dt]
    flat_args = (al.ctypes.data, ptr(oa), oa.rs, oa.cs, ptr(ob), ob.rs, ob.cs, be.ctypes.data, ptr(oi),
                 oi.rs, oi.cs, ptr(oc), oc.rs, oc.cs)

    set_params(case.params)
    plain = None
    if case.splitk:
        need = lib.ahip_gemm_ws_bytes(code, 1, M, N, K)
        assert need > 0, "the shape must be one that is split"
        if case.splitk == "short":
            # what ahip_gemm itself gives, then the same buffers again through the fallback
            check(lib.ahip_gemm(code, M, N, K, *flat_args, stream))
            plain_route = last_route()
            torch.cuda.synchronize()
            plain = dev[id(oc)].cpu().numpy()
            dev[id(oc)].copy_(torch.from_numpy(before))
            need -= 1
        ws = torch.full((lib.ahip_gemm_ws_bytes(code, 1, M, N, K) // isz,), float("nan"),
                        dtype=getattr(torch, dt), device="cuda")
        check(lib.ahip_gemm_splitk(code, M, N, K, *flat_args, ws.data_ptr(), need, stream))
    elif batch == 1 and not case.batched_api and not case.a_bs0:
        check(lib.ahip_gemm(code, M, N, K, *flat_args, stream))
    else:
        check(lib.ahip_gemm_batched(code, batch, M, N, K, al.ctypes.data, ptr(oa), oa.bs, oa.rs, oa.cs,
                                    ptr(ob), ob.bs, ob.rs, ob.cs, be.ctypes.data, ptr(oi), oi.bs, oi.rs,
                                    oi.cs, ptr(oc), oc.bs, oc.rs, oc.cs, stream))
    route = last_route()
    torch.cuda.synchronize()
    after = dev[id(oc)].cpu().numpy()

    assert route == case.route, "%s ran %s, not %s" % (case.id, route, case.route)
    if plain is not None:
        assert plain_route == route
        assert np.array_equal(_bits(plain), _bits(after)), "differs from ahip_gemm"

    # 1. nothing outside the M x N view changed
    inside = np.zeros(after.shape, dtype=bool)
    if M and N and batch:
        oc.view_of(inside)[...] = True
    changed = (_bits(after) != _bits(before)) & ~inside
    assert not changed.any(), "%s: %d elements outside C[0:M, 0:N] were written, first at flat " \
        "index %d (view starts at %d)" % (case.id, int(changed.sum()), int(np.flatnonzero(changed)[0]), oc.off)
    if not (M and N and batch):
        return 0.0
    # 2. the view holds no NaN
    got = oc.view_of(after).astype(np.float64)
    assert not np.isnan(got).any(), "%s: %d NaN in C[0:M, 0:N], first at %s" % (
        case.id, int(np.isnan(got).sum()), tuple(int(i) for i in np.argwhere(np.isnan(got))[0]))
    # 3. the values
    exact, absAB = expected(case, regime, alpha, beta, A, B, Cin)
    exact = np.broadcast_to(exact, got.shape)
    if regime == "A":
        bad = np.argwhere(got != exact)
        assert np.array_equal(got, exact), "%s: %d wrong elements, first at %s: got %r, want %r" % (
            case.id, len(bad), tuple(int(i) for i in bad[0]), got[tuple(bad[0])], exact[tuple(bad[0])])
        return 0.0
    bar = gemm_bar(dt, K, alpha, beta, np.broadcast_to(absAB, got.shape), np.abs(Cin),
                   against_reference=(dt == "float64"))
    ratio = np.abs(got - exact) / bar
    worst = float(ratio.max())
    assert worst <= 1.0, "%s: |got - exact| / bar = %.3g at %s" % (
        case.id, worst, tuple(int(i) for i in np.unravel_index(int(ratio.argmax()), ratio.shape)))
    return worst
