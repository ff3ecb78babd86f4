"""Inputs, plain references and the table of kernel forms for tests/test_gpu_reduce_matrix.py (every
CAReduce combiner and accumulator type on every layout the reduce dispatcher of
aesara_amd/exec_elemwise.py can select).  NumPy only: the generators and references are checked on
the host by tests/test_reduce_util_host.py, the form table by its dry runs.

Every comparison built on these is bit-exact.  The inputs are *runs*: a 2-d array ``R[nkept, nred]``
whose row i holds what output i reduces; ``place`` lays the runs out as the operand of a form.  The
result of a run does not depend on the order or grouping in which its elements are combined:

* integer add / mul / mul_without_zeros wrap: arithmetic in the ring Z / 2**bits;
* float add: integers in [-3, 3], fewer than 2**24 / 3 of them a run: every subset sum is exact;
* float mul: signed powers of two, the |exponents| of a whole run sum to at most 60, so the product
  of ANY subset of a run is a normal float32.  (index_util.prod_input bounds the exponent of every
  *consecutive* run only: a lane of a reduce kernel takes every 64th vector, and the exponents of
  such a subset of a long prod_input walk leave float32: test_reduce_util_host.py shows one.)
* maximum / minimum / and / or / xor are idempotent or exact anyway; +0.0 and -0.0 never share a
  run (no float run holds a zero at all), NaNs only where a test places them.
"""
from collections import namedtuple

import numpy as np

import index_util as iu

OPS = ("add", "mul", "mul_without_zeros", "maximum", "minimum", "and", "or", "xor")
WIDE = {"int8": "int64", "int16": "int64", "int32": "int64",
        "uint8": "uint64", "uint16": "uint64", "uint32": "uint64"}


def variants(op):
    """The legal (input dtype, accumulator dtype, output dtype) triples of ``op`` (reference:
    CAReduce._acc_dtype / _output_dtype; oracle/interp.py careduce): accumulation in the input
    type (wraps), small integers in a 64-bit accumulator and output, bool sums counted in int64,
    float32 through a float64 accumulator; maximum / minimum of int8 / float32 also with the wide
    accumulator and the narrow output that Max / Min get by default."""
    if op in ("add", "mul", "mul_without_zeros"):
        v = [(d, d, d) for d in iu.DTYPES] + [(d, w, w) for d, w in WIDE.items()]
        v.append(("float32", "float64", "float32"))
        if op == "add":
            v.append(("bool", "int64", "int64"))
        return v
    if op in ("maximum", "minimum"):
        return [(d, d, d) for d in iu.DTYPES + ("bool",)] + \
            [("int8", "int64", "int8"), ("float32", "float64", "float32")]
    return [(d, d, d) for d in iu.INT_DTYPES + ("bool",)]


# the pairs every form of the table runs with (the issue's list; maximum float64 also gets NaNs)
SIX = (("mul", ("float32", "float64", "float32")), ("minimum", ("int8", "int8", "int8")),
       ("and", ("uint16", "uint16", "uint16")), ("maximum", ("float64", "float64", "float64")),
       ("mul_without_zeros", ("int32", "int32", "int32")), ("add", ("bool", "int64", "int64")))


def vid(v):
    return v[0] if v[0] == v[1] == v[2] else "%s-acc_%s-out_%s" % v


# ---- runs ---------------------------------------------------------------------------------------
KINDS = {"add": ("plain",), "mul": ("plain",), "mul_without_zeros": ("plain", "zeros"),
         "maximum": ("plain", "onesided", "extreme"), "minimum": ("plain", "onesided", "extreme"),
         "and": ("plain", "ones"), "or": ("plain", "zeros"), "xor": ("plain",)}


def kinds(op, dtype):
    if dtype == "bool":
        return ("plain", "ones", "zeros")
    return KINDS[op]


def _pow2_runs(dtype, nkept, nred, rng):
    """+-1 everywhere, up to 30 factors 2 and up to 30 factors 0.5 at random places of each run"""
    r = rng.choice(np.array([1.0, -1.0], dtype), size=(nkept, nred))
    for i in range(nkept):
        k = min(30, nred // 3)
        where = rng.permutation(nred)[:2 * k]
        r[i, where[:k]] *= 2
        r[i, where[k:]] *= 0.5
    return r


def runs(op, dtype, nkept, nred, seed, kind="plain"):
    """``R[nkept, nred]`` for one (op, input dtype).  kind: 'plain'; 'onesided' — every element on
    the far side of zero from the identity's side (maximum: below zero, minimum: above), so that
    a zero where the identity belongs wins; 'extreme' — even runs equal to the identity
    throughout (dtype minimum / -inf for maximum), odd runs one-sided; 'ones' / 'zeros' — even
    runs all ones (all bits set, True) / all zero, odd runs plain."""
    rng = np.random.default_rng(seed)
    shape = (nkept, nred)
    fl = iu.is_float(dtype)
    if kind in ("ones", "zeros"):
        r = runs(op, dtype, nkept, nred, seed, "plain")
        if dtype == "bool":
            fill = kind == "ones"
        elif kind == "ones":
            fill = -1 if np.dtype(dtype).kind == "i" else iu.limits(dtype)[1]
        else:
            fill = 0
        r[0::2] = fill
        return r
    if dtype == "bool":
        assert kind == "plain"
        p = {"and": 0.98, "minimum": 0.98, "or": 0.02, "maximum": 0.02}.get(op, 0.5)
        if nred > 4096:                            # long runs: a handful of the rare value
            p = {0.98: 1 - 2.0 / nred, 0.02: 2.0 / nred}.get(p, p)
        return rng.random(shape) < p
    if op == "add":
        if fl:
            assert 3 * nred < 1 << 24
            return rng.integers(-3, 4, size=shape).astype(dtype)
        return iu.full_range(dtype, shape, seed)
    if op in ("mul", "mul_without_zeros"):
        r = _pow2_runs(dtype, nkept, nred, rng) if fl else \
            iu.full_range(dtype, shape, seed) | np.array(1, dtype)         # odd: never collapses to 0
        if op == "mul_without_zeros":                                      # zeros (+0.0) to be skipped
            r[rng.random(shape) < 0.1] = 0
        return r
    if op in ("maximum", "minimum"):
        lo, hi = iu.limits(dtype)
        side = -1 if op == "maximum" else 1
        if fl:
            r = rng.standard_normal(shape).astype(dtype)
            r[r == 0] = 1
            if kind == "plain":
                where = rng.integers(0, r.size, size=max(2, r.size // 16))
                r.reshape(-1)[where] = np.where(rng.random(where.size) < 0.5, np.inf, -np.inf)
                return r
            r = (side * np.abs(r) * np.array(10.0 ** rng.integers(-30, 30), dtype)).astype(dtype)
            r[r == 0] = side
            r.reshape(-1)[rng.integers(0, r.size, size=max(1, r.size // 16))] = side * np.inf
        else:
            r = iu.full_range(dtype, shape, seed)
            if kind == "plain":
                return r
            if op == "maximum" and lo < 0:
                r = rng.integers(lo, -1, size=shape, dtype=dtype, endpoint=True)
            elif op == "minimum":
                r = rng.integers(1, hi, size=shape, dtype=dtype, endpoint=True)
        if kind == "extreme":
            r[0::2] = (lo if op == "maximum" else hi)
        return r
    return iu.full_range(dtype, shape, seed)                               # and / or / xor: all bits


def nan_places(nred, nslices, vec):
    """Positions of a run at which the NaN cases put their NaN: the first element, the last (the
    ragged tail), the first element of slice 1 and the middle."""
    per = -(-(nred // vec) // max(nslices, 1)) * vec
    return sorted({0, nred - 1, min(per, nred - 1), nred // 2})


# ---- references ---------------------------------------------------------------------------------
def _exact_sums(r):
    """Per run, the sum of the elements as a Python integer (no wrap-around: 32-bit halves are
    summed in 64 bits, far from overflow, and put together with Python integers)."""
    assert r.shape[1] < 1 << 30
    if r.dtype == np.bool_ or r.dtype.itemsize < 8:
        return [int(s) for s in r.astype("int64").sum(axis=1)]
    u = r.view("uint64")
    lo = (u & np.uint64(0xFFFFFFFF)).sum(axis=1, dtype="uint64")
    hi = (u >> np.uint64(32)).sum(axis=1, dtype="uint64")
    tot = [int(a) + (int(b) << 32) for a, b in zip(lo, hi)]
    if r.dtype.kind == "i":       # the signed value of an element is its unsigned value - 2**64 if negative
        neg = (r < 0).sum(axis=1)
        tot = [t - (int(k) << 64) for t, k in zip(tot, neg)]
    return tot


def _exact_prods(r, mod):
    """Per run, the product of the elements modulo ``mod``, by a tree of pairwise products that
    never wrap: Python integers (object arrays), or for a modulus up to 2**32 residues below 2**32
    multiplied in uint64 (the product of two is below 2**64) and reduced explicitly."""
    if mod <= 1 << 32 and r.dtype != object:
        a = r.astype("int64" if r.dtype.kind == "i" else "uint64").astype("uint64") % np.uint64(mod)
        one = np.uint64(1)
        while a.shape[1] > 1:
            if a.shape[1] % 2:
                a = np.concatenate([a, np.full((a.shape[0], 1), one)], axis=1)
            a = (a[:, 0::2] * a[:, 1::2]) % np.uint64(mod)
        return [int(x) for x in a[:, 0]] if a.shape[1] else [1 % mod] * a.shape[0]
    a = r.astype(object)
    while a.shape[1] > 1:
        if a.shape[1] % 2:
            a = np.concatenate([a, np.ones((a.shape[0], 1), object)], axis=1)
        a = (a[:, 0::2] * a[:, 1::2]) % mod
    return [int(x) % mod for x in a[:, 0]] if a.shape[1] else [1 % mod] * a.shape[0]


def _to_dtype(values, dtype):
    """Python integers -> ``dtype`` by reduction mod 2**bits (two's complement)"""
    if dtype == "bool":
        return np.array([bool(v) for v in values], "bool")
    bits_ = 8 * np.dtype(dtype).itemsize
    u = np.array([int(v) % (1 << bits_) for v in values], dtype="uint%d" % bits_)
    return u.view(dtype) if np.dtype(dtype).kind == "i" else u.astype(dtype)


def _bit_planes(r, fold):
    u = r.view("uint%d" % (8 * r.dtype.itemsize))
    out = [0] * r.shape[0]
    for b in range(8 * r.dtype.itemsize):
        plane = ((u >> np.array(b, u.dtype)) & np.array(1, u.dtype)).astype("uint8")
        for i, bit in enumerate(fold(plane)):
            out[i] |= int(bit) << b
    return out


def ref_runs(op, r, acc, out):
    """The reduction of every run of ``r`` (NumPy [nkept, nred], nred >= 1 unless the op has an
    identity), accumulated in ``acc`` and stored as ``out``: [nkept] of dtype ``out``."""
    dtype = r.dtype.name
    nkept, nred = r.shape
    fl = iu.is_float(dtype)
    if op in ("maximum", "minimum"):
        if nred == 0:
            raise ValueError("zero-size array to reduction operation which has no identity")
        f = np.max if op == "maximum" else np.min
        if fl:
            nan = np.isnan(r).any(axis=1)
            v = f(np.where(np.isnan(r), 0, r), axis=1)
            v = np.where(nan, np.nan, v)
        else:
            v = f(r, axis=1)
        return v.astype(acc).astype(out)
    if op in ("and", "or", "xor"):
        if dtype == "bool":
            v = {"and": r.all(axis=1), "or": r.any(axis=1), "xor": r.sum(axis=1) % 2 == 1}[op]
            return v.astype(out)
        fold = {"and": lambda p: p.min(axis=1, initial=1), "or": lambda p: p.max(axis=1, initial=0),
                "xor": lambda p: p.sum(axis=1, dtype="int64") % 2}[op]
        return _to_dtype(_bit_planes(r, fold), acc).astype(out)
    if op == "add":
        if fl:
            tot = [float(s) for s in r.astype("float64").sum(axis=1)]      # small integers: exact
            assert all(t == int(t) and abs(t) < 1 << 24 for t in tot)
            return np.array(tot, acc).astype(out)
        if acc == "bool":
            return r.any(axis=1).astype(out)
        return _to_dtype(_exact_sums(r), acc).astype(out)
    assert op in ("mul", "mul_without_zeros")
    some = (r != 0).any(axis=1)
    if fl:
        # signed powers of two: the exponents add, the signs multiply (integer arithmetic)
        m, e = np.frexp(np.where(r == 0, 1, r).astype("float64"))
        assert (np.abs(m) == 0.5).all()
        esum = (e - 1).sum(axis=1)
        sign = 1 - 2 * ((r < 0).sum(axis=1) % 2)
        v = np.ldexp(sign.astype("float64"), esum)
        assert op == "mul_without_zeros" or (r != 0).all()
        v = np.where(some, v, 0.0)
        return v.astype(acc).astype(out)
    bits_ = 8 * np.dtype(acc).itemsize
    if op == "mul_without_zeros":
        p = _exact_prods(np.where(r == 0, 1, r), 1 << bits_)
        p = [x if s else 0 for x, s in zip(p, some)]
    else:
        p = _exact_prods(r, 1 << bits_)
    return _to_dtype(p, acc).astype(out)


def empty_result(op, acc, out):
    """What a reduction over no elements gives (the Op's identity), or ValueError"""
    if op in ("maximum", "minimum"):
        raise ValueError("zero-size array to reduction operation which has no identity")
    if op == "and":
        return np.array(True, out) if acc == "bool" else _to_dtype([-1], acc).astype(out)[0]
    return np.array(1 if op == "mul" else 0, acc).astype(out)


def canon(a):
    """``iu.bits`` of ``a`` with every NaN replaced by the one default NaN: the comparison is exact
    in everything but the payload and sign of a NaN."""
    a = np.array(a, copy=True)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return iu.bits(a)


# ---- layouts ------------------------------------------------------------------------------------
def place(r, shape, axis, view=None, seed=0):
    """The operand of shape ``shape`` whose reduction over ``axis`` has the runs ``r`` (output i in
    C order of the kept dims <- r[i]), as a NumPy array with the view geometry of ``view``:
    None (contiguous), 'T' (a transposed view of a contiguous array), 'rev_step' (first dim
    reversed, last dim every second element of the base), 'step' (last dim every second element),
    'off1' (contiguous, one element into its buffer: not 16-byte aligned).  The gaps of a stepped
    base hold other values of the same kind."""
    nd = len(shape)
    axis = sorted(range(nd) if axis is None else axis)
    kept = [d for d in range(nd) if d not in axis]
    a = r.reshape([shape[d] for d in kept + axis]).transpose(np.argsort(kept + axis))
    assert a.shape == tuple(shape)
    if view is None:
        return np.ascontiguousarray(a)
    if view == "T":
        return np.ascontiguousarray(a.transpose(list(range(nd))[::-1])).transpose(list(range(nd))[::-1])
    if view == "off1":
        base = np.empty(a.size + 1, a.dtype)
        base[0] = a.reshape(-1)[-1]
        v = base[1:].reshape(a.shape)
        v[...] = a
        return v
    base = np.ascontiguousarray(np.repeat(a, 2, axis=nd - 1)[..., :2 * a.shape[-1] + 1])
    base = np.concatenate([base, base[..., :1]], axis=nd - 1)      # odd pitch: the dims do not merge
    v = base[..., :-1:2]
    v = v[::-1] if view == "rev_step" else v
    v[...] = a
    return v


# ---- the table of forms -------------------------------------------------------------------------
# shape / axis / view as for ``place``; ``V`` in a shape stands for the elements of a 16-byte vector
# of the input type.  expect: what the dispatcher must select (checked on a dry run and again on the
# device): mode 0 row / 1 column, short, vec (True: > 1 whenever the type has 16-byte vectors of more
# than one element, 1: scalar loads), lanes, sliced, nslices, empty_last (the last slice holds no
# element).
Form = namedtuple("Form", "name shape axis view expect")
V = "V"

AXIS_FORMS = (
    Form("row_tiny", (5, 3), (1,), None, dict(mode=0, lanes=2, vec=1, short=False, sliced=False)),
    Form("row_short_vec", (5, 64), (1,), None, dict(mode=0, vec=True, short=True, sliced=False)),
    Form("row_loop", (7, (72, V)), (1,), None, dict(mode=0, vec=True, lanes=64, short=False, sliced=False)),
    Form("row_loop_ragged", (7, 501), (1,), None, dict(mode=0, vec=1, lanes=64, short=False, sliced=False)),
    Form("row_sliced_vec", (3, (512, V)), (1,), None, dict(mode=0, vec=True, lanes=64, nslices=2)),
    Form("row_sliced_ragged", (7, 2049), (1,), None, dict(mode=0, vec=1, lanes=64, nslices=8)),
    Form("row_sliced_empty_last", (2, 66049), (1,), None,
         dict(mode=0, vec=1, lanes=64, nslices=258, empty_last=True)),
    Form("row_rev_step", (6, 130), (1,), "rev_step", dict(mode=0, vec=1, lanes=64, short=False, sliced=False)),
    Form("col_narrow", (64, 8), (0,), None, dict(mode=1, lanes_below=64, sliced=False)),
    Form("col_wide_ragged", (15, 257), (0,), None, dict(mode=1, vec=1, lanes=128, sliced=False)),
    Form("col_wide_vec", (15, 260), (0,), None, dict(mode=1, lanes=128, sliced=False)),
    Form("col_sliced_vec", (2048, 16), (0,), None, dict(mode=1, lanes_below=64, sliced=True)),
    Form("col_sliced", (1024, 7), (0,), None, dict(mode=1, vec=1, lanes=8, nslices=8)),
    Form("col_sliced_ragged", (1027, 7), (0,), None, dict(mode=1, vec=1, lanes=8, nslices=8)),
    Form("col_sliced_empty_last", (16641, 7), (0,), None,
         dict(mode=1, vec=1, lanes=8, nslices=130, empty_last=True)),
    Form("mixed_3d_02", (6, 10, 12), (0, 2), None, dict(sliced=False)),
    Form("mixed_3d_1_T", (6, 10, 12), (1,), "T", dict(sliced=False)),
)
# the four forms every legal (op, variant) pair runs on (with FLAT_RAGGED below)
EVERY_PAIR = ("row_tiny", "row_sliced_ragged", "col_sliced_ragged")


def axis_form(name):
    return next(f for f in AXIS_FORMS if f.name == name)


def resolve(shape, dtype):
    v = 16 // np.dtype(dtype).itemsize
    return tuple(s[0] * v if isinstance(s, tuple) else s for s in shape)


def sliced_geometry(nred, vec, nslices):
    """(elements per slice, whether the last slice is empty) as the kernels cut a run"""
    nredv = nred // vec
    per = -(-nredv // nslices)
    return per * vec, per * (nslices - 1) >= nredv


# ---- plans, operands of a dry run, what the dispatcher selected ----------------------------------
def reduce_plan(v, nd, axis, op):
    """One CAReduce node over ``axis`` (None: all) of an ``nd``-d input; v = (dtype, acc, out)"""
    from aesara_amd.plan import Node, Plan, Var
    nout = 0 if axis is None else nd - len(axis)
    return Plan("red_" + op, {0: Var(0, v[0], [None] * nd), 1: Var(1, v[2], [None] * nout)}, [0], [1],
                [Node("CAReduce", [0], [1], {"scalar_op": op, "axis": None if axis is None else list(axis),
                                             "acc_dtype": v[1]})])


def pair_op(dtype):
    """The exact elementwise op of the two-operand forms: x (+) y with wrap-around, x * y with y a
    power of two, x != y"""
    return "xor" if dtype == "bool" else ("mul" if iu.is_float(dtype) else "add")


def pair_plan(v, op, nred_plans=1):
    """``nred_plans`` independent  Elemwise(pair_op)(x_k, y_k) -> full CAReduce  chains of 2-d
    operands: 2 * nred_plans inputs, nred_plans 0-d outputs"""
    from aesara_amd.plan import Node, Plan
    p = Plan("pairred_" + op, {}, [], [], [])
    for _ in range(nred_plans):
        x, y = p.new_var(v[0], [None, None]), p.new_var(v[0], [None, None])
        e, o = p.new_var(v[0], [None, None]), p.new_var(v[2], [])
        p.inputs += [x, y]
        p.outputs.append(o)
        p.nodes.append(Node("Elemwise", [x, y], [e], {"scalar": {
            "n_in": 2, "nodes": [{"op": pair_op(v[0]), "in": [["i", 0], ["i", 1]], "dtype": v[0]}],
            "out": [["t", 0]]}}))
        p.nodes.append(Node("CAReduce", [e], [o], {"scalar_op": op, "axis": None, "acc_dtype": v[1]}))
    return p


def towers_plan(v, op, n):
    """``n`` independent full reductions of 1-d inputs (one scalar program: a horizontal group)"""
    from aesara_amd.plan import Node, Plan
    p = Plan("towers_" + op, {}, [], [], [])
    for _ in range(n):
        x, o = p.new_var(v[0], [None]), p.new_var(v[2], [])
        p.inputs.append(x)
        p.outputs.append(o)
        p.nodes.append(Node("CAReduce", [x], [o], {"scalar_op": op, "axis": None, "acc_dtype": v[1]}))
    return p


def split_pair(a, y):
    """x with  pair_op(x, broadcast y) == a  exactly (y: float powers of two, any integers, bools)"""
    dt = a.dtype.name
    if dt == "bool":
        return a != y
    if iu.is_float(dt):
        x = (a / y).astype(dt)
        assert np.array_equal(canon(x * y), canon(a))
        return x
    return (a - y).astype(dt)             # wraps, as the sum does


def pair_operand(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    if dtype == "bool":
        return rng.random(shape) < 0.5
    if iu.is_float(dtype):
        return rng.choice(np.array([1, -1, 2, 0.5, -4], dtype), size=shape)
    return iu.full_range(dtype, shape, seed)


def geometry(a):
    """(base buffer flattened, element offset, element strides) of a NumPy view"""
    base = a
    while isinstance(base.base, np.ndarray):
        base = base.base
    assert base.dtype == a.dtype and base.flags.c_contiguous
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return base.reshape(-1), off, [s // a.itemsize for s in a.strides]


def fake_dev(a):
    """The operand of a dry run with the geometry of the NumPy view ``a`` (no data)"""
    from aesara_amd.device import DevArray
    from aesara_amd.executor import _FakeBuf
    base, off, strides = geometry(a)
    return DevArray(_FakeBuf(max(base.size, 1), a.dtype.name), off, a.shape, strides, a.dtype.name)


class Spy:
    """Records (entry point, arguments) of every launch of an executor, dry or real"""

    def __init__(self, ex):
        self.ex, self.calls = ex, []
        inner = ex._launch

        def launch(name, args):
            self.calls.append((name, args))
            return inner(name, args)
        ex._launch = launch

    def clear(self):
        del self.calls[:]
        self.ex._ew_memo.clear()

    def names(self):
        return [n for n, _ in self.calls]

    def axis_passes(self):
        """per ahip_elemwise_reduce_axis launch: dict(mode, nslices, vec, lanes)"""
        return [dict(mode=a[1], nslices=a[8], vec=a[11], lanes=a[12])
                for n, a in self.calls if n == "ahip_elemwise_reduce_axis"]

    def memo(self, kind):
        return [k for k in self.ex._ew_memo if k and k[0] == kind]


def check_axis_form(form, dtype, spy, nred):
    """Assert that the launches ``spy`` recorded for ``form`` are the form's: returns
    (nslices, vec) of the first pass."""
    e, what = form.expect, (form.name, dtype)
    passes = spy.axis_passes()
    keys = spy.memo("axis")
    assert passes and len(keys) == len(passes) and not spy.memo("all"), (what, spy.names())
    first = passes[0]
    key = next(k for k in keys if k[10] == first["lanes"] and k[9] == first["mode"] and k[7] == first["vec"])
    short = key[16]
    itemsize = np.dtype(dtype).itemsize
    sliced = e.get("sliced", "nslices" in e)
    assert len(passes) == (2 if sliced else 1), (what, passes)
    assert (first["nslices"] > 1) == sliced, (what, passes)
    if "mode" in e:
        assert first["mode"] == e["mode"], (what, passes)
    if "lanes" in e:
        assert first["lanes"] == e["lanes"], (what, passes)
    if "lanes_below" in e:
        assert first["lanes"] < e["lanes_below"], (what, passes)
    if e.get("vec") is True:
        assert first["vec"] == 16 // itemsize and (first["vec"] > 1 or itemsize == 16), (what, passes)
    elif "vec" in e:
        assert first["vec"] == e["vec"], (what, passes)
    if "short" in e:
        assert bool(short) == e["short"], (what, key)
    if "nslices" in e:
        assert first["nslices"] == e["nslices"], (what, passes)
    if sliced:
        assert passes[1]["nslices"] == 1 and passes[1]["mode"] == 1, (what, passes)
    if e.get("empty_last"):
        assert sliced_geometry(nred, first["vec"], first["nslices"])[1], (what, passes)
    return first["nslices"], first["vec"]


# ---- full reductions ----------------------------------------------------------------------------
CUS = 256            # compute units of the device the lengths below are sized for (MI355X)


def flat_vec(dtype):
    """elements per lane and load of the flat full-reduction stream (exec_elemwise._pick_vec)"""
    from aesara_amd.exec_common import TUNE
    return max(1, min(8, TUNE["vecbytes"] // np.dtype(dtype).itemsize))


def red_block():
    from aesara_amd.exec_common import TUNE
    return TUNE["red_block"]


def flat_cap():
    """workgroups (= partials) a flat full reduction gets at most (csrc/elemwise_launch.hip:
    ahip_elemwise_reduce_all — CUs x 4 x 256 / block)"""
    return CUS * max(1, 4 * 256 // red_block())


def full_forms(dtype):
    """Single-operand full reductions: Form(name, shape, None, view, expect) with expect =
    dict(nd, vec, flat1) of the ("all", ...) memo key.  A single flat launch never has more than
    ``flat_cap()`` = 256 partials, so its finalize collects with one wave: the horizontal group
    and the tiled form (below) are the ones that reach two collecting waves."""
    b, v = red_block(), flat_vec(dtype)
    odd = dict(nd=1, vec=1, flat1=False)
    vecd = dict(nd=1, vec=v, flat1=v > 1)
    return (
        Form("flat_1", (1,), None, None, dict(nd=1, vec=1, flat1=False)),
        Form("flat_63", (63,), None, None, odd), Form("flat_64", (64,), None, None, vecd),
        Form("flat_65", (65,), None, None, odd),
        Form("flat_block-1", (b * v - 1,), None, None, odd), Form("flat_block", (b * v,), None, None, vecd),
        Form("flat_block+1", (b * v + 1,), None, None, odd),
        Form("flat_ragged", ((5 * b + 77) * v,), None, None, vecd),                 # 6 partials
        Form("flat_over_cap", ((flat_cap() * b + 1000) * v,), None, None, vecd),    # grid-stride walk
        Form("scalar_off1", (2 * b + 1,), None, "off1", odd),
        Form("strided_2d", (9, 130), None, "step", dict(nd=2, vec=1, flat1=False)),
    )


FLAT_RAGGED = "flat_ragged"
# two-operand forms: (name, shape of x, shape of y before the view, view of y, expectation)
PAIR_FORMS = (
    ("bcast_inner", (37, 64), (37, 1), None, dict(entry="ahip_elemwise_reduce_all", invariant=(False, False))),
    ("scalar_operand", (37, 64), (1, 1), None, dict(entry="ahip_elemwise_reduce_all", invariant=(False, True))),
    ("tiled_32", (35, 70), (35, 70), "T", dict(entry="ahip_elemwise_tiled")),
    ("tiled_64", (50, 130), (50, 130), "T", dict(entry="ahip_elemwise_tiled")),
    ("tiled_many", (40, 4100), (40, 4100), "T", dict(entry="ahip_elemwise_tiled")),   # 258 tiles of 32
)


def check_full_form(form, spy):
    e, names = form.expect, spy.names()
    assert names == ["ahip_elemwise_reduce_all"], (form.name, names)
    (k,) = spy.memo("all")
    assert (k[5], k[6], k[8]) == (e["nd"], e["vec"], e["flat1"]), (form.name, k[3:10])
    if form.view == "step":
        assert "s" in k[4], (form.name, k[4])


def check_pair_form(name, expect, spy):
    names = spy.names()
    assert names == [expect["entry"]], (name, names)
    if "invariant" in expect:
        (k,) = spy.memo("all")
        assert tuple(k[9]) == expect["invariant"], (name, k[9])


def hgroup_lengths(dtype):
    """three flat lengths of one horizontal group: a short one, a ragged one and one with more
    block-sized pieces than its share of the grid"""
    b, v = red_block(), flat_vec(dtype)
    return (64 * v, (3 * b + 5) * v, (300 * b + 9) * v)
