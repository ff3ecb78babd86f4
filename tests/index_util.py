"""Input generators and NumPy references for tests/test_gpu_index_sort_scan.py (gather, scatter,
N-d indexing, argmax, sort, searchsorted, nonzero, cumulative).  NumPy only: the generators are
checked on the host by tests/test_index_util_host.py.

Every comparison built on these is bit-exact, so the float inputs of the scans are made of values
whose every partial sum / product is exactly representable under any association."""
import numpy as np

DTYPES = ("uint8", "int8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "float32", "float64")
INT_DTYPES = DTYPES[:8]
INDEX_DTYPES = ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64")
FLOATS = ("float32", "float64")
SMALL_INTS = ("uint8", "int8", "int16", "uint16")      # scatter-add by compare-and-swap on a word


def is_float(dtype):
    return dtype in FLOATS


def bits(a):
    """The raw bytes of ``a`` as the unsigned integer of its item size (NaN payloads, the sign of
    NaN and of zero all count in a comparison of these)."""
    a = np.ascontiguousarray(a)
    return a.view("uint%d" % (8 * a.dtype.itemsize))


def limits(dtype):
    if is_float(dtype):
        return -np.inf, np.inf
    ii = np.iinfo(dtype)
    return int(ii.min), int(ii.max)


def _nan_patterns(dtype):
    """quiet NaNs of both signs, two of them with a payload"""
    if dtype == "float32":
        return np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC00001], "uint32").view("float32")
    return np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000012345, 0xFFF8000000000001],
                    "uint64").view("float64")


def full_range(dtype, shape, seed):
    """Integers over the whole range of the type (sums and products of these wrap); floats: normal
    deviates sprinkled with NaNs carrying payloads, both zeros and both infinities."""
    rng = np.random.default_rng(seed)
    if not is_float(dtype):
        lo, hi = limits(dtype)
        a = rng.integers(lo, hi, size=shape, dtype=dtype, endpoint=True)
        flat = a.reshape(-1)
        edge = np.array([lo, hi, lo + 1, hi - 1], dtype)
        where = rng.integers(0, flat.size, size=max(1, flat.size // 4))
        flat[where] = edge[rng.integers(0, 4, size=where.size)]
        return a
    a = rng.standard_normal(shape).astype(dtype)
    flat = a.reshape(-1)
    special = np.concatenate([_nan_patterns(dtype), np.array([-0.0, 0.0, np.inf, -np.inf], dtype)])
    where = rng.integers(0, flat.size, size=max(1, flat.size // 3))
    flat[where] = special[rng.integers(0, special.size, size=where.size)]
    return a


# ---- cumulative -------------------------------------------------------------------------------
def sum_input(dtype, shape, seed):
    """cumsum input.  Floats: integers in [-3, 3] (any partial sum of up to 2**16 of them is an
    integer below 2**24: exact in float32 under every association).  Integers: the whole range."""
    if is_float(dtype):
        n = int(np.prod(shape))
        assert n <= 1 << 16
        return np.random.default_rng(seed).integers(-3, 4, size=shape).astype(dtype)
    return full_range(dtype, shape, seed)


def prod_exponents(shape, axis, seed):
    """The binary exponents of the prefix products along ``axis``: a random walk with steps
    -1 / 0 / +1 reflected at +-20 (a triangular wave of the free walk)."""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.integers(-1, 2, size=shape), axis=axis)
    return 20 - np.abs(np.mod(walk + 20, 80) - 40)


def prod_input(dtype, shape, axis, seed):
    """cumprod input.  Floats: factors from {1, -1, 2, 0.5} whose prefix products along ``axis``
    keep an exponent within [-20, 20], so the product of ANY run of consecutive factors is a signed
    power of two within 2**+-40: exact under every association.  Integers: odd factors (a product
    of odd numbers never collapses to zero) large enough to wrap."""
    rng = np.random.default_rng(seed + 1)
    if is_float(dtype):
        e = prod_exponents(shape, axis, seed)
        step = np.diff(e, axis=axis, prepend=0)
        assert np.abs(step).max() <= 1
        f = np.where(step == 0, rng.choice([1.0, -1.0], size=shape), np.exp2(step.astype("float64")))
        return f.astype(dtype)
    lo, hi = limits(dtype)
    pool = np.array([1, 1, 1, 3, 5, 7, hi if lo == 0 else -1, 11], dtype)
    return pool[rng.integers(0, pool.size, size=shape)]


def ref_cum(x, axis, mode):
    fn = np.cumprod if mode == "mul" else np.cumsum
    return fn(x, axis=axis, dtype=x.dtype)


# ---- sort -------------------------------------------------------------------------------------
def sort_keys(dtype, shape, seed):
    """Few distinct values (many ties) including the extremes of the type; floats with both
    infinities, both zeros and NaNs of both signs."""
    rng = np.random.default_rng(seed)
    if is_float(dtype):
        pool = np.concatenate([np.array([-np.inf, -1.5, -0.0, 0.0, 1.5, np.inf], dtype),
                               _nan_patterns(dtype)[:3]])
    else:
        lo, hi = limits(dtype)
        pool = np.array([lo, lo + 1, hi // 2, hi // 2 + 1, hi - 1, hi, 0 if lo else 1, 7], dtype)
    return pool[rng.integers(0, pool.size, size=shape)]


def stable_argsort(x, axis=-1):
    """ascending, NaN after every number, ties (and NaNs, and the two zeros) in input order"""
    return np.argsort(x, axis=axis, kind="stable").astype("int64")


# ---- scatter ----------------------------------------------------------------------------------
def scatter_case(dtype, row, seed, nrows=3, nidx=4096):
    """(dst [nrows, row], idx [nidx] int64 with negative spellings, y [nidx, row]) with addends
    near the extremes of the type, so that the sums wrap."""
    rng = np.random.default_rng(seed)
    lo, hi = limits(dtype)
    pool = np.array([hi, hi - 1, lo, lo + 1, 1, hi // 2, hi // 2 + 1, 3], dtype)
    dst = pool[rng.integers(0, pool.size, size=(nrows, row))]
    y = pool[rng.integers(0, pool.size, size=(nidx, row))]
    idx = rng.integers(-nrows, nrows, size=nidx).astype("int64")
    return dst, idx, y


def ref_scatter_add(dst, idx, y):
    out = dst.copy()
    np.add.at(out, idx, y)
    return out


def ref_scatter_set(dst, idx, y):
    out = dst.copy()
    for i, r in enumerate(idx.tolist()):       # sequential: the last duplicate wins
        out[r] = y[i]
    return out


def wide_scatter_add(dst, idx, y):
    """the same sums without wrap-around (Python integers)"""
    out = dst.astype(object)
    for i, r in enumerate(idx.tolist()):
        out[r] = out[r] + y[i].astype(object)
    return out


def word_lanes(dtype, nrows, row, idx, offset=0):
    """32-bit word number -> set of byte lanes written, for a contiguous [nrows, row] destination
    that starts ``offset`` elements into a 4-byte aligned allocation"""
    size = np.dtype(dtype).itemsize
    lanes = {}
    for r in sorted(set(int(i) % nrows for i in idx)):
        for e in range(row):
            byte = (offset + r * row + e) * size
            lanes.setdefault(byte // 4, set()).add(byte % 4)
    return lanes


# ---- gather -----------------------------------------------------------------------------------
def gather_rows_elems(dtype):
    """row lengths in elements for rows of one element, 15 bytes (the whole elements that fit),
    16 / 32 / 48 bytes, 16 * 64, 16 * 65 and 16 * (4 * 64 + 1) bytes"""
    size = np.dtype(dtype).itemsize
    return sorted({1, max(1, 15 // size)} | {b // size for b in (16, 32, 48, 16 * 64, 16 * 65, 16 * 257)})


def index_vector(dtype, n, nrows, seed):
    """n valid row numbers of ``dtype``; signed types use the negative spelling for about half"""
    rng = np.random.default_rng(seed)
    lo = -nrows if np.dtype(dtype).kind == "i" else 0
    v = rng.integers(lo, nrows, size=n)
    if n >= 4:
        v[0], v[1], v[-1] = nrows - 1, lo, 0
    return v.astype(dtype)


# ---- argmax -----------------------------------------------------------------------------------
ARGMAX_CASES = ("equal", "last", "ties", "extremes", "all_min", "signed_zero", "nan_first", "nan_last",
                "nan_twice")


def argmax_lines(dtype, nlines, k, seed):
    """[nlines, k]: line i holds data case ARGMAX_CASES[i % ...] (the float-only cases fall back to
    'ties' for integers).  Reduce over axis 1, or over axis 0 of the transpose."""
    rng = np.random.default_rng(seed)
    lo, hi = limits(dtype)
    fl = is_float(dtype)
    if fl:
        ext = np.array([-np.inf, np.finfo(dtype).max, -np.finfo(dtype).max, 0.0, np.finfo(dtype).tiny], dtype)
    elif lo == 0:
        ext = np.array([0, 1, hi >> 1, (hi >> 1) + 1, hi - 1], dtype)    # uint64: both sides of 2**63
    else:
        ext = np.array([lo, lo + 1, -1, 0, hi - 1], dtype)
    out = np.empty((nlines, k), dtype)
    for i in range(nlines):
        case = ARGMAX_CASES[i % len(ARGMAX_CASES)]
        if not fl and case in ("signed_zero", "nan_first", "nan_last", "nan_twice"):
            case = "ties"
        row = rng.integers(0, 3, size=k).astype(dtype)                   # 'ties'
        if case == "equal":
            row[:] = 5
        elif case == "last":
            row[-1] = 9
        elif case == "extremes":
            row = ext[rng.integers(0, ext.size, size=k)]
        elif case == "all_min":
            row[:] = lo
        elif case == "signed_zero":
            row = -1 - row
            p = int(rng.integers(0, k))
            row[p] = -0.0
            row[p + 1:p + 2] = 0.0
        elif case == "nan_first":
            row[0] = np.nan
        elif case == "nan_last":
            row[-1] = np.nan
        elif case == "nan_twice":
            p = int(rng.integers(0, k))
            row[p] = -np.nan
            row[(p + k // 2) % k] = np.nan
        out[i] = row
    return out


# ---- searchsorted -----------------------------------------------------------------------------
def searchsorted_case(dtype, nx, seed):
    """(x sorted [nx] with runs of duplicates — floats end in NaNs from nx = 3 on —, keys): the
    keys lie below all of x, above all, on every run and between the runs; floats add NaN keys."""
    rng = np.random.default_rng(seed)
    lo, hi = limits(dtype)
    if is_float(dtype):
        pool = np.array([-3.5, -1.0, 0.0, 2.0, 1e30], dtype)
        between = pool + np.array(0.25, dtype)
    else:
        span = hi - lo
        pool = np.array([lo + 2 + (span - 8) * j // 4 for j in range(5)], dtype)   # spans the range
        between = pool + np.array(1, dtype)
    nnan = 1 + nx // 8 if is_float(dtype) and nx >= 3 else 0
    x = np.concatenate([np.sort(pool[rng.integers(0, pool.size, size=nx - nnan)]),
                        np.resize(_nan_patterns(dtype)[:1], nnan) if nnan else np.empty(0, dtype)])
    keys = [np.array([lo, hi], dtype), pool, between]
    if is_float(dtype):
        keys.append(_nan_patterns(dtype)[:2])
    keys = np.concatenate(keys)
    order = np.arange(keys.size)
    order[2:] = 2 + rng.permutation(keys.size - 2)        # the two outer keys stay in front
    return x, keys[order]


def keys_of_shape(keys, shape):
    return np.resize(keys, shape) if int(np.prod(shape)) else np.empty(shape, keys.dtype)


# ---- nonzero ----------------------------------------------------------------------------------
def nonzero_input(dtype, shape, seed, fill="mixed"):
    """mixed: about half the entries clear (floats: +0.0 and -0.0), the others set (floats: NaN
    among them); clear: nothing set (floats: -0.0 everywhere); set: everything"""
    rng = np.random.default_rng(seed)
    if is_float(dtype):
        setv = np.concatenate([np.array([1.0, -2.0, np.finfo(dtype).tiny, np.inf], dtype), _nan_patterns(dtype)[:2]])
        clear = np.array([0.0, -0.0], dtype)
    else:
        lo, hi = limits(dtype)
        setv = np.array([1, hi, lo if lo else 2, hi // 2 + 1], dtype)
        clear = np.array([0], dtype)
    s = setv[rng.integers(0, setv.size, size=shape)]
    c = clear[rng.integers(0, clear.size, size=shape)]
    if fill == "set":
        return s
    if fill == "clear":
        return np.full(shape, -0.0, dtype) if is_float(dtype) else c
    return np.where(rng.random(shape) < 0.5, s, c)
