"""The index (csrc/index.hip), sort (csrc/sort.hip) and scan (csrc/cumulative.hip) kernels at every
element type, index type and dispatch edge: one-node plans on device tensors (views carry the
strides and the misalignment), the C ABI where a plan cannot reach a case, NumPy as the reference.
Every comparison is bit-exact (tests/index_util.py builds float scan inputs whose partial results
are exact), and the form a shape is meant to select is asserted through the library's own queries.

Kernel / dispatch branch -> test that reaches it (and the query that proves the path):
  take_rows_vec_kernel lg 0..6, 4-in-flight loop + tail, take_rows_kernel (odd rows, x[1:],
    x[:, 1:], one element in), 8 index types        test_gather_rows_...[int8|uint16|float32|float64]
  scatter_add_kernel / scatter_set_kernel (rows 1, 3, 7), scatter_add_rows_kernel lg 3..6,
    atomic_acc_small on shared words                test_scatter_rows_contended_and_wrapping[T-set|inc]
  ... destination one element in (C ABI)            test_scatter_rows_into_a_destination_...[T-set|inc]
  N-d set / inc / buffered inc                      test_nd_inc_subtensor_int16[...]
  linearize_kernel 1, 2, 3, 8 arrays, broadcast     test_nd_gather_*; errors incl. uint64 >= 2**63:
                                                    test_nd_index_errors_leave_the_executor_usable[k]
  argmax_rows_kernel vector + element form          test_argmax_row_form[T]      (ahip_argmax_ws_bytes == 0)
  argmax_cols_kernel<V>, <1>, argmax_fold_kernel    test_argmax_column_form_sliced[T]  (... > 0)
  sort_rows_kernel n = 1, 2, 3 .. M, sort_chunks_kernel + merge_pass_kernel M+1, 2M+1, 3M
                                                    test_sort_and_argsort[T-layout]  (ahip_sort_max_row)
  searchsorted_kernel                               test_searchsorted[T]
  nonzero_write_kernel 1..8 dims, chunked count     test_nonzero[T]  (ahip_cumulative_ws_bytes > 0)
  cum_wave_kernel / cum_wave_vec_kernel, single pass and chunked
                                                    test_cumulative_flat_lengths[T-mode]  (== 0 / > 0)
  cum_lines_kernel / cum_lines_vec_kernel chunked, transposed and offset views, axis=None
                                                    test_cumulative_lines_and_views[T-mode]  (> 0)
  launch-list replay of each op                     test_replayed_executor_gives_the_same_results[op]
Rows of 15 bytes exist for 1-byte items only; wider items use the whole elements that fit in 15."""
import ctypes as C

import numpy as np
import pytest

import index_util as iu

pytestmark = pytest.mark.gpu

_EX = {}


# ---- plumbing ---------------------------------------------------------------------------------
def _code(dtype):
    from aesara_amd.device import dtype_code
    return dtype_code(dtype)


def _lib():
    from aesara_amd._lib import lib
    return lib


def _upload(flat):
    """1-d NumPy array -> device tensor of the same dtype"""
    import torch
    name = flat.dtype.name
    if name in ("uint16", "uint32", "uint64"):
        return torch.from_numpy(flat.view(name[1:])).cuda().view(getattr(torch, name))
    return torch.from_numpy(flat).cuda()


def dev(a):
    """The device image of a NumPy array WITH its view geometry: the base buffer is uploaded and
    the same offset / strides are applied to it (a torch view; negative strides, which torch
    cannot express, as a DevArray over the uploaded tensor)."""
    import torch
    from aesara_amd.device import DevArray
    a = np.asarray(a)
    base = a
    while isinstance(base.base, np.ndarray):
        base = base.base
    if base.dtype != a.dtype or not base.flags.c_contiguous or a.size == 0:
        base = a = np.ascontiguousarray(a)
    t = _upload(base.reshape(-1))
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    strides = [s // a.itemsize for s in a.strides]
    if all(s >= 0 for s in strides):
        return torch.as_strided(t, a.shape, strides, off)
    return DevArray.from_torch(t).view(a.shape, strides, off)


def host(t):
    import torch
    name = str(t.dtype).split(".")[-1]
    if name in ("uint16", "uint32", "uint64"):
        return t.view(getattr(torch, name[1:])).cpu().numpy().view(name)
    return t.cpu().numpy()


def executor(op, ins, outs, params, **kw):
    """cached one-node plan executor; ins / outs: lists of (dtype, ndim)"""
    from aesara_amd.executor import PlanExecutor
    from aesara_amd.plan import Node, Plan, Var
    key = (op, tuple(ins), tuple(outs), repr(sorted(params.items())), repr(sorted(kw.items())))
    ex = _EX.get(key)
    if ex is None:
        vs = {i: Var(i, dt, [None] * nd) for i, (dt, nd) in enumerate(list(ins) + list(outs))}
        n = len(ins)
        out_ids = list(range(n, n + len(outs)))
        ex = _EX[key] = PlanExecutor(Plan(op, vs, list(range(n)), out_ids,
                                          [Node(op, list(range(n)), out_ids, params)]), **kw)
    return ex


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(iu.bits(got), iu.bits(want))


def cum_ws(dtype, outer, n, inner):
    return int(_lib().ahip_cumulative_ws_bytes(_code(dtype), outer, n, inner))


def argmax_ws(dtype, nrows, k, rs, cs):
    return int(_lib().ahip_argmax_ws_bytes(_code(dtype), nrows, k, rs, cs))


def sort_max_row(dtype):
    return int(_lib().ahip_sort_max_row(_code(dtype)))


# ---- gather -----------------------------------------------------------------------------------
def _take(dtype, idx_dtype="int64", **kw):
    return executor("AdvancedSubtensor1", [(dtype, 2), (idx_dtype, 1)], [(dtype, 2)], {}, **kw)


@pytest.mark.parametrize("dtype", ["int8", "uint16", "float32", "float64"])
def test_gather_rows_every_row_size_index_type_and_alignment(dtype):
    size = np.dtype(dtype).itemsize
    ex = _take(dtype)
    for row in iu.gather_rows_elems(dtype):
        x = iu.full_range(dtype, (7, row), 10 + row)
        for n in (1, 65):
            idx = iu.index_vector("int64", n, 7, n + row)
            (got,) = ex(dev(x), dev(idx))
            assert same_bits(host(got), x[idx]), (row, n)
    row = 16 * 65 // size
    x = iu.full_range(dtype, (7, row), 3)
    big = iu.index_vector("int64", 130, 7, 4)
    for idx in (big[::2], big[:65][::-1], big[::-2]):
        assert (idx < 0).any() and idx.shape == (65,)
        (got,) = ex(dev(x), dev(idx))
        assert same_bits(host(got), x[idx]), idx.strides
    for idt in iu.INDEX_DTYPES:
        idx = iu.index_vector(idt, 65, 7, 5)
        (got,) = _take(dtype, idt)(dev(x), dev(idx))
        assert same_bits(host(got), x[idx.astype("int64")]), idt
    idx = iu.index_vector("int64", 65, 7, 6)
    wide = iu.full_range(dtype, (8, row + 16 // size), 7)
    flat = iu.full_range(dtype, (7 * row + 1,), 8)
    odd = iu.full_range(dtype, (8, row + 1), 9)
    views = {"row stride beyond the row": wide[:7, :row],            # still whole 16-byte units
             "x[1:] of rows that are no multiple of 16 bytes": odd[1:],
             "x[:, 1:]": wide[:7, 1:row + 1],
             "one element in": flat[1:].reshape(7, row)}
    for what, v in views.items():
        assert v.shape[0] == 7
        (got,) = ex(dev(v), dev(idx))
        assert same_bits(host(got), v[idx]), what


# ---- scatter ----------------------------------------------------------------------------------
SCATTER_ROWS = (1, 3, 7, 8, 9, 65, 257)      # element kernel: 1, 3, 7; lane groups of 8 .. 64: the rest


@pytest.mark.parametrize("mode", ["set", "inc"])
@pytest.mark.parametrize("dtype", iu.INT_DTYPES)
def test_scatter_rows_contended_and_wrapping(dtype, mode):
    ex = executor("AdvancedIncSubtensor1", [(dtype, 2), (dtype, 2), ("int64", 1)], [(dtype, 2)],
                  {"set_instead_of_inc": mode == "set", "inplace": False})
    for row in SCATTER_ROWS:
        dst, idx, y = iu.scatter_case(dtype, row, 20 + row)
        want = (iu.ref_scatter_set if mode == "set" else iu.ref_scatter_add)(dst, idx, y)
        d = dev(dst)
        (got,) = ex(d, dev(y), dev(idx))
        assert np.array_equal(host(got), want), row
        assert np.array_equal(host(d), dst), row              # not in place


@pytest.mark.parametrize("mode", ["set", "inc"])
@pytest.mark.parametrize("dtype", iu.SMALL_INTS)
def test_scatter_rows_into_a_destination_one_element_into_its_allocation(dtype, mode):
    """C ABI (a plan always scatters into a fresh, aligned copy): the end of one row and the start
    of the next share a 32-bit word, and so do the destination and its neighbours in the buffer."""
    import torch
    from aesara_amd._lib import check
    lib = _lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    size = np.dtype(dtype).itemsize
    for row in (1, 3, 7, 9, 65):
        dst, idx, y = iu.scatter_case(dtype, row, 40 + row)
        base = iu.full_range(dtype, (3 * row + 8,), row)
        base[1:1 + 3 * row] = dst.reshape(-1)
        want = base.copy()
        want[1:1 + 3 * row] = (iu.ref_scatter_set if mode == "set" else iu.ref_scatter_add)(dst, idx, y).reshape(-1)
        tb, ti, ty = dev(base), dev(idx), dev(y)
        bad = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert (tb.data_ptr() + size) % 4 != 0
        check(lib.ahip_scatter_rows(_code(dtype), C.c_void_p(tb.data_ptr() + size), 3, row, row,
                                    C.c_void_p(ti.data_ptr()), _code("int64"), idx.size, 1,
                                    C.c_void_p(ty.data_ptr()), row, 1 if mode == "inc" else 0,
                                    C.c_void_p(bad.data_ptr()), stream))
        torch.cuda.synchronize()
        assert int(bad.item()) == 0
        assert np.array_equal(host(tb), want), row           # the neighbours of the view included


@pytest.mark.parametrize("kind", ["set", "inc", "ignore_duplicates"])
def test_nd_inc_subtensor_int16(kind):
    rng = np.random.default_rng(3)
    x = iu.full_range("int16", (6, 5), 1)
    i0 = rng.integers(-6, 6, size=40).astype("int64")
    i1 = rng.integers(-5, 5, size=40).astype("int64")
    y = iu.scatter_case("int16", 1, 2, nidx=40)[2].reshape(40)
    params = {"set_instead_of_inc": kind == "set", "inplace": False}
    if kind == "ignore_duplicates":
        params["ignore_duplicates"] = True
    want = x.copy()
    if kind == "set":
        for a, b, v in zip(i0, i1, y):
            want[a, b] = v
    elif kind == "inc":
        np.add.at(want, (i0, i1), y)
    else:
        want[i0, i1] += y
    ex = executor("AdvancedIncSubtensor", [("int16", 2), ("int16", 1), ("int64", 1), ("int64", 1)],
                  [("int16", 2)], params)
    (got,) = ex(dev(x), dev(y), dev(i0), dev(i1))
    assert np.array_equal(host(got), want)
    assert len(set(zip((i0 % 6).tolist(), (i1 % 5).tolist()))) < 40       # there are duplicates


# ---- N-d integer indexing ---------------------------------------------------------------------
MIXED = ("int8", "uint16", "int64")


def _nd_indices(shape, k, n, seed, dtypes=MIXED):
    rng = np.random.default_rng(seed)
    out = []
    for d in range(k):
        dt = dtypes[d % len(dtypes)]
        lo = -shape[d] if np.dtype(dt).kind == "i" else 0
        out.append(rng.integers(lo, shape[d], size=n).astype(dt))
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_nd_gather_mixed_index_types(k):
    shape = {1: (5, 4), 2: (5, 4, 3), 3: (5, 4, 3, 2), 8: (2,) * 8}[k]
    x = iu.full_range("float32", shape, k)
    idx = _nd_indices(shape, k, 9, 30 + k)
    assert any((i.astype("int64") < 0).any() for i in idx)
    ex = executor("AdvancedSubtensor", [("float32", len(shape))] + [(i.dtype.name, 1) for i in idx],
                  [("float32", 1 + len(shape) - k)], {})
    (got,) = ex(dev(x), *[dev(i) for i in idx])
    assert same_bits(host(got), x[tuple(i.astype("int64") for i in idx)])
    # the same entries through strided and reversed index views
    big = _nd_indices(shape, k, 18, 40 + k)
    views = [b[::2] if d % 2 == 0 else b[::-2] for d, b in enumerate(big)]
    (got,) = ex(dev(x), *[dev(v) for v in views])
    assert same_bits(host(got), x[tuple(v.astype("int64") for v in views)])


def test_nd_gather_broadcast_index_shapes():
    x = iu.full_range("float64", (5, 4, 3), 1)
    i0 = np.array([[-5], [2], [4]], "int8")
    i1 = np.array([3, 0, 2, 1], "uint16")
    i2 = np.array(-1, "int64")
    ex = executor("AdvancedSubtensor", [("float64", 3), ("int8", 2), ("uint16", 1), ("int64", 0)],
                  [("float64", 2)], {})
    (got,) = ex(dev(x), dev(i0), dev(i1), dev(i2))
    want = x[i0.astype("int64"), i1.astype("int64"), i2]
    assert want.shape == (3, 4) and same_bits(host(got), want)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_nd_index_errors_leave_the_executor_usable(k):
    shape = (4, 3, 2, 2)[:k + 1]
    x = np.arange(int(np.prod(shape)), dtype="int32").reshape(shape)
    xd = dev(x)
    for dt in ("int64", "uint64"):
        ex = executor("AdvancedSubtensor", [("int32", k + 1)] + [(dt, 1)] * k, [("int32", 2)], {})
        good = _nd_indices(shape, k, 5, 50 + k, dtypes=(dt,))

        def check_good():
            (got,) = ex(xd, *[dev(i) for i in good])
            assert np.array_equal(host(got), x[tuple(i.astype("int64") for i in good)])
        check_good()
        if dt == "int64":      # one past the end and -dim - 1, in every array (the second one included)
            bads = [(d, v) for d in range(k) for v in (shape[d], -shape[d] - 1)]
        else:                  # beyond int64: as a signed value these would be -1, int64's minimum and -dim
            bads = [(d, v) for d in range(k) for v in (2 ** 64 - 1, 2 ** 63, 2 ** 64 - shape[d])]
        for pos, value in bads:
            bad = [i.copy() for i in good]
            bad[pos][3] = value
            with pytest.raises(IndexError):
                ex(xd, *[dev(i) for i in bad])
            check_good()


# ---- argmax -----------------------------------------------------------------------------------
def _argmax(dtype, axis):
    return executor("Argmax", [(dtype, 2)], [("int64", 1)], {"axis": [axis]})


@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_argmax_row_form(dtype):
    V = 16 // np.dtype(dtype).itemsize
    ex = _argmax(dtype, 1)
    for k in (1, 63, 64, 65, V * 129):
        x = iu.argmax_lines(dtype, 18, k, k)
        assert argmax_ws(dtype, 18, k, k if k > 1 else 1, 1 if k > 1 else 0) == 0      # row form
        (got,) = ex(dev(x))
        assert np.array_equal(host(got), np.argmax(x, axis=1)), k
        v = iu.argmax_lines(dtype, 18, k + 1, k + 100)[:, 1:]                          # misaligned rows
        assert argmax_ws(dtype, 18, k, k + 1, 1 if k > 1 else 0) == 0
        (got,) = ex(dev(v))
        assert np.array_equal(host(got), np.argmax(v, axis=1)), k


@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_argmax_column_form_sliced(dtype):
    V = 16 // np.dtype(dtype).itemsize
    ex = _argmax(dtype, 0)
    for nout in (16, 17, 128 * V + V):
        for k in (64, 65, 100):
            x = np.ascontiguousarray(iu.argmax_lines(dtype, nout, k, nout + k).T)
            assert x.shape == (k, nout)
            assert argmax_ws(dtype, nout, k, 1, nout) > 0, (nout, k)     # sliced column form + fold
            (got,) = ex(dev(x))
            assert np.array_equal(host(got), np.argmax(x, axis=0)), (nout, k)


# ---- sort / argsort ---------------------------------------------------------------------------
def _sort_ex(op, dtype):
    from aesara_amd.executor import PlanExecutor
    from aesara_amd.plan import Node, Plan, Var
    key = (op, dtype)
    if key not in _EX:
        vs = {0: Var(0, dtype, [None, None]), 1: Var(1, "int64", []),
              2: Var(2, "int64" if op == "ArgSort" else dtype, [None, None])}
        _EX[key] = PlanExecutor(Plan(op, vs, [0, 1], [2], [Node(op, [0, 1], [2], {"kind": "quicksort"})]))
    return _EX[key]


def _sort_lengths(dtype):
    M = sort_max_row(dtype)
    size = np.dtype(dtype).itemsize
    assert M * (size + 4) <= 64 * 1024 < 2 * M * (size + 4)            # the LDS limit
    assert M == (4096 if size == 8 else 8192)
    return M, (1, 2, 3, 5, 64, 65, M - 1, M, M + 1, 2 * M + 1, 3 * M)


@pytest.mark.parametrize("layout", ["last", "first", "reversed"])
@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_sort_and_argsort(dtype, layout):
    M, lengths = _sort_lengths(dtype)
    for n in lengths:
        for rows in (1, 3):
            keys = iu.sort_keys(dtype, (rows, n), n + rows)
            if layout == "last":
                x, axis = keys, 1
            elif layout == "first":
                x, axis = np.ascontiguousarray(keys.T), 0               # the sorted axis has stride `rows`
            else:
                x, axis = np.ascontiguousarray(keys[:, ::-1])[:, ::-1], 1
            order = iu.stable_argsort(x, axis)
            (gi,) = _sort_ex("ArgSort", dtype)(dev(x), np.int64(axis))
            assert np.array_equal(host(gi), order), (n, rows)
            (gv,) = _sort_ex("Sort", dtype)(dev(x), np.int64(axis))
            assert same_bits(host(gv), np.take_along_axis(x, order, axis)), (n, rows)


# ---- searchsorted -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_searchsorted(dtype):
    rng = np.random.default_rng(9)
    for nx in (0, 1, 2, 3, 1000):
        x, keys = iu.searchsorted_case(dtype, nx, nx)
        perm = rng.permutation(nx)
        xp = x[perm]
        sorter = iu.stable_argsort(xp)
        big, bigp = np.zeros(2 * nx, dtype), np.zeros(2 * nx, dtype)
        big[::2], bigp[::2] = x, xp
        for vshape in ((0,), (1,), (3, 5)):
            v = iu.keys_of_shape(keys, vshape)
            for side in ("left", "right"):
                plain = executor("Searchsorted", [(dtype, 1), (dtype, len(vshape))],
                                 [("int64", len(vshape))], {"side": side})
                sorted_ = executor("Searchsorted", [(dtype, 1), (dtype, len(vshape)), ("int64", 1)],
                                   [("int64", len(vshape))], {"side": side})
                want = np.searchsorted(x, v, side=side).astype("int64")
                for xs in (x, big[::2]):
                    (got,) = plain(dev(xs), dev(v))
                    assert np.array_equal(host(got), want), (nx, vshape, side)
                wants = np.searchsorted(xp, v, side=side, sorter=sorter).astype("int64")
                assert np.array_equal(wants, want)
                for xs in (xp, bigp[::2]):
                    (got,) = sorted_(dev(xs), dev(v), dev(sorter))
                    assert np.array_equal(host(got), want), (nx, vshape, side, "sorter")


# ---- nonzero ----------------------------------------------------------------------------------
NZ_SHAPES = ((37,), (5, 7), (3, 4, 5), (2, 3, 2, 3), (2,) * 5, (2, 2, 3, 2, 2, 2), (2,) * 7, (2,) * 8)


@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_nonzero(dtype):
    def run(x):
        ex = executor("Nonzero", [(dtype, x.ndim)], [("int64", 1)] * x.ndim, {})
        got = ex(dev(x))
        want = np.nonzero(x)
        assert len(got) == x.ndim
        for g, w in zip(got, want):
            g = host(g)
            assert g.dtype == np.int64 and np.array_equal(g, w), (x.shape, len(w))
        return len(want[0])
    for shape in NZ_SHAPES:
        n = run(iu.nonzero_input(dtype, shape, len(shape)))
        assert 0 < n < int(np.prod(shape))
    assert run(iu.nonzero_input(dtype, (9, 5), 1, "clear")) == 0
    assert run(iu.nonzero_input(dtype, (9, 5), 1, "set")) == 45
    n = 2051
    assert cum_ws("int64", 1, n, 1) > 0            # the running count behind it is chunked
    assert 0 < run(iu.nonzero_input(dtype, (n,), 2)) < n
    assert run(iu.nonzero_input(dtype, (n,), 2, "set")) == n


# ---- cumulative -------------------------------------------------------------------------------
def _cum_input(dtype, mode, shape, axis, seed):
    ax = 0 if axis is None else axis
    return iu.prod_input(dtype, shape, ax, seed) if mode == "mul" else iu.sum_input(dtype, shape, seed)


def _cum(dtype, mode, x, axis):
    ex = executor("CumOp", [(dtype, x.ndim)], [(dtype, 1 if axis is None else x.ndim)],
                  {"axis": axis, "mode": mode})
    (got,) = ex(dev(x))
    return host(got)


@pytest.mark.parametrize("mode", ["add", "mul"])
@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_cumulative_flat_lengths(dtype, mode):
    V = 16 // np.dtype(dtype).itemsize
    for n in (1, 63, 64, 65, 256, 257, 64 * V - 1, 64 * V, 64 * V + V, 64 * V + 1):
        assert cum_ws(dtype, 1, n, 1) == 0, n                    # single pass
        x = _cum_input(dtype, mode, (n,), 0, n)
        assert same_bits(_cum(dtype, mode, x, 0), iu.ref_cum(x, 0, mode)), n
    chunked = [n for n in (2048, 2051, 4096 + 64 * V) if cum_ws(dtype, 1, n, 1) > 0]
    assert chunked, "no flat length takes the chunked form"
    for n in (chunked[0], chunked[0] + 1):
        assert cum_ws(dtype, 1, n, 1) > 0, n                     # reduce, scan the totals, scan
        x = _cum_input(dtype, mode, (n,), 0, n)
        assert same_bits(_cum(dtype, mode, x, 0), iu.ref_cum(x, 0, mode)), n
    # a view that starts one element in (the element form), and the largest extent of the matrix
    n = 64 * V
    x = _cum_input(dtype, mode, (n + 1,), 0, 5)[1:]
    assert same_bits(_cum(dtype, mode, x, 0), iu.ref_cum(x, 0, mode))
    x = _cum_input(dtype, mode, (1 << 16,), 0, 6)
    assert cum_ws(dtype, 1, 1 << 16, 1) > 0
    assert same_bits(_cum(dtype, mode, x, 0), iu.ref_cum(x, 0, mode))


@pytest.mark.parametrize("mode", ["add", "mul"])
@pytest.mark.parametrize("dtype", iu.DTYPES)
def test_cumulative_lines_and_views(dtype, mode):
    V = 16 // np.dtype(dtype).itemsize
    for shape, axis in (((130, 64), 0), ((3, 200, 65), 1), ((130, 64 * V), 0), ((130, 64 * V + 1), 0)):
        outer = int(np.prod(shape[:axis]))
        inner = int(np.prod(shape[axis + 1:]))
        assert inner >= 64 and cum_ws(dtype, outer, shape[axis], inner) > 0, shape   # thread per line, chunked
        x = _cum_input(dtype, mode, shape, axis, sum(shape))
        assert same_bits(_cum(dtype, mode, x, axis), iu.ref_cum(x, axis, mode)), shape
    for axis in (0, 1):                                          # a transposed view
        x = np.ascontiguousarray(_cum_input(dtype, mode, (130, 64), axis, 7 + axis).T).T
        assert x.shape == (130, 64) and x.strides[0] == x.itemsize
        assert same_bits(_cum(dtype, mode, x, axis), iu.ref_cum(x, axis, mode)), axis
    x = _cum_input(dtype, mode, (8, 64 * V + 1), 1, 9)[:, 1:]   # rows that start one element in
    assert same_bits(_cum(dtype, mode, x, 1), iu.ref_cum(x, 1, mode))
    m = _cum_input(dtype, mode, (65,), 0, 10).reshape(5, 13)     # axis=None on a matrix
    assert same_bits(_cum(dtype, mode, m, None), iu.ref_cum(m.reshape(-1), 0, mode))


# ---- replay -----------------------------------------------------------------------------------
def _replay_cases():
    f32, i64 = "float32", "int64"
    return {
        "gather": ("AdvancedSubtensor1", [(f32, 2), (i64, 1)], [(f32, 2)], {},
                   lambda s: [iu.full_range(f32, (7, 260), s), iu.index_vector(i64, 65, 7, s)],
                   lambda a: [a[0][a[1]]]),
        "scatter_add": ("AdvancedIncSubtensor1", [("int16", 2), ("int16", 2), (i64, 1)], [("int16", 2)],
                        {"set_instead_of_inc": False, "inplace": False},
                        lambda s: [iu.scatter_case("int16", 9, s)[j] for j in (0, 2, 1)],
                        lambda a: [iu.ref_scatter_add(a[0], a[2], a[1])]),
        "scatter_set": ("AdvancedIncSubtensor1", [("uint8", 2), ("uint8", 2), (i64, 1)], [("uint8", 2)],
                        {"set_instead_of_inc": True, "inplace": False},
                        lambda s: [iu.scatter_case("uint8", 9, s)[j] for j in (0, 2, 1)],
                        lambda a: [iu.ref_scatter_set(a[0], a[2], a[1])]),
        "nd_gather": ("AdvancedSubtensor", [(f32, 3), ("int8", 1), ("uint16", 1)], [(f32, 2)], {},
                      lambda s: [iu.full_range(f32, (5, 4, 3), s)] + _nd_indices((5, 4), 2, 9, s),
                      lambda a: [a[0][a[1].astype(i64), a[2].astype(i64)]]),
        "argmax": ("Argmax", [("uint64", 2)], [(i64, 1)], {"axis": [1]},
                   lambda s: [iu.argmax_lines("uint64", 18, 258, s)], lambda a: [np.argmax(a[0], axis=1)]),
        "sort": ("Sort", None, None, None,
                 lambda s: [iu.sort_keys(f32, (3, 8193), s)],
                 lambda a: [np.take_along_axis(a[0], iu.stable_argsort(a[0], 1), 1)]),
        "argsort": ("ArgSort", None, None, None,
                    lambda s: [iu.sort_keys(f32, (3, 65), s)], lambda a: [iu.stable_argsort(a[0], 1)]),
        "searchsorted": ("Searchsorted", [("uint64", 1), ("uint64", 2)], [(i64, 2)], {"side": "right"},
                         lambda s: [iu.searchsorted_case("uint64", 1000, s)[0],
                                    iu.keys_of_shape(iu.searchsorted_case("uint64", 1000, s)[1], (3, 5))],
                         lambda a: [np.searchsorted(a[0], a[1], side="right").astype(i64)]),
        "nonzero": ("Nonzero", [(f32, 2)], [(i64, 1)] * 2, {},
                    lambda s: [iu.nonzero_input(f32, (9, 5), s)], lambda a: list(np.nonzero(a[0]))),
        "cumsum": ("CumOp", [(f32, 1)], [(f32, 1)], {"axis": 0, "mode": "add"},
                   lambda s: [iu.sum_input(f32, (2051,), s)], lambda a: [iu.ref_cum(a[0], 0, "add")]),
        "cumprod": ("CumOp", [("int8", 2)], [("int8", 2)], {"axis": 0, "mode": "mul"},
                    lambda s: [iu.prod_input("int8", (130, 64), 0, s)], lambda a: [iu.ref_cum(a[0], 0, "mul")]),
    }


@pytest.mark.parametrize("name", sorted(_replay_cases()))
def test_replayed_executor_gives_the_same_results(name):
    from aesara_amd.executor import PlanExecutor
    from aesara_amd.plan import Node, Plan, Var
    op, ins, outs, params, make, ref = _replay_cases()[name]
    if op in ("Sort", "ArgSort"):
        vs = {0: Var(0, "float32", [None, None]), 1: Var(1, "int64", []),
              2: Var(2, "int64" if op == "ArgSort" else "float32", [None, None])}
        ex = PlanExecutor(Plan(op, vs, [0, 1], [2], [Node(op, [0, 1], [2], {"kind": "quicksort"})]),
                          use_graph=True)
        extra = [np.int64(1)]
    else:
        ex = executor(op, ins, outs, params, use_graph=True)
        extra = []
    for seed in (1, 2):
        args = make(seed)
        got = ex(*[dev(a) for a in args], *extra)
        want = ref(args)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert same_bits(host(g), w), (name, seed)
