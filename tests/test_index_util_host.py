"""Host checks of the generators and references in tests/index_util.py: the bit-exact comparisons
of tests/test_gpu_index_sort_scan.py rest on these properties.  NumPy only, no device."""
import math

import numpy as np
import pytest

import index_util as iu


@pytest.mark.parametrize("dtype", iu.FLOATS)
def test_sum_inputs_have_exact_prefix_sums_under_any_cut(dtype):
    n = 1 << 16
    x = iu.sum_input(dtype, (n,), 3)
    assert x.dtype == np.dtype(dtype) and set(np.unique(x)) <= set(range(-3, 4))
    wide = np.cumsum(x.astype("float64"))
    assert np.array_equal(wide, np.round(wide)) and np.abs(wide).max() < 2 ** 24   # exact in float32
    same = np.cumsum(x, dtype=dtype)
    assert np.array_equal(iu.bits(wide.astype(dtype)), iu.bits(same))
    rng = np.random.default_rng(5)
    for _ in range(4):
        cuts = [0] + sorted(int(c) for c in rng.integers(1, n, size=3)) + [n]
        pieces, carry = [], np.zeros((), dtype)
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == b:
                continue
            part = np.cumsum(x[a:b], dtype=dtype)          # scanned on its own ...
            pieces.append((part + carry).astype(dtype))     # ... and offset by the pieces before it
            carry = (carry + part[-1]).astype(dtype)
        assert np.array_equal(np.concatenate(pieces), same)


@pytest.mark.parametrize("dtype", iu.FLOATS)
def test_product_inputs_keep_every_prefix_exponent_within_20(dtype):
    for shape, axis in (((1 << 16,), 0), ((130, 64), 0), ((3, 200, 65), 1)):
        x = iu.prod_input(dtype, shape, axis, 11)
        assert x.dtype == np.dtype(dtype)
        assert set(np.unique(np.abs(x))) <= {0.5, 1.0, 2.0} and (x[np.abs(x) != 1] > 0).all()
        e = np.cumsum(np.log2(np.abs(x.astype("float64"))), axis=axis)
        assert e.min() >= -20 and e.max() <= 20
        assert np.array_equal(e, iu.prod_exponents(shape, axis, 11))
        assert e.max() - e.min() > 20                     # the walk does reach a wall
        wide = np.cumprod(x.astype("float64"), axis=axis)
        assert np.array_equal(iu.bits(wide.astype(dtype)), iu.bits(iu.ref_cum(x, axis, "mul")))
    x = iu.prod_input(dtype, (1 << 16,), 0, 11)
    assert (x == -1).any() and (x == 2).any() and (x == 0.5).any()


def test_stable_argsort_reference_matches_pure_python_sorted():
    nan, nnan = float("nan"), -float("nan")
    for dtype in iu.FLOATS:
        x = np.array([2.0, nan, -0.0, 0.0, 2.0, -np.inf, nnan, 0.0, -0.0, np.inf, 2.0, nan], dtype)
        assert x.size == 12
        vals = x.tolist()
        want = sorted(range(x.size), key=lambda i: (1, 0.0) if math.isnan(vals[i]) else (0, vals[i]))
        assert iu.stable_argsort(x).tolist() == want
        assert want[-3:] == [1, 6, 11] and want[1:5] == [2, 3, 7, 8]      # NaNs last, zeros in input order
    for dtype in iu.DTYPES:
        x = iu.sort_keys(dtype, (300,), 2)
        vals = x.tolist()
        want = sorted(range(x.size), key=lambda i: (1, 0) if vals[i] != vals[i] else (0, vals[i]))
        assert iu.stable_argsort(x).tolist() == want
        assert len(set(iu.bits(x).tolist())) <= 9 < x.size           # many ties


@pytest.mark.parametrize("dtype", iu.INT_DTYPES)
def test_scatter_inputs_contend_and_wrap(dtype):
    for row in (1, 3, 9):
        dst, idx, y = iu.scatter_case(dtype, row, 7)
        assert idx.shape == (4096,) and y.shape == (4096, row) and dst.shape == (3, row)
        assert (idx < 0).any() and (idx >= 0).any()
        assert set((idx % 3).tolist()) == {0, 1, 2}              # every destination row is hit
        if dtype in iu.SMALL_INTS:
            for offset in (0, 1):
                lanes = iu.word_lanes(dtype, 3, row, idx, offset)
                assert max(len(v) for v in lanes.values()) >= 2  # two columns of one 32-bit word
        got = iu.ref_scatter_add(dst, idx, y)
        wide = iu.wide_scatter_add(dst, idx, y)
        assert got.dtype == np.dtype(dtype)
        assert (got.astype(object) != wide).any()                # the sums really wrap ...
        bits_ = 8 * np.dtype(dtype).itemsize
        back = np.array([[int(v) % (1 << bits_) for v in r] for r in wide], dtype=object)
        assert (got.astype(object) % (1 << bits_) == back).all()  # ... and only wrap
        last = iu.ref_scatter_set(dst, idx, y)
        for r in range(3):
            assert np.array_equal(last[r], y[np.flatnonzero(idx % 3 == r)[-1]])


@pytest.mark.parametrize("dtype", iu.INT_DTYPES)
def test_integer_scan_references_wrap(dtype):
    n = 300
    x = iu.sum_input(dtype, (n,), 13)
    wide = np.cumsum(x.astype(object))
    assert (iu.ref_cum(x, 0, "add").astype(object) != wide).any()
    p = iu.prod_input(dtype, (n,), 0, 13)
    widep = np.cumprod(p.astype(object))
    got = iu.ref_cum(p, 0, "mul")
    assert (got.astype(object) != widep).any() and (got != 0).all()
    bits_ = 8 * np.dtype(dtype).itemsize
    assert all(int(a) % (1 << bits_) == int(b) % (1 << bits_) for a, b in zip(got.tolist(), widep.tolist()))


def test_float_specials_are_present_in_moved_data():
    for dtype in iu.FLOATS:
        x = iu.full_range(dtype, (7, 64), 1)
        b = iu.bits(x)
        assert np.isnan(x).any() and (np.signbit(x) & np.isnan(x)).any()
        assert len(set(b[np.isnan(x)].tolist())) >= 3            # payloads differ
        assert ((x == 0) & np.signbit(x)).any() and ((x == 0) & ~np.signbit(x)).any()
        k = iu.sort_keys(dtype, (400,), 1)
        assert np.isnan(k).any() and np.isinf(k).any() and ((k == 0) & np.signbit(k)).any()


def test_argmax_and_searchsorted_cases_reach_their_edges():
    u = iu.argmax_lines("uint64", 18, 65, 1)
    assert (u >= 2 ** 63).any() and (u < 2 ** 63).any()
    line = u[iu.ARGMAX_CASES.index("extremes")]
    assert int(line.max()) >= 2 ** 63 and np.argmax(line) != np.argmax(line.view("int64"))
    i = iu.argmax_lines("int64", 18, 65, 1)
    assert (i[iu.ARGMAX_CASES.index("all_min")] == np.iinfo("int64").min).all()
    f = iu.argmax_lines("float32", 18, 65, 1)
    z = f[iu.ARGMAX_CASES.index("signed_zero")]
    p = int(np.argmax(z))
    assert np.signbit(z[p]) and z[p] == 0 and (p == 64 or (z[p + 1] == 0 and not np.signbit(z[p + 1])))
    assert np.argmax(f[iu.ARGMAX_CASES.index("nan_last")]) == 64
    assert np.isnan(f[iu.ARGMAX_CASES.index("nan_twice")]).sum() == 2
    for dtype in iu.DTYPES:
        x, keys = iu.searchsorted_case(dtype, 1000, 3)
        fin = x[x == x]
        assert (np.sort(fin) == fin).all() and len(np.unique(fin)) == 5 < fin.size
        assert keys[0] < fin.min() and keys[1] > fin.max()
        assert any(k in fin for k in keys.tolist()) and any(k == k and k not in fin for k in keys[2:].tolist())
        if iu.is_float(dtype):
            assert np.isnan(x[-1]) and np.isnan(keys).sum() == 2
    xu, _ = iu.searchsorted_case("uint64", 1000, 3)
    assert (xu >= 2 ** 63).any() and (xu < 2 ** 63).any()


def test_nonzero_inputs():
    for dtype in iu.DTYPES:
        m = iu.nonzero_input(dtype, (2,) * 8, 4)
        cnt = np.count_nonzero(m)
        assert 0 < cnt < m.size
        assert np.count_nonzero(iu.nonzero_input(dtype, (9, 5), 4, "clear")) == 0
        assert np.count_nonzero(iu.nonzero_input(dtype, (9, 5), 4, "set")) == 45
        if iu.is_float(dtype):
            assert np.isnan(m).any() and ((m == 0) & np.signbit(m)).any()
            assert np.signbit(iu.nonzero_input(dtype, (9, 5), 4, "clear")).all()
