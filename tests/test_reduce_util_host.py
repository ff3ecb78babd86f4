"""Host checks of tests/reduce_util.py: the bit-exact comparisons of tests/test_gpu_reduce_matrix.py
rest on these properties.  NumPy and dry runs of the executor only, no device."""
import numpy as np
import pytest

import index_util as iu
import interp
import reduce_util as ru


def _fold(op, dtype, xs):
    """left fold of a 1-d array in ``dtype`` arithmetic (NumPy scalars, one element at a time)"""
    f = {"add": np.add, "mul": np.multiply}[op]
    acc = xs[0]
    for x in xs[1:]:
        acc = f(acc, x, dtype=dtype)
    return acc


@pytest.mark.parametrize("dtype", iu.FLOATS)
@pytest.mark.parametrize("op", ["add", "mul", "mul_without_zeros"])
def test_float_runs_are_exact_under_any_order_and_any_cut(op, dtype):
    """random permutations, random cuts into contiguous partials and strided partials (lane l
    takes elements l, l + 64, ...: what a reduce kernel does) all give the bits of the reference,
    in the input type as in float64"""
    nred = 5000
    r = ru.runs(op, dtype, 3, nred, 7)
    want = ru.ref_runs(op, r, dtype, dtype)
    assert np.array_equal(ru.canon(want), ru.canon(ru.ref_runs(op, r, "float64", dtype)))
    rng = np.random.default_rng(1)
    plain = "mul" if op != "add" else "add"
    for i in range(3):
        row = r[i][r[i] != 0] if op == "mul_without_zeros" else r[i]
        assert row.size > nred // 2
        for trial in range(4):
            perm = row[rng.permutation(row.size)]
            assert iu.bits(_fold(plain, dtype, perm)) == iu.bits(want[i]), (op, dtype, "permuted")
            cuts = [0] + sorted(int(c) for c in rng.integers(1, row.size, size=5)) + [row.size]
            parts = [_fold(plain, dtype, row[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if a < b]
            assert iu.bits(_fold(plain, dtype, np.array(parts, dtype))) == iu.bits(want[i]), (op, dtype, "cut")
            lanes = int(rng.choice([2, 64, 256]))
            parts = [_fold(plain, dtype, row[l::lanes]) for l in range(lanes)]
            assert iu.bits(_fold(plain, dtype, np.array(parts[::-1], dtype))) == iu.bits(want[i]), (op, dtype, "lanes")
    if op != "add":
        e = np.log2(np.abs(np.where(r == 0, 1, r).astype("float64")))
        assert np.abs(e).sum(axis=1).max() <= 60 and (r < 0).any() and (e > 0).any() and (e < 0).any()


def test_index_util_products_are_not_exact_for_strided_partials():
    """why float mul does not reuse iu.prod_input: it bounds the exponent of every CONSECUTIVE run,
    but the partial of a lane (every 64th element) of a long walk leaves float32"""
    x = iu.prod_input("float32", (1 << 20,), 0, 11).astype("float64")
    e = np.log2(np.abs(x))
    assert np.abs(np.cumsum(e)).max() <= 20
    assert max(abs(e[l::64].sum()) for l in range(64)) > 126


@pytest.mark.parametrize("op", ["maximum", "minimum"])
def test_one_sided_runs_hold_nothing_on_the_other_side_of_the_identity(op):
    for dtype in iu.DTYPES:
        lo, hi = iu.limits(dtype)
        for kind in ("onesided", "extreme"):
            r = ru.runs(op, dtype, 6, 300, 3, kind)
            assert r.dtype == np.dtype(dtype) and not (r == 0).any() or lo == 0
            if op == "maximum" and lo < 0:
                assert (r < 0).all()                 # a zero where -inf / the minimum belongs would win
            if op == "minimum":
                assert (r > 0).all()
            if kind == "extreme":
                assert (r[0::2] == (lo if op == "maximum" else hi)).all()
                ext = ru.ref_runs(op, r, dtype, dtype)
                assert (ext[0::2] == (lo if op == "maximum" else hi)).all()
        p = ru.runs(op, dtype, 6, 300, 3)
        if iu.is_float(dtype):                       # no zero of either sign, no NaN, both infinities
            assert not (p == 0).any() and not np.isnan(p).any() and (p == np.inf).any() and (p == -np.inf).any()


def test_bit_and_zero_runs():
    for dtype in iu.INT_DTYPES + ("bool",):
        ones = ru.runs("and", dtype, 4, 100, 2, "ones")
        w = ru.ref_runs("and", ones, dtype, dtype)
        all_ones = np.array([True, True]) if dtype == "bool" else np.array([-1, -1]).astype(dtype)
        assert np.array_equal(iu.bits(w[0::2]), iu.bits(all_ones))
        zeros = ru.runs("or", dtype, 4, 100, 2, "zeros")
        assert not ru.ref_runs("or", zeros, dtype, dtype)[0::2].any()
    for dtype in ("int32", "float32", "uint8"):
        z = ru.runs("mul_without_zeros", dtype, 4, 200, 2, "zeros")
        w = ru.ref_runs("mul_without_zeros", z, dtype, dtype)
        assert (z[0::2] == 0).all() and (w[0::2] == 0).all() and (w[1::2] != 0).all()
        assert (z[1::2] == 0).any()                  # zeros to skip in the other runs
        if dtype == "float32":
            assert not np.signbit(z[z == 0]).any()


@pytest.mark.parametrize("op", ru.OPS)
def test_references_agree_with_the_oracle_at_a_tiny_shape(op):
    for v in ru.variants(op):
        for kind in ru.kinds(op, v[0]):
            r = ru.runs(op, v[0], 4, 9, 5, kind)
            want = interp.careduce(r, op, [1], v[1], v[2])
            got = ru.ref_runs(op, r, v[1], v[2])
            assert got.dtype == want.dtype and np.array_equal(ru.canon(got), ru.canon(want)), (op, v, kind)
            a = ru.place(r, (3, 4, 3), (0, 2), None)
            want3 = interp.careduce(a, op, [0, 2], v[1], v[2])
            assert np.array_equal(ru.canon(want3), ru.canon(got)), (op, v, kind, "placed")
        if op not in ("maximum", "minimum"):
            v = ru.variants(op)[-1]
            e = interp.careduce(np.zeros((0,), v[0]), op, None, v[1], v[2])
            assert np.array_equal(ru.canon(e), ru.canon(ru.empty_result(op, v[1], v[2])))


def test_integer_references_wrap_and_only_wrap():
    for dtype in iu.INT_DTYPES:
        r = ru.runs("add", dtype, 2, 3000, 9)
        wide = [sum(int(x) for x in row) for row in r]
        got = ru.ref_runs("add", r, dtype, dtype)
        bits_ = 8 * np.dtype(dtype).itemsize
        assert any(int(g) != w for g, w in zip(got, wide))
        assert all(int(g) % (1 << bits_) == w % (1 << bits_) for g, w in zip(got, wide))
        p = ru.runs("mul", dtype, 2, 300, 9)
        widep = [1, 1]
        for i in range(2):
            for x in p[i]:
                widep[i] *= int(x)
        gotp = ru.ref_runs("mul", p, dtype, dtype)
        assert all(int(g) % (1 << bits_) == w % (1 << bits_) and int(g) % 2 for g, w in zip(gotp, widep))
        if dtype in ru.WIDE:
            w64 = ru.ref_runs("add", r, ru.WIDE[dtype], ru.WIDE[dtype])
            assert [int(x) for x in w64] == wide       # the 64-bit accumulator holds the whole sum


def test_views_place_the_runs():
    r = np.arange(24, dtype="int16").reshape(4, 6)
    for view in (None, "T", "rev_step", "step", "off1"):
        a = ru.place(r, (6, 4), (0,), view)
        assert a.shape == (6, 4) and np.array_equal(a.sum(axis=0), r.sum(axis=1))
        base, off, strides = ru.geometry(a)
        picked = [base[off + sum(i * s for i, s in zip(ix, strides))] for ix in np.ndindex(*a.shape)]
        assert picked == a.reshape(-1).tolist(), view
    assert ru.geometry(ru.place(r, (4, 6), (1,), "off1"))[1] == 1
    assert ru.geometry(ru.place(r, (4, 6), (1,), "rev_step"))[2][0] < 0
    assert ru.geometry(ru.place(r, (6, 4), (0,), "T"))[2] == [1, 6]
    base, _, strides = ru.geometry(ru.place(r, (4, 6), (1,), "step"))
    assert strides == [13, 2] and len(set(base.tolist())) > 1


# ---- the shapes of the form table select the forms they are named after (dry runs) ----------------
@pytest.fixture
def dry(monkeypatch):
    """executor dry runs that record the selected kernels without cross-compiling them (the device
    tests compile and run every one of them; tests/test_host_logic.py covers dry-run compilation)"""
    import aesara_amd.device as device
    from aesara_amd.executor import PlanExecutor
    monkeypatch.setattr(device, "compile_cached", lambda source: b"")

    def make(plan):
        ex = PlanExecutor(plan, dry_run=True)
        return ex, ru.Spy(ex)
    return make


_VARIANTS = sorted({v for _, v in ru.SIX} | {("uint16", "uint64", "uint64"), ("int64",) * 3, ("uint32",) * 3})


@pytest.mark.parametrize("v", _VARIANTS, ids=[ru.vid(v) for v in _VARIANTS])
def test_every_shape_of_the_table_selects_its_form(dry, v):
    dt = v[0]
    for form in ru.AXIS_FORMS:
        shape = ru.resolve(form.shape, dt)
        nred = int(np.prod([shape[d] for d in form.axis]))
        ex, spy = dry(ru.reduce_plan(v, len(shape), form.axis, "add" if dt != "float64" else "maximum"))
        ex(ru.fake_dev(ru.place(np.zeros((int(np.prod(shape)) // nred, nred), dt), shape, form.axis, form.view)))
        ru.check_axis_form(form, dt, spy, nred)
        if "nslices" in form.expect:            # two passes: the partials are [nslices, nkept] of the accumulator
            assert spy.names().count("ahip_elemwise_reduce_axis") == 2
            k2 = [k for k in spy.memo("axis") if k[3] == (v[1],)]
            assert k2 and all(k[12] == v[1] for k in spy.memo("axis")), spy.memo("axis")
    for form in ru.full_forms(dt):
        ex, spy = dry(ru.reduce_plan(v, len(form.shape), None, "mul"))
        ex(ru.fake_dev(ru.place(np.zeros((1, int(np.prod(form.shape))), dt), form.shape, None, form.view)))
        ru.check_full_form(form, spy)
    for name, xs, ys, yview, expect in ru.PAIR_FORMS:
        ex, spy = dry(ru.pair_plan(v, "minimum" if dt != "bool" else "add"))
        y = np.zeros(ys, dt)
        ex(ru.fake_dev(np.zeros(xs, dt)), ru.fake_dev(np.ascontiguousarray(y.T).T if yview == "T" else y))
        ru.check_pair_form(name, expect, spy)
        assert ("ahip_elemwise_tiled" in spy.names()) == name.startswith("tiled")
    ex, spy = dry(ru.towers_plan(v, "and" if dt not in iu.FLOATS else "mul", 3))
    ex(*[ru.fake_dev(np.zeros(n, dt)) for n in ru.hgroup_lengths(dt)])
    assert spy.names() == ["ahip_elemwise_reduce_all_multi"]


def test_lengths_against_the_launchers_grid_arithmetic():
    """the partial counts the full-reduction lengths are sized for (csrc/elemwise_launch.hip)"""
    for dt in ("int8", "float64"):
        b, v = ru.red_block(), ru.flat_vec(dt)
        forms = {f.name: f for f in ru.full_forms(dt)}
        items = forms["flat_ragged"].shape[0] // v
        assert 1 < -(-items // b) <= 8 and items % b and forms["flat_ragged"].shape[0] % v == 0
        assert forms["flat_over_cap"].shape[0] // v > ru.flat_cap() * b
        assert forms["flat_over_cap"].shape[0] * np.dtype(dt).itemsize <= 9 << 20
        lens = ru.hgroup_lengths(dt)
        cap = ru.CUS * max(1, 8 * 256 // b)                  # the group's grid, shared by items
        share = -(-cap * (lens[2] // v) // sum(n // v for n in lens))
        assert min(share, -(-(lens[2] // v) // b)) > 256     # two collecting waves
    name, xs, _, _, _ = ru.PAIR_FORMS[-1]
    assert name == "tiled_many" and -(-xs[0] // 32) * -(-xs[1] // 32) > 256 and min(xs) < 48


def test_empty_last_slices_exist():
    for name in ("row_sliced_empty_last", "col_sliced_empty_last"):
        f = ru.axis_form(name)
        nred = f.shape[1] if name.startswith("row") else f.shape[0]
        per, empty = ru.sliced_geometry(nred, 1, f.expect["nslices"])
        assert empty and per * (f.expect["nslices"] - 1) >= nred
    assert not ru.sliced_geometry(2049, 1, 8)[1] and not ru.sliced_geometry(1027, 1, 8)[1]
