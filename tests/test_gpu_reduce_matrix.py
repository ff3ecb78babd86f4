"""Every CAReduce combiner and accumulator type on every layout the reduce dispatcher can select
(exec_elemwise._run_reduce / _launch_reduce_axis): row forms with 1 .. 64 lanes, scalar and
16-byte loads, the loop-free short variant, the column form with its LDS fold, both sliced with the
second pass over the partials (also with an empty last slice), stepped / reversed / transposed
views, 3-d mixed axes; the full-reduction forms flat, scalar, n-d strided, loop-invariant operands,
LDS-tiled, the horizontal group; empty inputs; launch-list replay.

tests/reduce_util.py builds inputs whose result does not depend on the order of combination, so
every comparison is bit-exact (NaNs compare equal whatever their payload); the references are
plain NumPy / Python-integer restatements checked on the host (tests/test_reduce_util_host.py,
which also proves on dry runs that each shape selects the form it is named after: the same
assertions run here on the real executor).

Coverage: every legal (op, dtype / accumulator) pair runs on the tiny row form, the ragged sliced
row form, the ragged sliced column form and the ragged flat multi-partial form
(test_every_pair_on_four_forms); six pairs — and maximum float64 with NaNs — run on every form of
the table (test_six_pairs_on_*)."""
import zlib

import numpy as np
import pytest

import reduce_util as ru

pytestmark = pytest.mark.gpu

_EX = {}


# ---- plumbing -----------------------------------------------------------------------------------
def _executor(plan, **kw):
    from aesara_amd.executor import PlanExecutor
    return PlanExecutor(plan, **kw)


def dev(a):
    """The device image of a NumPy array with its view geometry (negative strides, which torch
    cannot express, as a DevArray over the uploaded buffer)."""
    import torch
    from aesara_amd.device import DevArray
    if a.size == 0:
        a = np.ascontiguousarray(a)
    base, off, strides = ru.geometry(a)
    name = base.dtype.name
    if name in ("uint16", "uint32", "uint64"):
        t = torch.from_numpy(base.view(name[1:])).cuda().view(getattr(torch, name))
    else:
        t = torch.from_numpy(base).cuda()
    if all(s >= 0 for s in strides):
        return torch.as_strided(t, a.shape, strides, off)
    return DevArray.from_torch(t).view(a.shape, strides, off)


def host(t):
    import torch
    name = str(t.dtype).split(".")[-1]
    if name in ("uint16", "uint32", "uint64"):
        return t.view(getattr(torch, name[1:])).cpu().numpy().view(name)
    return t.cpu().numpy()


def _same(got, want, what):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(ru.canon(got), ru.canon(want)), (what, got, want)


def _ex(key, make_plan, **kw):
    hit = _EX.get((key, repr(kw)))
    if hit is None:
        ex = _executor(make_plan(), **kw)
        hit = _EX[(key, repr(kw))] = (ex, ru.Spy(ex))
    return hit


def _seed(*what):
    return zlib.crc32(repr(what).encode())


def _nan_copies(r, places):
    """one copy of the runs per place, with a NaN there in one run (the runs take turns)"""
    for j, pos in enumerate(places):
        r2 = r.copy()
        r2[j % r.shape[0], pos] = np.nan
        yield pos, r2


# ---- runners ------------------------------------------------------------------------------------
def run_axis_form(op, v, form, nan=False):
    dt, acc, out = v
    shape = ru.resolve(form.shape, dt)
    nd = len(shape)
    kept_shape = [shape[d] for d in range(nd) if d not in form.axis]
    nred = int(np.prod([shape[d] for d in form.axis]))
    nkept = int(np.prod(kept_shape))
    ex, spy = _ex(("axis", op, v, nd, form.axis), lambda: ru.reduce_plan(v, nd, form.axis, op))
    geo = None
    cases = [(kind, ru.runs(op, dt, nkept, nred, _seed(op, v, form.name, kind), kind))
             for kind in ru.kinds(op, dt)]
    for kind, r in cases:
        spy.clear()
        (got,) = ex(dev(ru.place(r, shape, form.axis, form.view)))
        if geo is None:
            geo = ru.check_axis_form(form, dt, spy, nred)
        want = ru.ref_runs(op, r, acc, out).reshape(kept_shape)
        _same(got, want, (op, v, form.name, shape, form.axis, kind))
    if nan:
        for pos, r in _nan_copies(cases[-1][1], ru.nan_places(nred, geo[0], geo[1])):
            (got,) = ex(dev(ru.place(r, shape, form.axis, form.view)))
            want = ru.ref_runs(op, r, acc, out).reshape(kept_shape)
            assert np.isnan(want).sum() == 1
            _same(got, want, (op, v, form.name, shape, form.axis, "nan at %d" % pos))


def run_full_form(op, v, form, nan=False):
    dt, acc, out = v
    n = int(np.prod(form.shape))
    nd = len(form.shape)
    ex, spy = _ex(("full", op, v, nd), lambda: ru.reduce_plan(v, nd, None, op))
    checked = False
    cases = [(kind, ru.runs(op, dt, 1, n, _seed(op, v, form.name, kind), kind)) for kind in ru.kinds(op, dt)]
    for kind, r in cases:
        spy.clear()
        (got,) = ex(dev(ru.place(r, form.shape, None, form.view)))
        if not checked:
            ru.check_full_form(form, spy)
            checked = True
        _same(got, ru.ref_runs(op, r, acc, out).reshape(()), (op, v, form.name, form.shape, None, kind))
    if nan:
        for pos, r in _nan_copies(cases[-1][1], ru.nan_places(n, 1, 1)):
            (got,) = ex(dev(ru.place(r, form.shape, None, form.view)))
            assert np.isnan(host(got)), (op, v, form.name, form.shape, None, "nan at %d" % pos)


def run_pair_form(op, v, pform, nan=False):
    dt, acc, out = v
    name, xs, ys, yview, expect = pform
    n = int(np.prod(xs))
    ex, spy = _ex(("pair", op, v), lambda: ru.pair_plan(v, op))
    checked = False
    y = ru.pair_operand(dt, ys, _seed(op, v, name, "y"))
    yd = np.ascontiguousarray(y.T).T if yview == "T" else y
    cases = [(kind, ru.runs(op, dt, 1, n, _seed(op, v, name, kind), kind)) for kind in ru.kinds(op, dt)]
    if nan:
        cases += [("nan at %d" % pos, r) for pos, r in _nan_copies(cases[-1][1], ru.nan_places(n, 1, 1))]
    for kind, r in cases:
        x = ru.split_pair(r.reshape(xs), y)
        spy.clear()
        (got,) = ex(dev(x), dev(yd))
        if not checked:
            ru.check_pair_form(name, expect, spy)
            checked = True
        _same(got, ru.ref_runs(op, r, acc, out).reshape(()), (op, v, name, xs, None, kind))


def run_hgroup(op, v):
    """three independent full reductions of one scalar program and different lengths: one
    ahip_elemwise_reduce_all_multi launch (the largest member has more than 256 partials: two
    waves collect in its finalize)"""
    dt, acc, out = v
    lengths = ru.hgroup_lengths(dt)
    ex, spy = _ex(("towers", op, v), lambda: ru.towers_plan(v, op, len(lengths)))
    for kind in ru.kinds(op, dt):
        rs = [ru.runs(op, dt, 1, n, _seed(op, v, "hgroup", kind, n), kind) for n in lengths]
        spy.clear()
        got = ex(*[dev(r.reshape(-1)) for r in rs])
        assert spy.names() == ["ahip_elemwise_reduce_all_multi"], (op, v, spy.names())
        for g, r, n in zip(got, rs, lengths):
            _same(g, ru.ref_runs(op, r, acc, out).reshape(()), (op, v, "hgroup", (n,), None, kind))


# ---- the matrix ---------------------------------------------------------------------------------
_PAIRS = [(op, v) for op in ru.OPS for v in ru.variants(op)]


@pytest.mark.parametrize("op,v", _PAIRS, ids=["%s-%s" % (op, ru.vid(v)) for op, v in _PAIRS])
def test_every_pair_on_four_forms(op, v):
    for name in ru.EVERY_PAIR:
        run_axis_form(op, v, ru.axis_form(name))
    run_full_form(op, v, next(f for f in ru.full_forms(v[0]) if f.name == ru.FLAT_RAGGED))


_SIX = [(op, v, False) for op, v in ru.SIX] + [("maximum", ("float64",) * 3, True)]
_SIX_IDS = ["%s-%s%s" % (op, ru.vid(v), "-nan" if nan else "") for op, v, nan in _SIX]
_ROW = [f.name for f in ru.AXIS_FORMS if f.name.startswith("row")]
_COL = [f.name for f in ru.AXIS_FORMS if not f.name.startswith("row")]


@pytest.mark.parametrize("op,v,nan", _SIX, ids=_SIX_IDS)
def test_six_pairs_on_row_forms(op, v, nan):
    for name in _ROW:
        run_axis_form(op, v, ru.axis_form(name), nan)


@pytest.mark.parametrize("op,v,nan", _SIX, ids=_SIX_IDS)
def test_six_pairs_on_column_and_mixed_forms(op, v, nan):
    for name in _COL:
        run_axis_form(op, v, ru.axis_form(name), nan)


@pytest.mark.parametrize("op,v,nan", _SIX, ids=_SIX_IDS)
def test_six_pairs_on_single_operand_full_forms(op, v, nan):
    for form in ru.full_forms(v[0]):
        run_full_form(op, v, form, nan)


@pytest.mark.parametrize("op,v,nan", _SIX, ids=_SIX_IDS)
def test_six_pairs_on_fused_full_forms(op, v, nan):
    """loop-invariant and broadcast operands, the LDS-tiled kernel (6, 3 and 258 tiles: the last
    with two collecting waves in the finalize)"""
    for pform in ru.PAIR_FORMS:
        run_pair_form(op, v, pform, nan)


@pytest.mark.parametrize("op,v", ru.SIX, ids=_SIX_IDS[:6])
def test_six_pairs_in_a_horizontal_group(op, v):
    run_hgroup(op, v)


@pytest.mark.parametrize("op", ru.OPS)
def test_empty_input_gives_the_identity_or_raises(op):
    """add -> 0, mul -> 1, and -> all ones / True, or / xor -> 0, mul_without_zeros -> its identity 0;
    maximum / minimum raise ValueError.  Full reduction of (0,) and (0, 5), axis reductions over
    an empty axis."""
    vs = [v for _, v in ru.SIX if v in ru.variants(op)] + [ru.variants(op)[0], ru.variants(op)[-1]]
    for v in vs:
        for shape, axis in (((0,), None), ((0, 5), None), ((0, 5), (0,)), ((3, 0), (1,))):
            nd = len(shape)
            ex, _ = _ex(("empty", op, v, nd, axis), lambda: ru.reduce_plan(v, nd, axis, op))
            x = dev(np.zeros(shape, v[0]))
            if op in ("maximum", "minimum"):
                with pytest.raises(ValueError, match="zero-size array"):
                    ex(x)
                continue
            (got,) = ex(x)
            kept = [s for d, s in enumerate(shape) if axis is not None and d not in axis]
            want = np.full(kept, ru.empty_result(op, v[1], v[2]), v[2])
            _same(got, want, (op, v, "empty", shape, axis))


_REPLAY = [("minimum", ("int8",) * 3), ("and", ("uint16",) * 3), ("mul_without_zeros", ("int32",) * 3),
           ("mul", ("float32", "float64", "float32"))]


@pytest.mark.parametrize("op,v", _REPLAY, ids=["acc%d" % np.dtype(v[1]).itemsize for _, v in _REPLAY])
def test_replayed_sliced_and_multi_partial_reductions(op, v):
    """launch-list replay, three calls with new data: the partial buffer of the sliced form and
    the epoch-tagged granules of the finalize are reused from call to call"""
    dt, acc, out = v
    form = ru.axis_form("row_sliced_ragged")
    shape = ru.resolve(form.shape, dt)
    ex, spy = _ex(("axis", op, v, 2, form.axis), lambda: ru.reduce_plan(v, 2, form.axis, op), use_graph=True)
    for call in range(3):
        r = ru.runs(op, dt, shape[0], shape[1], _seed(op, v, "replay", call))
        (got,) = ex(dev(ru.place(r, shape, form.axis)))
        if call == 0:      # (the first call of a replaying executor launches twice: eager, then recording)
            first = spy.axis_passes()[0]
            assert first["nslices"] == form.expect["nslices"] and first["mode"] == 0, spy.axis_passes()
        _same(got, ru.ref_runs(op, r, acc, out), (op, v, form.name, shape, form.axis, "call %d" % call))
    form = next(f for f in ru.full_forms(dt) if f.name == ru.FLAT_RAGGED)
    ex, spy = _ex(("full", op, v, 1), lambda: ru.reduce_plan(v, 1, None, op), use_graph=True)
    for call in range(3):
        r = ru.runs(op, dt, 1, form.shape[0], _seed(op, v, "replay full", call))
        (got,) = ex(dev(r.reshape(-1)))
        _same(got, ru.ref_runs(op, r, acc, out).reshape(()), (op, v, form.name, form.shape, None, "call %d" % call))
    assert "ahip_elemwise_reduce_all" in spy.names()
