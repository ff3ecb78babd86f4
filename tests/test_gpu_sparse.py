"""The sparse kernels on the device: every case of tests/sparse_util.CASES through PlanExecutor on its
committed plan, with NumPy only (no front end).  Each case is recorded once and replayed twice; the
three calls must agree bit for bit, and every result is held to the bars of sparse_util.py against
the stored reference outputs of tests/golden/sparse.  Malformed operands raise ``ValueError`` — also
from a replayed launch list — and the next call on good operands passes."""
import numpy as np
import pytest

import sparse_util
from sparse_util import CASES

pytestmark = pytest.mark.gpu

ALL = [(n, dt) for n in CASES for dt in sparse_util.case_dtypes(n)]
WORST = {}


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _executor(name, dtype):
    from aesara_amd.executor import PlanExecutor
    return PlanExecutor(sparse_util.op_plan(name, dtype), use_graph=True)


@pytest.mark.parametrize("name,dtype", ALL, ids=[f"{n}-{dt}" for n, dt in ALL])
def test_case_three_calls_same_bits_inside_the_bar(name, dtype):
    z = np.load(sparse_util.case_file(name, dtype))
    xs = sparse_util.load_inputs(z)
    ex = _executor(name, dtype)
    calls = [[_np(o) for o in ex(*xs)] for _ in range(3)]
    for later in calls[1:]:
        assert len(later) == len(calls[0])
        for a, b in zip(calls[0], later):
            assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    got = calls[0][0]
    assert got.shape == z["out"].shape and got.dtype == z["out"].dtype, (got.shape, got.dtype)
    if "out_indices" in z.files:        # a sparse result: the pattern is exact
        indices, indptr, rows, cols = calls[0][1:5]
        assert indices.dtype == np.int32 and indptr.dtype == np.int32
        assert np.array_equal(indices, z["out_indices"]) and np.array_equal(indptr, z["out_indptr"])
        assert (int(rows), int(cols)) == tuple(z["out_shape"])
    r = sparse_util.ratio(name, dtype, got, xs, z)
    WORST[name, dtype] = r
    print(f"{name} {dtype}: {r:.4f} of the bar" + (" (exact)" if sparse_util.exact_case(name) else ""))
    assert r <= 1.0, (name, dtype, r)
    if CASES[name]["op"] != "sfd":      # (SparseFromDense reads its output length on the host: never replayed)
        assert not ex._no_replay


def test_worst_case_is_reported():
    if WORST:
        (name, dtype), r = max(WORST.items(), key=lambda kv: kv[1])
        print(f"worst case: {name} {dtype} at {r:.4f} of its bar ({len(WORST)} cases)")
        assert r <= 1.0


# ------------------------------------------------------------------ malformed operands -
def _break(xs, how, minor):
    data, indices, indptr = xs[0], xs[1].copy(), xs[2].copy()
    if how == "index_at_extent":
        indices[len(indices) // 2] = minor
    elif how == "negative_index":
        indices[0] = -1
    elif how == "decreasing_indptr":
        k = int(np.argmax(np.diff(indptr))) + 1         # the end of the longest row, pulled below its start
        indptr[k] = indptr[k - 1] - 1 if indptr[k - 1] > 0 else indptr[k + 1] + 1
    elif how == "last_indptr_beyond_nnz":
        indptr[-1] = len(indices) + 3
    return [data, indices, indptr] + list(xs[3:])


MALFORMED = ("index_at_extent", "negative_index", "decreasing_indptr", "last_indptr_beyond_nnz")
# one case per kernel that walks a sparse operand, with and without the flip
GUARDED = ("sdot_r65_csr_n2", "sdot_r65_csc_n64", "sdot_lens_csr_n65", "dotr_r65_csr_n3", "sdg_lens_csr_n3",
           "sdg_lens_csc_n65", "dfs_lens_csr", "sum_lens_csc_a0", "mul_lens_csr")


@pytest.mark.parametrize("name", GUARDED)
def test_malformed_operands_raise_and_the_next_call_passes(name):
    dtype = "float32"
    z = np.load(sparse_util.case_file(name, dtype))
    xs = sparse_util.load_inputs(z)
    c = CASES[name]
    _i, _p, _major, minor = sparse_util.pattern(c["pattern"])
    ex = _executor(name, dtype)
    good = _np(ex(*xs)[0])
    for how in MALFORMED:
        for _ in range(2):              # the second time through the recorded launch list
            with pytest.raises(ValueError, match="malformed sparse operand x"):
                ex(*_break(xs, how, minor))
        again = _np(ex(*xs)[0])
        assert again.tobytes() == good.tobytes(), (name, how)
    assert sparse_util.ratio(name, dtype, good, xs, z) <= 1.0
