"""Sparse graphs under ``aesara.function(..., mode="HIP")``: the reference's front end (from the packed
overlay, like tests/test_gpu_linalg_function.py) over the real PlanExecutor.  ``structured_dot`` and
``sparse.dot`` with their gradients, a logistic-regression step on a csr and a csc design matrix held
on the device, the dense -> sparse -> dense round trip, sparse outputs in both forms, a sparse shared
variable, and a malformed argument.  Skipped where the overlay is not packed.

Bars: as in tests/sparse_util.py — a sum of k terms is held to (k + 2) eps sum |a| |b| per element
against the float64 evaluation in NumPy / SciPy (float64: twice the bar, both sides round)."""
import numpy as np
import pytest
import scipy.sparse

import ref_overlay

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_overlay.available(),
                                 reason="no reference front end (oracle/_ref overlay not packed)")]

DTYPES = ("float32", "float64")
FORMATS = ("csr", "csc")


@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    import aesara_amd
    aesara_amd.get_mode()            # registers linker "hip" / mode "HIP" with the reference
    return ae


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _eps(dtype):
    return float(np.finfo(dtype).eps) * (1.0 if dtype == "float32" else 2.0)


def _design(fmt, dtype, rows=70, cols=45, seed=0):
    """A design matrix with an empty row and an empty column, rows of up to 45 entries."""
    rng = np.random.default_rng(seed)
    dense = rng.standard_normal((rows, cols)) * (rng.random((rows, cols)) < 0.3)
    dense[3, :] = 0.0
    dense[:, 5] = 0.0
    dense[7, :] = rng.standard_normal(cols)
    dense[7, 5] = 0.0
    return scipy.sparse.csr_matrix(dense.astype(dtype)).asformat(fmt)


def _held(got, exact, absum, k, dtype, what):
    bar = (k + 2) * _eps(dtype) * absum
    err = np.abs(_np(got).astype("float64") - exact)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    worst = float(r.max()) if r.size else 0.0
    print(f"{what} {dtype}: {worst:.4f} of the bar")
    assert worst <= 1.0, (what, dtype, worst)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_structured_dot_and_sparse_dot_with_their_gradients(ae, fmt, dtype):
    import aesara.sparse as sp
    import aesara.tensor as at
    from aesara.tensor.type import TensorType
    from aesara_amd.sparse import DeviceSparse
    x = (sp.csr_matrix if fmt == "csr" else sp.csc_matrix)("x", dtype)
    w, v = TensorType(dtype, (None, None))("w"), TensorType(dtype, (None, None))("v")
    y = sp.structured_dot(x, w)
    y2 = sp.dot(x, w)
    gx, gw = ae.grad((y * v).sum(), [x, w])
    gw2 = ae.grad((y2 * v).sum(), w)
    f = ae.function([x, w, v], [y, y2, gx, gw, gw2], mode="HIP")
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert "StructuredDot" in ops and "SparseDot" in ops and "SampledDot" in ops, ops
    X = _design(fmt, dtype)
    rng = np.random.default_rng(1)
    W, V = rng.standard_normal((45, 6)).astype(dtype), rng.standard_normal((70, 6)).astype(dtype)
    X64, W64, V64 = X.astype("float64"), W.astype("float64"), V.astype("float64")
    A = abs(X64)
    per_row, per_col = int(X.getnnz(axis=1).max()), int(X.getnnz(axis=0).max())
    coo = X.asformat(fmt)
    major_of = np.repeat(np.arange(len(coo.indptr) - 1), np.diff(coo.indptr))
    r, c = (major_of, coo.indices) if fmt == "csr" else (coo.indices, major_of)
    first = None
    for call in range(3):                # the second and third calls replay the recorded launch list
        res = f(X, W, V)
        gxs = res[2]
        assert isinstance(gxs, DeviceSparse) and gxs.format == fmt and gxs.shape == X.shape
        assert np.array_equal(_np(gxs.indices), X.indices) and np.array_equal(_np(gxs.indptr), X.indptr)
        bits = [_np(res[0]), _np(res[1]), _np(gxs.data), _np(res[3]), _np(res[4])]
        if first is None:
            first = bits
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, bits)), call
    _held(first[0], np.asarray(X64 @ W64), np.asarray(A @ np.abs(W64)), per_row, dtype, f"structured_dot {fmt}")
    _held(first[1], np.asarray(X64 @ W64), np.asarray(A @ np.abs(W64)), per_row, dtype, f"sparse.dot {fmt}")
    _held(first[2], np.sum(V64[r] * W64[c], axis=1), np.sum(np.abs(V64[r] * W64[c]), axis=1), 6, dtype,
          f"structured gradient {fmt}")
    for k in (3, 4):
        _held(first[k], np.asarray(X64.T @ V64), np.asarray(A.T @ np.abs(V64)), per_col, dtype,
              f"gradient of the dense operand {fmt}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_logistic_regression_step_on_a_device_resident_design_matrix(ae, fmt, dtype):
    """w <- w - lr X^T (sigmoid(X w) - y) / m with ``w`` (n x 1) a device shared variable updated in
    place and ONE ``DeviceSparse`` passed to three calls.  Every step is judged on its own, from the
    weights the device held before it: z = X w carries (k + 2) eps |X||w| (k: the longest row); the
    sigmoid is 1/4-Lipschitz and the residual's chain-rule form (factors below 20 for |z| < 3, products
    below 1) adds at most 32 eps; the gradient is a sum of c terms (the longest column) over m, so
    dw <= lr (|X|^T dr + (c + 3) eps |X|^T |r|) / m + 2 eps |w|."""
    import aesara.sparse as sp
    import aesara.tensor as at
    from aesara.tensor.type import TensorType
    from aesara_amd.sharedvar import hip_shared
    from aesara_amd.sparse import DeviceSparse
    X = _design(fmt, dtype)
    m, n = X.shape
    rng = np.random.default_rng(2)
    w0 = (0.1 * rng.standard_normal((n, 1))).astype(dtype)
    yv = (rng.random((m, 1)) < 0.5).astype(dtype)
    lr = 0.5
    x = (sp.csr_matrix if fmt == "csr" else sp.csc_matrix)("x", dtype)
    y = TensorType(dtype, (None, None))("y")
    w = hip_shared(w0, "w")
    p = at.sigmoid(sp.structured_dot(x, w))
    loss = -(y * at.log(p) + (1 - y) * at.log(1 - p)).mean()
    gw = ae.grad(loss, w)
    f = ae.function([x, y], loss, updates=[(w, w - np.asarray(lr, dtype) * gw)], mode="HIP")
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert ops.count("StructuredDot") >= 2, ops
    Xd = DeviceSparse.from_scipy(X, device="cuda")
    X64, A, y64 = X.astype("float64"), abs(X.astype("float64")), yv.astype("float64")
    k, c = int(X.getnnz(axis=1).max()), int(X.getnnz(axis=0).max())
    eps = _eps(dtype)
    for step in range(3):
        before = _np(w.get_value()).astype("float64")
        got_loss = float(_np(f(Xd, yv)))
        after = _np(w.get_value())
        assert after.dtype == np.dtype(dtype) and after.shape == (n, 1)
        z = X64 @ before
        assert np.abs(z).max() < 3.0
        pr = 1.0 / (1.0 + np.exp(-z))
        r = pr - y64
        want = before - lr * (X64.T @ r) / m
        dz = (k + 2) * eps * (A @ np.abs(before))
        dr = dz / 4 + 32 * eps
        bar = lr * (A.T @ dr + (c + 3) * eps * (A.T @ np.abs(r))) / m + 2 * eps * np.abs(want)
        err = np.abs(after.astype("float64") - want)
        worst = float((err / bar).max())
        print(f"logistic step {step} {fmt} {dtype}: {worst:.4f} of the bar")
        assert worst <= 1.0, (fmt, dtype, step, worst)
        want_loss = float(-(y64 * np.log(pr) + (1 - y64) * np.log(1 - pr)).mean())
        assert abs(got_loss - want_loss) <= (k + 40) * eps * max(1.0, abs(want_loss))


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_to_sparse_to_dense_round_trip(ae, fmt):
    import aesara.sparse as sp
    import aesara.tensor as at
    w = at.dmatrix("w")
    # (the negation in between keeps the rewrites from cancelling the two conversions)
    f = ae.function([w], sp.dense_from_sparse(-(sp.csr_from_dense if fmt == "csr" else sp.csc_from_dense)(w)),
                    mode="HIP")
    assert [n.op for n in f.maker.linker.plan.nodes if n.op.startswith(("Sparse", "Dense"))] == \
        ["SparseFromDense", "DenseFromSparse"]
    W = _design("csr", "float64", rows=67, cols=131, seed=4).toarray()
    for _ in range(3):
        got = _np(f(W))
        assert got.dtype == W.dtype and np.array_equal(got, -W)
    assert _np(f(np.zeros((3, 0)))).shape == (3, 0)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_sparse_output_as_device_sparse_and_as_scipy(ae, fmt):
    import aesara.sparse as sp
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    from aesara_amd.sparse import DeviceSparse
    x = (sp.csr_matrix if fmt == "csr" else sp.csc_matrix)("x", "float32")
    X = _design(fmt, "float32")
    other = "csc" if fmt == "csr" else "csr"
    out = sp.structured_sigmoid(-x).T
    f = ae.function([x], out, mode="HIP")
    want = X.copy()
    want.data = (1.0 / (1.0 + np.exp(want.data.astype("float64")))).astype("float32")
    for arg in (X, DeviceSparse.from_scipy(X, device="cuda")):
        got = f(arg)
        assert isinstance(got, DeviceSparse) and got.format == other and got.shape == X.shape[::-1]
        assert got.data.is_cuda and got.indices.is_cuda
        back = got.to_scipy()
        assert back.format == other and abs(back - want.T).max() <= 4 * np.finfo("float32").eps
    g = ae.function([x], out, mode=Mode(HipLinker(return_numpy=True), HIP_QUERY))
    got = g(X)
    assert scipy.sparse.issparse(got) and got.format == other and got.dtype == np.float32
    assert got.shape == X.shape[::-1] and abs(got - want.T).max() <= 4 * np.finfo("float32").eps


def test_an_update_of_a_sparse_shared_variable_goes_back_as_scipy(ae):
    import aesara.sparse as sp
    X = _design("csr", "float64")
    s = ae.shared(X.copy(), name="s")
    f = ae.function([], sp.sp_sum(s, axis=1), updates=[(s, -s)], mode="HIP")
    sums = _np(f())
    held = s.get_value()
    assert scipy.sparse.issparse(held) and held.format == "csr" and abs(held + X).max() == 0
    assert np.allclose(sums, np.asarray(X.sum(axis=1)).ravel(), rtol=0, atol=1e-12)
    assert np.allclose(_np(f()), -sums, rtol=0, atol=1e-12)


def test_a_malformed_argument_raises_through_the_function(ae):
    import aesara.sparse as sp
    import aesara.tensor as at
    x, w = sp.csr_matrix("x", "float64"), at.dmatrix("w")
    f = ae.function([x, w], sp.structured_dot(x, w), mode="HIP")
    X = _design("csr", "float64")
    W = np.ones((45, 2))
    good = _np(f(X, W))
    bad = X.copy()
    bad.indices[10] = 45
    with pytest.raises(ValueError, match="malformed sparse operand x"):
        f(bad, W)
    assert _np(f(X, W)).tobytes() == good.tobytes()
    wide = X.copy()
    wide.indices = wide.indices.astype("int64")
    with pytest.raises(TypeError, match="64-bit index arrays are not supported"):
        f(wide, W)
