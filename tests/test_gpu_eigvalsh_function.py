"""``slinalg.eigvalsh`` and ``aesara.grad`` through it under ``aesara.function(..., mode="HIP")``: the
reference's front end (from the packed overlay, like tests/test_gpu_linalg_function.py) over the real
PlanExecutor, against NumPy float64.  ``A = Q diag(1 ... n) Q^T`` and ``B = Q' diag(1 ... 10) Q'^T``.

The eigenvalue bar is the one of tests/test_gpu_eigvalsh.py.  The gradient bar is Davis-Kahan's:
``||d gA||_F <= 4 kappa(B) sum_i |gw_i| bar_w / gap_i`` (``gap_i``: the distance from ``w_i`` to its
nearest neighbour), and the same with ``|gw_i w_i|`` for ``gB``.  The Op folds a gradient into the named
triangle (``g_ij + g_ji``); the test unfolds it, ``(F + F^T) / 2``, and wants exact zeros in the other
triangle.  Skipped where the overlay is not packed."""
import numpy as np
import pytest

import ref_overlay
from test_gpu_eigvalsh import DTYPES, KAPPA_B, bar, reference, spd

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_overlay.available(),
                                 reason="no reference front end (oracle/_ref overlay not packed)")]


@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    import aesara_amd
    aesara_amd.get_mode()            # registers linker "hip" / mode "HIP" with the reference
    return ae


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def unit_gaps(n, dtype):
    Q = np.linalg.qr(np.random.default_rng(n).standard_normal((n, n)))[0]
    M = (Q * np.arange(1.0, n + 1)) @ Q.T
    M = ((M + M.T) / 2).astype(dtype).astype("float64")
    return np.tril(M) + np.tril(M, -1).T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lower", [False, True])
@pytest.mark.parametrize("n", [3, 65])
def test_generalised_eigenvalues_and_their_gradients(ae, n, lower, dtype):
    import aesara.tensor as at
    from aesara.tensor.slinalg import eigvalsh
    A, B, c = at.matrix("A", dtype=dtype), at.matrix("B", dtype=dtype), at.vector("c", dtype=dtype)
    w = eigvalsh(A, B, lower)
    f = ae.function([A, B, c], [w] + ae.grad((w * c).sum(), [A, B]), mode="HIP")
    ops = [nd.op for nd in f.maker.linker.plan.nodes]
    assert ops.count("Eigvalsh") == 1 and ops.count("EigvalshGrad") == 1, ops
    M, Bm = unit_gaps(n, dtype), spd(n, dtype)
    cv = np.random.default_rng(n + 1).standard_normal(n).astype(dtype)
    L = np.linalg.cholesky(Bm)
    C = np.linalg.solve(L, np.linalg.solve(L, M).T).T
    w64, Y = np.linalg.eigh((C + C.T) / 2)
    V = np.linalg.solve(L.T, Y)
    c64 = cv.astype("float64")
    want = [(V * c64) @ V.T, -(V * (c64 * w64)) @ V.T]
    bar_w = bar(M, dtype, KAPPA_B)
    gaps = np.array([np.min(np.abs(np.delete(w64, i) - w64[i])) for i in range(n)])
    caps = [4 * KAPPA_B * np.sum(np.abs(g) * bar_w / gaps) for g in (c64, c64 * w64)]
    other = np.triu(np.ones((n, n), bool), 1) if lower else np.tril(np.ones((n, n), bool), -1)
    first = None
    for call in range(3):
        got = [_np(g) for g in f(M.astype(dtype), Bm.astype(dtype), cv)]
        assert all(g.dtype == np.dtype(dtype) for g in got)
        err = np.max(np.abs(got[0] - reference(M, Bm)))
        print(f"n={n} lower={lower} {dtype} call {call}: w at {err / bar_w:.2e} of its bar")
        assert err <= bar_w
        for name, F, G, cap in zip(("gA", "gB"), got[1:], want, caps):
            F = F.astype("float64")
            e = np.linalg.norm((F + F.T) / 2 - G)
            print(f"  {name}: {e:.3e}, {e / cap:.2e} of the bar {cap:.3e}")
            assert e <= cap and not np.any(F[other])
        first = first or got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_standard_problem(ae, dtype):
    import aesara.tensor as at
    from aesara.tensor.slinalg import eigvalsh
    from aesara.tensor.type_other import NoneConst
    A = at.matrix("A", dtype=dtype)
    f = ae.function([A], eigvalsh(A, NoneConst), mode="HIP")
    assert [nd.op for nd in f.maker.linker.plan.nodes] == ["Eigvalsh"]
    M = unit_gaps(33, dtype)
    assert np.max(np.abs(_np(f(M.astype(dtype))) - reference(M))) <= bar(M, dtype)


def test_the_pinned_refusals_still_hold(ae):
    import aesara.tensor as at
    from aesara.tensor import nlinalg, slinalg
    from aesara_amd.lower import UnsupportedOp
    A = at.matrix("A")
    for out, name in ((nlinalg.eigh(A)[0], "Eigh"), (slinalg.cholesky(A), "Cholesky")):
        with pytest.raises(UnsupportedOp, match=rf"^{name} has no HIP lowering"):
            ae.function([A], out, mode="HIP")
