"""``nlinalg.pinv``, ``aesara.grad`` through it and ``matrix_power`` with a negative exponent under
``aesara.function(..., mode="HIP")``: the reference's front end (from the packed overlay, like
tests/test_gpu_eigvalsh_function.py) over the real PlanExecutor, against NumPy float64.

The forward bar is the one of tests/test_gpu_pinv.py.  The gradient is checked against central differences
of NumPy's ``pinv`` with step 1e-6: truncation ``h^2`` and rounding ``eps / h`` are both below 1e-9, the
tolerance is 1e-6 of the gradient's norm.  ``matrix_power(M, -2) = P P`` with ``P = pinv(M)``: an error
``d`` of ``P`` gives ``2 ||P||_2 d`` to first order, plus ``n eps ||P||_F^2`` for the product.  Skipped
where the overlay is not packed."""
import numpy as np
import pytest

import ref_overlay
from test_gpu_pinv import DTYPES, bar, graded

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


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 3), (70, 130)])
def test_pinv(ae, shape, dtype):
    import aesara.tensor as at
    from aesara.tensor import nlinalg
    A = at.matrix("A", dtype=dtype)
    f = ae.function([A], nlinalg.pinv(A), mode="HIP")
    M = graded(*shape, dtype)
    got = _np(f(M.astype(dtype)))
    err, cap = np.linalg.norm(got.astype("float64") - np.linalg.pinv(M)), bar(M, dtype)
    print(f"{shape} {dtype}: {err / cap:.2e} of the bar {cap:.3e}")
    assert got.dtype == np.dtype(dtype) and got.shape == shape[::-1] and err <= cap


def test_gradient_against_central_differences(ae):
    import aesara.tensor as at
    from aesara.tensor import nlinalg
    A = at.matrix("A", dtype="float64")
    f = ae.function([A], ae.grad(nlinalg.pinv(A)[0].sum(), A), mode="HIP")
    M, h = graded(5, 3, "float64"), 1e-6
    want = np.zeros_like(M)
    for i, j in np.ndindex(*M.shape):
        E = np.zeros_like(M)
        E[i, j] = h
        want[i, j] = (np.linalg.pinv(M + E)[0].sum() - np.linalg.pinv(M - E)[0].sum()) / (2 * h)
    err = np.linalg.norm(_np(f(M)) - want) / np.linalg.norm(want)
    print(f"gradient: relative error {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES)
def test_matrix_power_with_a_negative_exponent(ae, dtype):
    import aesara.tensor as at
    from aesara.tensor import nlinalg
    A = at.matrix("A", dtype=dtype)
    f = ae.function([A], nlinalg.matrix_power(A, -2), mode="HIP")
    M = graded(4, 4, dtype)
    P = np.linalg.pinv(M)
    cap = 2 * np.linalg.norm(P, 2) * bar(M, dtype) + 4 * float(np.finfo(dtype).eps) * np.linalg.norm(P) ** 2
    err = np.linalg.norm(_np(f(M.astype(dtype))).astype("float64") - np.linalg.matrix_power(M, -2))
    print(f"matrix_power {dtype}: {err / cap:.2e} of the bar {cap:.3e}")
    assert err <= cap
