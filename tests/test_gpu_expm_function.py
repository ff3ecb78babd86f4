"""``slinalg.expm`` and ``aesara.grad`` through it under ``aesara.function(..., mode="HIP")``: the reference's
front end (from the packed overlay, like tests/test_gpu_pinv_function.py) over the real PlanExecutor, against
SciPy in float64.  One function returns ``expm(A)`` and the gradient of ``(expm(A) * W).sum()``, which is
``ExpmGrad(A, W)``: at n = 5 both take the one-launch path, at n = 33 the gradient's 66 x 66 block matrix takes
the blocked one.  References, yardsticks and the bar are those of tests/test_gpu_expm.py.  Skipped where the
overlay is not packed."""
import numpy as np
import pytest

import ref_overlay
from test_gpu_expm import DTYPES, check, gaussian, reference

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
@pytest.mark.parametrize("n", [5, 33])
def test_expm_and_its_gradient(ae, n, dtype):
    import aesara.tensor as at
    from aesara.tensor.slinalg import expm
    A, W = at.matrix("A", dtype=dtype), at.matrix("W", dtype=dtype)
    f = ae.function([A, W], [expm(A), ae.grad((expm(A) * W).sum(), A)], mode="HIP")
    M, G = gaussian(n, 2), gaussian(n, 1.0, seed=1)
    E, dA = (_np(v) for v in f(M.astype(dtype), G.astype(dtype)))
    assert E.dtype == dA.dtype == np.dtype(dtype) and E.shape == dA.shape == (n, n)
    check(E, *reference(M), dtype, f"function expm n={n}")
    check(dA, *reference(M, G), dtype, f"function grad n={n}")
