"""``at.convolve`` under ``aesara.function(..., mode="HIP")`` (the reference's front end from the packed overlay,
like tests/test_gpu_expm_function.py): the three modes at ``(TILE_OUT + 1, TAP_CHUNK + 1)`` in float32, a float32 /
float64 pair and int32, against the references and the bar of tests/test_gpu_convolve.py."""
import numpy as np
import pytest

from test_gpu_convolve import MODES, TAP_CHUNK, TILE_OUT, case, check
from test_gpu_expm_function import _np, ae, pytestmark  # noqa: F401  (gpu; skipped where the overlay is not packed)

M, N = TILE_OUT + 1, TAP_CHUNK + 1


@pytest.mark.parametrize("dtypes", [("float32", "float32"), ("float32", "float64"), ("int32", "int32")])
@pytest.mark.parametrize("mode", MODES)
def test_convolve_through_function(ae, mode, dtypes):
    import aesara.tensor as at
    a, v = (at.vector(name, dtype=dt) for name, dt in zip("av", dtypes))
    f = ae.function([a, v], at.convolve(a, v, mode), mode="HIP")
    out = np.promote_types(*dtypes).name
    if out == "int32":
        x, y = (np.random.default_rng(k).integers(-8, 8, k).astype("int32") for k in (M, N))
        got = _np(f(x, y))
        assert got.dtype == np.dtype("int32") and np.array_equal(got, np.convolve(x, y, mode))
    else:
        x, y = case(M, N, mode)[:2]
        got = _np(f(x.astype(dtypes[0]), y.astype(dtypes[1])))
        check(got, M, N, mode, out, "function")
