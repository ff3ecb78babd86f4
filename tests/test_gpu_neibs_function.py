"""``images2neibs`` / ``neibs2images`` and their gradient under ``aesara.function(..., mode="HIP")``; exact."""
import numpy as np
import pytest

from test_gpu_expm_function import _np, ae, pytestmark  # noqa: F401  (gpu; skipped where the overlay is not packed)
from test_gpu_neibs import image, restate


def test_symbolic_shape_and_step_follow_their_values(ae):
    import aesara.tensor as at
    from aesara.tensor.nnet.neighbours import images2neibs
    x, (shp, stp) = at.tensor4("x", dtype="float32"), (at.TensorType("int64", shape=(2,))(k) for k in ("shp", "stp"))
    f = ae.function([x, shp, stp], images2neibs(x, shp, stp, mode="valid"), mode="HIP")
    v = image((2, 3, 7, 9), "float32")
    for patch, step in (((3, 3), (2, 3)), ((1, 3), (3, 2)), ((3, 3), (2, 3))):
        np.testing.assert_array_equal(_np(f(v, np.asarray(patch), np.asarray(step))), restate(v, patch, step, "valid"))


@pytest.mark.parametrize("mode", ["valid", "ignore_borders"])
def test_neibs2images_inverts_images2neibs(ae, mode):
    import aesara.tensor as at
    from aesara.tensor.nnet.neighbours import images2neibs, neibs2images
    x = at.tensor4("x", dtype="float32")
    v = image((2, 3, 8, 10) if mode == "valid" else (2, 3, 7, 9), "float32")
    f = ae.function([x], neibs2images(images2neibs(x, (2, 2), mode=mode), (2, 2), x.shape, mode=mode), mode="HIP")
    want = v.copy()
    want[:, :, v.shape[2] // 2 * 2:], want[:, :, :, v.shape[3] // 2 * 2:] = 0, 0
    np.testing.assert_array_equal(_np(f(v)), want)


@pytest.mark.parametrize("step", [None, (1, 1)])
def test_gradient(ae, step):
    import aesara.tensor as at
    from aesara.tensor.nnet.neighbours import images2neibs
    x, w = at.tensor4("x", dtype="float32"), at.matrix("w", dtype="float32")
    f = ae.function([x, w], ae.grad((images2neibs(x, (2, 2), step) * w).sum(), x), mode="HIP")
    shape = (2, 3, 6, 8)                    # disjoint patches go through neibs2images, overlapping ones through a Scan
    index = np.arange(np.prod(shape), dtype="float32").reshape(shape)
    where = restate(index, (2, 2), step or (2, 2), "valid").astype("int64")
    wv = image(where.shape, "float32")
    want = np.bincount(where.ravel(), wv.ravel(), np.prod(shape)).reshape(shape).astype("float32")
    np.testing.assert_array_equal(_np(f(image(shape, "float32"), wv)), want)
