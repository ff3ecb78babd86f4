"""``images2neibs`` lowers to one ``Images2Neibs`` node; ``neibs_geometry`` and ``restate`` against the Op's ``perform``."""
import numpy as np
import pytest

from test_eigvalsh_lowering import dummy_mode
from test_expm_lowering import ae, needs_reference  # noqa: F401
from test_gpu_neibs import BAND, MODES, image, plan_of, restate

# (image shape, patch, step, mode, error or None)
ROWS = [((2, 3, 7, 9), (3, 3), (1, 1), "valid", None), ((2, 3, 7, 9), (3, 3), (2, 3), "valid", None),
        ((2, 3, 7, 9), (3, 3), (4, 6), "ignore_borders", None), ((2, 3, 2, 9), (3, 3), (1, 1), "ignore_borders", None),
        ((1, 2, 3, 5), (3, 5), (1, 1), "half", None), ((1, 2, 6, 10), (2, 5), (1, 1), "full", None),
        ((1, 1, 7, 9), (3, 3), (2, 4), "wrap_centered", None), ((1, 2, BAND + 1, 5), (3, 3), (1, 1), "full", None),
        ((1, 2, 7, 11), (2, 5), (2, 5), "ignore_borders", None),
        ((2, 3, 7, 9), (3, 3), (0, 1), "valid", (ValueError, "neib_step wrong step ; values <= ")),
        ((2, 3, 7, 9), (3, -1), (1, 1), "full", (ValueError, "neib_shape values <=")),
        ((2, 3, 7, 9), (2, 3), (1, 1), "wrap_centered", (TypeError, "Images2Neibs:")),
        ((2, 3, 7, 9), (9, 9), (1, 1), "wrap_centered", (TypeError, "Images2Neibs:")),
        ((2, 3, 7, 9), (3, 3), (3, 3), "valid", (TypeError, r"neib_shape\[")), ((2, 3, 7, 9), (3, 3), (1, 3), "half", (TypeError, r"neib_shape\[")),
        ((2, 3, 2, 9), (3, 3), (1, 1), "full", (TypeError, r"neib_shape\["))]


@needs_reference
@pytest.mark.parametrize("mode", MODES)
def test_images2neibs_lowers_to_one_node(ae, mode):
    """Without the lowering the compile raises ``UnsupportedOp: Images2Neibs has no HIP lowering``."""
    import aesara.tensor as at
    from aesara.tensor.nnet.neighbours import images2neibs
    x, (shp, stp) = at.tensor4("x", dtype="int16"), (at.TensorType("int64", shape=(2,))(k) for k in ("shp", "stp"))
    for ins, out in (([x], images2neibs(x, (3, 3), (1, 1), mode=mode)), ([x, shp, stp], images2neibs(x, shp, stp, mode=mode))):
        plan = ae.function(ins, out, mode=dummy_mode()).maker.linker.plan
        assert [(n.op, n.params) for n in plan.nodes] == [("Images2Neibs", {"mode": mode})]
        assert plan.vars[plan.outputs[0]].dtype == "int16" and len(plan.nodes[0].inputs) == 3


@needs_reference
@pytest.mark.parametrize("shape,patch,step,mode,error", ROWS)
def test_geometry_and_restatement_against_perform(ae, shape, patch, step, mode, error):
    from aesara.tensor.nnet.neighbours import Images2Neibs
    from aesara_amd.exec_neibs import neibs_geometry
    op, x = Images2Neibs(mode), image(shape, "float32")
    node = op.make_node(x, np.asarray(patch), np.asarray(step))
    cell = [None]
    perform = lambda: op.perform(node, [x, np.asarray(patch), np.asarray(step)], [cell], mode)  # noqa: E731
    if error is None:
        perform()
        g = neibs_geometry(shape, patch, step, mode)
        assert g.out_shape == cell[0].shape == (shape[0] * shape[1] * g.grid[0] * g.grid[1], patch[0] * patch[1])
        np.testing.assert_array_equal(restate(x, patch, step, mode), cell[0])
        return
    for call in (perform, lambda: neibs_geometry(shape, patch, step, mode)):
        with pytest.raises(error[0], match="^" + error[1]):
            call()
