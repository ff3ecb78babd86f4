"""``slinalg.expm`` and its gradient through the lowering and the executor's host logic (no GPU): each lowers
to one ``Expm`` / ``ExpmGrad`` node without parameters, integer operands are refused by name, a dry run calls
C-ABI entry points only — one ``ahip_expm_tile`` up to 64 rows in float32 and 48 in float64, the blocked
path's launches above — and an empty operand launches nothing."""
import numpy as np
import pytest

import ref_overlay
from test_eigvalsh_lowering import dry, dummy_mode
from test_gpu_expm import DTYPES, plan_of

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
def test_expm_and_its_gradient_lower_to_one_node_each(ae, dtype):
    """The test that shows the feature: without the lowering the compile raises ``UnsupportedOp: Expm has no
    HIP lowering``."""
    import aesara.tensor as at
    from aesara.tensor.slinalg import expm
    A = at.matrix("A", dtype=dtype)
    plan = ae.function([A], expm(A), mode=dummy_mode()).maker.linker.plan
    assert [(n.op, n.params) for n in plan.nodes] == [("Expm", {})]
    assert [plan.vars[v].dtype for v in plan.nodes[0].inputs + plan.nodes[0].outputs] == [dtype] * 2
    plan = ae.function([A], ae.grad(expm(A).sum(), A), mode=dummy_mode()).maker.linker.plan
    grads = [n for n in plan.nodes if n.op == "ExpmGrad"]
    assert len(grads) == 1 and grads[0].params == {} and not [n for n in plan.nodes if n.op == "Expm"]
    assert [plan.vars[v].dtype for v in grads[0].inputs + grads[0].outputs] == [dtype] * 3


@needs_reference
def test_integer_operands_are_refused_by_name(ae):
    from aesara.tensor.slinalg import expm
    from aesara.tensor.type import TensorType
    from aesara_amd.lower import UnsupportedOp
    M = TensorType("int32", shape=(None, None))("M")
    with pytest.raises(UnsupportedOp, match=r"^Expm has no HIP lowering.*int32"):
        ae.function([M], expm(M), mode=dummy_mode())


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dry_runs_touch_only_c_abi_entry_points(dtype, grad):
    """The last size of the tile path and the first of the blocked one: 64 | 65 rows in float32, 48 | 49 in
    float64; the gradient runs on twice its operand's rows."""
    from aesara_amd import dist
    assert {"Expm", "ExpmGrad"} <= dist._VIEW_REP_ONLY                      # replicated under sharding
    limit = {"float32": 64, "float64": 48}[dtype] // (2 if grad else 1)
    for n, tiled in ((limit, True), (limit + 1, False)):
        ex, (out,) = dry(plan_of(dtype, grad), *[np.zeros((n, n), dtype)] * (2 if grad else 1))
        assert tuple(out.shape) == (n, n) and out.dtype == dtype
        assert all(t.startswith("ahip_") for t in ex.trace), ex.trace
        assert ex.trace.count("ahip_expm_tile") == int(tiled) and ("ahip_expm_norm1" in ex.trace) == (not tiled)
        assert ("ahip_getrf_panel" in ex.trace) == ("ahip_gemm" in ex.trace) == (not tiled)


@pytest.mark.parametrize("grad", [False, True])
def test_an_empty_operand_launches_nothing(grad):
    ex, (out,) = dry(plan_of("float32", grad), *[np.zeros((0, 0), "float32")] * (2 if grad else 1))
    assert tuple(out.shape) == (0, 0) and ex.trace == []


def test_a_non_square_operand_is_refused_in_scipys_words():
    with pytest.raises(np.linalg.LinAlgError, match="Last 2 dimensions of the array must be square"):
        dry(plan_of("float32"), np.zeros((3, 2), "float32"))
