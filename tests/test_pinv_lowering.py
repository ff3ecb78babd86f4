"""``nlinalg.pinv`` through the lowering and the executor's host logic (no GPU): each form lowers to one
``MatrixPinv`` node with its ``hermitian``, its gradient lowers onto Ops that already had handlers, integer
operands are refused by name, a dry run calls C-ABI entry points only — one tile launch up to 64 columns,
the launches of one sweep above — and the info words become NumPy's message."""
import numpy as np
import pytest

import ref_overlay
from test_eigvalsh_lowering import dry, dummy_mode
from test_gpu_pinv import DTYPES, plan_of

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hermitian", [False, True])
def test_each_form_lowers_to_one_node(ae, hermitian, dtype):
    """The test that shows the feature: without the lowering the compile raises ``UnsupportedOp: MatrixPinv
    has no HIP lowering``."""
    import aesara.tensor as at
    from aesara.tensor import nlinalg
    A = at.matrix("A", dtype=dtype)
    plan = ae.function([A], nlinalg.pinv(A, hermitian=hermitian), mode=dummy_mode()).maker.linker.plan
    assert [(n.op, n.params) for n in plan.nodes] == [("MatrixPinv", {"hermitian": hermitian})]
    assert [plan.vars[v].dtype for v in plan.nodes[0].inputs + plan.nodes[0].outputs] == [dtype] * 2


@needs_reference
def test_the_gradient_lowers_onto_ops_that_had_handlers(ae):
    import aesara.tensor as at
    from aesara.tensor import nlinalg
    from aesara_amd.executor import PlanExecutor
    A = at.matrix("A")
    plan = ae.function([A], ae.grad(nlinalg.pinv(A).sum(), A), mode=dummy_mode()).maker.linker.plan
    ops = [n.op for n in plan.nodes]
    assert ops.count("MatrixPinv") == 1 and all(hasattr(PlanExecutor, f"_op_{op}") for op in ops), ops
    M = at.matrix("M")
    plan = ae.function([M], nlinalg.matrix_power(M, -2), mode=dummy_mode()).maker.linker.plan
    assert [n.op for n in plan.nodes].count("MatrixPinv") == 1


@needs_reference
def test_integer_operands_are_refused_by_name(ae):
    from aesara.tensor import nlinalg
    from aesara.tensor.type import TensorType
    from aesara_amd.lower import UnsupportedOp
    M = TensorType("int32", shape=(None, None))("M")
    with pytest.raises(UnsupportedOp, match=r"^MatrixPinv has no HIP lowering.*int32"):
        ae.function([M], nlinalg.pinv(M), mode=dummy_mode())


@pytest.mark.parametrize("dtype", DTYPES)
def test_dry_runs_touch_only_c_abi_entry_points(dtype):
    from aesara_amd import dist
    assert "MatrixPinv" in dist._VIEW_REP_ONLY                              # replicated under sharding
    ex, (p,) = dry(plan_of(dtype), np.zeros((3, 2), dtype))
    assert tuple(p.shape) == (2, 3) and p.dtype == dtype
    assert all(t.startswith("ahip_") for t in ex.trace) and ex.trace.count("ahip_gesvj_tile") == 1, ex.trace
    assert not {"ahip_gesvj_gram", "ahip_geqr2_panel", "ahip_syev_apply"} & set(ex.trace)
    # 70 columns of the transposed view: padded to 128 = 4 blocks, 2 pairs, 3 steps a sweep, A and V per step
    ex, (p,) = dry(plan_of(dtype), np.zeros((70, 130), dtype))
    assert tuple(p.shape) == (130, 70) and all(t.startswith("ahip_") for t in ex.trace)
    assert ex.trace.count("ahip_gesvj_gram") == ex.trace.count("ahip_gesvj_gram_tile") == 3
    assert ex.trace.count("ahip_syev_apply") == 6 and ex.trace.count("ahip_gesvj_done") == 1
    # a tall operand of at most 64 columns goes through the QR, a hermitian one through the eigen-solver
    ex, _ = dry(plan_of(dtype), np.zeros((200, 40), dtype))
    assert ex.trace.count("ahip_geqr2_panel") == 1 and ex.trace.count("ahip_gesvj_tile") == 1
    ex, _ = dry(plan_of(dtype, True), np.zeros((6, 6), dtype))
    assert ex.trace.count("ahip_syev_tile") == 1 and "ahip_gesvj_tile" not in ex.trace


@pytest.mark.parametrize("shape", [(0, 3), (3, 0), (0, 0)])
def test_an_empty_operand_launches_nothing(shape):
    ex, (p,) = dry(plan_of("float32"), np.zeros(shape, "float32"))
    assert tuple(p.shape) == shape[::-1] and ex.trace == []


def test_info_words_become_numpys_error():
    from aesara_amd.exec_linalg import EIG, INFO_TAG, NONFINITE, is_linalg_code, linalg_error
    for code in (INFO_TAG | (EIG << 32) | 0xFFFFFFFF, INFO_TAG | (NONFINITE << 32) | 0xFFFFFFFF):
        e = linalg_error(code, "MatrixPinv")
        assert is_linalg_code(code) and isinstance(e, np.linalg.LinAlgError) and str(e) == "SVD did not converge"
