"""``slinalg.eigvalsh`` and its gradient through the lowering and the executor's host logic (no GPU):
each form lowers to one ``Eigvalsh`` / ``EigvalshGrad`` node with its ``lower``, integer operands are
refused by name, a dry run calls C-ABI entry points only — one tile launch up to 64 rows, one per step
of the tournament above — and the new info codes become SciPy's messages."""
import numpy as np
import pytest

import ref_overlay
from test_gpu_eigvalsh import DTYPES, plan_of

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


def dummy_mode():
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    return Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY)


def dry(plan, *ins):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan, dry_run=True)
    return ex, ex(*ins)


@needs_reference
@pytest.mark.parametrize("lower", [False, True])
def test_each_form_lowers_to_one_node(ae, lower):
    """The test that shows the feature: without the lowering the first compile raises
    ``UnsupportedOp: Eigvalsh has no HIP lowering``."""
    import aesara.tensor as at
    from aesara.tensor.slinalg import eigvalsh
    from aesara.tensor.type_other import NoneConst
    A, B, c = at.matrix("A"), at.matrix("B"), at.vector("c")
    for ins, b in (([A], NoneConst), ([A, B], B)):
        plan = ae.function(ins, eigvalsh(A, b, lower), mode=dummy_mode()).maker.linker.plan
        assert [(n.op, n.params, len(n.inputs)) for n in plan.nodes] == [("Eigvalsh", {"lower": lower}, len(ins))]
    w = eigvalsh(A, B, lower)
    plan = ae.function([A, B, c], ae.grad((w * c).sum(), [A, B]), mode=dummy_mode()).maker.linker.plan
    grads = [n for n in plan.nodes if n.op == "EigvalshGrad"]
    assert len(grads) == 1 and grads[0].params == {"lower": lower}
    assert len(grads[0].inputs) == 3 and len(grads[0].outputs) == 2
    # a float32 / float64 pair goes to the dtype make_node declared, through a cast
    plan = ae.function([A, B], eigvalsh(at.cast(A, "float32"), B, lower), mode=dummy_mode()).maker.linker.plan
    node = next(n for n in plan.nodes if n.op == "Eigvalsh")
    assert [plan.vars[v].dtype for v in node.inputs + node.outputs] == ["float64"] * 3


@needs_reference
def test_integer_operands_are_refused_by_name(ae):
    from aesara.tensor.slinalg import eigvalsh
    from aesara.tensor.type import TensorType
    from aesara.tensor.type_other import NoneConst
    from aesara_amd.lower import UnsupportedOp
    for dt in ("int32", "int64"):
        M = TensorType(dt, shape=(None, None))("M")
        with pytest.raises(UnsupportedOp, match=rf"^Eigvalsh has no HIP lowering for operands of dtypes.*{dt}"):
            ae.function([M], eigvalsh(M, NoneConst), mode=dummy_mode())


@pytest.mark.parametrize("dtype", DTYPES)
def test_dry_runs_touch_only_c_abi_entry_points(dtype):
    from aesara_amd import dist
    assert {"Eigvalsh", "EigvalshGrad"} <= dist._VIEW_REP_ONLY          # replicated under sharding
    ex, (w,) = dry(plan_of(dtype, True), np.zeros((64, 64), dtype))
    assert tuple(w.shape) == (64,) and w.dtype == dtype
    assert all(t.startswith("ahip_") for t in ex.trace) and ex.trace.count("ahip_syev_tile") == 1, ex.trace
    assert not {"ahip_syev_gather", "ahip_syev_apply", "ahip_syev_off"} & set(ex.trace)
    # 130 rows: padded to 192 = 6 blocks, 3 pairs, 5 steps a sweep, columns then rows per step
    ex, (w,) = dry(plan_of(dtype, False), np.zeros((130, 130), dtype))
    assert tuple(w.shape) == (130,) and all(t.startswith("ahip_") for t in ex.trace)
    assert ex.trace.count("ahip_syev_tile") == ex.trace.count("ahip_syev_gather") == 5
    assert ex.trace.count("ahip_syev_apply") == 10 and ex.trace.count("ahip_syev_off") == 2
    # the generalised problem factors b: one diagonal block per 64 rows
    ex, _ = dry(plan_of(dtype, True, True), np.zeros((130, 130), dtype), np.zeros((130, 130), dtype))
    assert ex.trace.count("ahip_potrf_diag") == 3 and all(t.startswith("ahip_") for t in ex.trace)
    with pytest.raises(ValueError, match="shapes of a .* and b .* are incompatible"):
        dry(plan_of(dtype, True, True), np.zeros((3, 3), dtype), np.zeros((4, 4), dtype))
    with pytest.raises(ValueError, match="expected a square matrix"):
        dry(plan_of(dtype, True), np.zeros((3, 4), dtype))


def test_info_words_become_scipys_errors():
    from aesara_amd.exec_linalg import EIG, INFO_TAG, is_linalg_code, linalg_error
    from aesara_amd.exec_sparse import is_sparse_code
    minor = INFO_TAG | (EIG << 32) | (0xFFFFFFFF - 70)
    stall = INFO_TAG | (EIG << 32) | 0xFFFFFFFF
    for code in (minor, stall):
        assert is_linalg_code(code) and not is_sparse_code(code) and code >> 34 == INFO_TAG >> 34
    e = linalg_error(minor, "Eigvalsh")
    assert isinstance(e, np.linalg.LinAlgError)
    assert str(e).startswith("The leading minor of order 70 of B is not positive definite.")
    e = linalg_error(stall, "EigvalshGrad")
    assert isinstance(e, np.linalg.LinAlgError) and str(e) == "Eigenvalues did not converge"
