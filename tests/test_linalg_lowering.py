"""SolveTriangular, CholeskySolve, Solve, MatrixInverse and Det through the rewrite query, the lowering
and the executor's host logic (no GPU): each Op lowers to its plan op with its props, the plans of
linalg_util.op_plan are what the linker lowers, the gradient graphs compile, the rest of the family is
refused by name, a dry run calls C-ABI entry points only, a map-Scan over solves stays a launch list,
and every stored reference output is inside its bars."""
import numpy as np
import pytest

import linalg_util
import ref_overlay
from linalg_util import CASES, NB

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")

LINALG_CALLS = {"ahip_trsm_diag", "ahip_getrf_panel", "ahip_laswp", "ahip_lu_det", "ahip_mirror_triangle",
                "ahip_check_finite"}


@pytest.fixture(scope="module")
def ae():
    return ref_overlay.import_reference()


@pytest.fixture(scope="module")
def gen(ae):
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_linalg_golden
    return gen_linalg_golden


def dummy_mode():
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    return Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY)


def dry(plan, *ins):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan, dry_run=True)
    return ex, ex(*ins)


# ------------------------------------------------------------------ lowering ----------
@needs_reference
def test_each_op_lowers_to_its_plan_op(ae):
    """The test that shows the feature: without the lowering the first compile raises
    ``UnsupportedOp: Solve has no HIP lowering``."""
    import aesara.tensor as at
    from aesara.tensor import nlinalg, slinalg
    A, b, B = at.matrix("A"), at.vector("b"), at.matrix("B")
    built = {
        "Solve": ([A, b], slinalg.solve(A, b, assume_a="sym", lower=True, check_finite=False),
                  {"assume_a": "sym", "lower": True, "check_finite": False}),
        "SolveTriangular": ([A, B], slinalg.solve_triangular(A, B, trans="T", lower=True, unit_diagonal=True),
                            {"lower": True, "trans": 1, "unit_diagonal": True, "check_finite": True}),
        "CholeskySolve": ([A, b], slinalg.cho_solve((A, False), b),
                          {"lower": False, "check_finite": True}),
        "MatrixInverse": ([A], nlinalg.matrix_inverse(A), {}),
        "Det": ([A], nlinalg.det(A), {}),
    }
    for opname, (ins, out, params) in built.items():
        f = ae.function(ins, out, mode=dummy_mode())
        nodes = f.maker.linker.plan.nodes
        assert [n.op for n in nodes] == [opname], [n.op for n in nodes]
        assert nodes[0].params == params
    for trans, want in ((0, 0), (2, 1), ("N", 0), ("C", 1)):
        f = ae.function([A, b], slinalg.solve_triangular(A, b, trans=trans), mode=dummy_mode())
        assert f.maker.linker.plan.nodes[0].params["trans"] == want


@needs_reference
def test_the_tested_plans_are_what_the_linker_lowers(gen):
    bad = [(name, dt) for name in CASES for dt in linalg_util.DTYPES
           if not linalg_util.same_lowering(gen.lower(*gen.op_graph(name, dt), name), linalg_util.op_plan(name, dt))]
    assert not bad, bad
    assert {(c["name"], c["dtype"]) for c in linalg_util.load_cases()} == \
        {(n, dt) for n in CASES for dt in linalg_util.DTYPES}


@needs_reference
def test_mixed_float_operands_go_to_the_declared_dtype_through_a_cast(ae):
    import aesara.tensor as at
    from aesara.tensor import slinalg
    A, b = at.fmatrix("A"), at.dvector("b")
    plan = ae.function([A, b], slinalg.solve(A, b), mode=dummy_mode()).maker.linker.plan
    solve = [n for n in plan.nodes if n.op == "Solve"][0]
    assert [plan.vars[v].dtype for v in solve.inputs] == ["float64", "float64"]
    assert plan.vars[solve.outputs[0]].dtype == "float64" and "Elemwise" in [n.op for n in plan.nodes]


@needs_reference
@pytest.mark.parametrize("what", ["solve", "solve_triangular", "matrix_inverse", "det"])
def test_gradient_graphs_lower_completely_and_dry_run(ae, what):
    import aesara.tensor as at
    from aesara.tensor import nlinalg, slinalg
    A, b, w = at.dmatrix("A"), at.dvector("b"), at.dvector("w")
    n = NB + 1
    if what == "solve":
        cost = (slinalg.solve(A, b) * w).sum()
    elif what == "solve_triangular":
        cost = (slinalg.solve_triangular(A, b, lower=True) * w).sum()
    elif what == "matrix_inverse":
        cost = (nlinalg.matrix_inverse(A) * at.outer(b, w)).sum()
    else:
        cost = nlinalg.det(A) * w.sum() + b.sum()
    f = ae.function([A, b, w], [cost] + ae.grad(cost, [A, b]), mode=dummy_mode(), on_unused_input="ignore")
    plan = f.maker.linker.plan
    ops = {n.op for n in plan.nodes}
    assert ops & set(linalg_util.PLAN_OPS.values()), ops
    ex, res = dry(plan, np.zeros((n, n)), np.zeros(n), np.zeros(n))
    assert tuple(res[1].shape) == (n, n) and tuple(res[2].shape) == (n,)
    assert LINALG_CALLS & set(ex.trace) and all(t.startswith("ahip_") for t in ex.trace)


@needs_reference
def test_the_rest_of_the_family_is_refused_by_name(ae):
    import aesara.tensor as at
    from aesara.tensor import nlinalg, slinalg
    from aesara.tensor.type import TensorType
    from aesara_amd.lower import UnsupportedOp
    A, b = at.matrix("A"), at.vector("b")
    with pytest.raises(UnsupportedOp, match=r"^Eigh has no HIP lowering"):
        ae.function([A], nlinalg.eigh(A), mode=dummy_mode())
    with pytest.raises(UnsupportedOp, match=r"^Cholesky has no HIP lowering"):
        ae.function([A], slinalg.cholesky(A), mode=dummy_mode())
    for dt in ("complex128", "float16", "int32"):
        M, v = TensorType(dt, shape=(None, None))("M"), TensorType(dt, shape=(None,))("v")
        graphs = {"Det": lambda: nlinalg.det(M), "MatrixInverse": lambda: nlinalg.matrix_inverse(M)}
        if dt != "float16":          # (SolveBase.make_node asks SciPy for the result dtype: no float16 there)
            graphs.update({"Solve": lambda: slinalg.solve(M, v),
                           "SolveTriangular": lambda: slinalg.solve_triangular(M, v),
                           "CholeskySolve": lambda: slinalg.cho_solve((M, True), v)})
        # a complex or float16 variable never enters a plan: the lowering of the graph's inputs refuses
        # it, naming the dtype, before any Op is looked at; an integer operand reaches the Op's handler
        want = r"^{op} has no HIP lowering.*int32" if dt == "int32" else \
            rf"^dtype {dt} of \w+ has no HIP kernels"
        for opname, build in graphs.items():
            with pytest.raises(UnsupportedOp, match=want.format(op=opname)):
                ae.function([M, v], build(), mode=dummy_mode(), on_unused_input="ignore")


# ------------------------------------------------------------------ dry runs ----------
@pytest.mark.parametrize("op", sorted(linalg_util.PLAN_OPS))
def test_a_dry_run_at_n_130_touches_only_c_abi_entry_points(op):
    name = {"tri": "tri_n130_l1t1_70", "chol": "chol_n130", "solve": "solve_n130_pos_l1", "inv": "inv_n130",
            "det": "det_n130"}[op]
    for dt in linalg_util.DTYPES:
        xs = [np.zeros(a.shape, dt) for a in linalg_util.operands(name, dt)]
        ex, (out,) = dry(linalg_util.op_plan(name, dt), *xs)
        assert tuple(out.shape) == linalg_util.out_shape(name) and out.dtype == dt
        assert ex.trace and all(t.startswith("ahip_") for t in ex.trace), ex.trace
        own = [t for t in ex.trace if t in LINALG_CALLS]
        blocks = -(-130 // NB)
        if op == "tri":
            assert own.count("ahip_trsm_diag") == blocks and own.count("ahip_check_finite") == 2
            assert ex.trace.count("ahip_gemm") == blocks - 1
        elif op == "chol":
            assert own.count("ahip_trsm_diag") == 2 * blocks
        else:
            assert own.count("ahip_getrf_panel") == blocks
            assert own.count("ahip_mirror_triangle") == (1 if op == "solve" else 0)
            assert own.count("ahip_lu_det") == (1 if op == "det" else 0)


def test_host_errors_are_raised_in_the_offending_call():
    plan = linalg_util.op_plan("solve_n3", "float32")
    with pytest.raises(ValueError, match="expected a square matrix") as ei:
        dry(plan, np.zeros((3, 4), "float32"), np.zeros((3,), "float32"))
    assert "[HIP step" in str(ei.value)
    with pytest.raises(ValueError, match="incompatible"):
        dry(plan, np.zeros((3, 3), "float32"), np.zeros((4,), "float32"))
    with pytest.raises(TypeError, match="does not match float32"):
        dry(plan, np.zeros((3, 3), "float64"), np.zeros((3,), "float32"))


def test_info_words_become_the_errors_of_the_libraries_the_reference_calls():
    from aesara_amd.exec_linalg import INFO_TAG, NONFINITE, SINGULAR, is_linalg_code, linalg_error
    code = INFO_TAG | (SINGULAR << 32) | (0xFFFFFFFF - 4)
    assert is_linalg_code(code) and not is_linalg_code(5) and not is_linalg_code(-3)
    assert not is_linalg_code(2 ** 63 - 1)          # the saturated bad index of a uint64 beyond int64
    e = linalg_error(code, "SolveTriangular")
    assert isinstance(e, np.linalg.LinAlgError) and "resolution failed at diagonal 4" in str(e)
    assert str(linalg_error(code, "MatrixInverse")) == "Singular matrix"
    assert isinstance(linalg_error(code, "Solve"), np.linalg.LinAlgError)
    e = linalg_error(INFO_TAG | (NONFINITE << 32) | 0xFFFFFFFF, "Solve")
    assert isinstance(e, ValueError) and str(e) == "array must not contain infs or NaNs"


@needs_reference
def test_a_map_scan_over_solves_stays_a_launch_list(ae):
    import aesara
    import aesara.tensor as at
    from aesara.tensor import slinalg
    from aesara_amd.executor import PlanExecutor
    As, bs = at.dtensor3("As"), at.dmatrix("bs")
    xs, _ = aesara.map(lambda a, b: slinalg.solve(a, b), [As, bs])
    plan = ae.function([As, bs], xs, mode=dummy_mode()).maker.linker.plan
    assert "Scan" in [n.op for n in plan.nodes]
    ex = PlanExecutor(plan, dry_run=True)
    (out,) = ex(np.zeros((3, 5, 5)), np.zeros((3, 5)))
    assert tuple(out.shape) == (3, 5)
    assert ex.scan_modes and all(m.startswith("launch-list") for m in ex.scan_modes.values()), ex.scan_modes
    # the step plan's executor made the launches: one panel per step
    inner = [e[0] for e in ex._inner.values() if isinstance(e, tuple) and isinstance(e[0], PlanExecutor)]
    assert sum(i.trace.count("ahip_getrf_panel") for i in inner) == 3


# ------------------------------------------------------------------ fixtures ----------
def test_every_stored_reference_output_is_inside_its_bars():
    worst = 0.0
    for c in linalg_util.load_cases():
        name, dt = c["name"], c["dtype"]
        z = np.load(linalg_util.case_file(name, dt))
        out = z["out"]
        assert out.shape == linalg_util.out_shape(name) and out.dtype == np.dtype(dt), (name, dt)
        r = linalg_util.ratios(name, dt, out, z)
        assert all(v <= 1.0 for v in r.values()), (name, dt, r)
        worst = max([worst] + list(r.values()))
        if c["op"] == "det":
            assert 1e-20 < abs(float(z["x64"])) < 1e20
    assert 0.0 < worst <= 1.0
    parity = {c["name"]: c["parity"] for c in linalg_util.load_cases() if c["op"] == "det"}
    assert parity["det_swap1"] == -1 and parity["det_swap2"] == 1
    # the bars catch what a residual alone cannot: the transposed inverse of a symmetric case's result
    z = np.load(linalg_util.case_file("inv_n65", "float32"))
    assert linalg_util.ratios("inv_n65", "float32", z["out"].T, z)["forward"] > 1.0
