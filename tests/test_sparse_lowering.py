"""Sparse values through the rewrite query, the lowering, the boundary and the executor's host logic
(no GPU): every sparse Op lowers to its plan op, the relabelling Ops add no node, the boundary field
lists the right positions, the plans of sparse_util.op_plan are what the linker lowers, the rest of
the family is refused by name, a dry run calls C-ABI entry points only, ``DeviceSparse`` round-trips,
and every stored reference output is inside its bar."""
import numpy as np
import pytest
import scipy.sparse

import ref_overlay
import sparse_util
from sparse_util import CASES

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")

SPARSE_CALLS = {"ahip_csr_spmm", "ahip_csr_sddmm", "ahip_csr_to_dense", "ahip_csr_mul_dense",
                "ahip_dense_count_rows", "ahip_dense_fill_csr", "ahip_csr_flip_finish"}


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
    import gen_sparse_golden
    return gen_sparse_golden


def dummy_mode(executor=None, **kw):
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    return Mode(HipLinker(executor_factory=executor or (lambda plan: (lambda *a: None)), **kw), HIP_QUERY)


def lowered(ae, ins, outs, **kw):
    return ae.function(ins, outs, mode=dummy_mode(), on_unused_input="ignore", **kw).maker.linker.plan


def dry(plan, *ins):
    from aesara_amd.executor import PlanExecutor
    ex = PlanExecutor(plan, dry_run=True)
    return ex, ex(*ins)


# ------------------------------------------------------------------ lowering ----------
@needs_reference
def test_each_op_lowers_to_its_plan_op(ae):
    """The test that shows the feature: without the lowering the first compile raises
    ``UnsupportedOp: non-tensor variable type Sparse (SparseTensorType{...})``."""
    import aesara.sparse as sp
    import aesara.tensor as at
    from aesara.sparse import basic as S
    x, xc = sp.csr_matrix("x", "float64"), sp.csc_matrix("xc", "float64")
    w, v, g = at.dmatrix("w"), at.dvector("v"), at.dmatrix("g")
    built = {
        "structured_dot csr": ([x, w], sp.structured_dot(x, w), ["StructuredDot"]),
        "structured_dot csc": ([xc, w], sp.structured_dot(xc, w), ["StructuredDot"]),
        "dot sparse matrix": ([x, w], sp.dot(x, w), ["SparseDot"]),
        "dot sparse vector": ([xc, v], sp.dot(xc, v), ["SparseDot"]),
        "dot dense sparse": ([x, w], sp.dot(w.T, x), ["DimShuffle", "SparseDot"]),
        "sdg csr": ([x, w, g], S.sdg_csr(sp.csm_indices(x), sp.csm_indptr(x), w, g), ["SampledDot"]),
        "sdg csc": ([xc, w, g], S.sdg_csc(sp.csm_indices(xc), sp.csm_indptr(xc), w, g), ["SampledDot"]),
        "dense_from_sparse": ([xc], sp.dense_from_sparse(xc), ["DenseFromSparse"]),
        "csr_from_dense": ([w], sp.csr_from_dense(w), ["SparseFromDense", "Shape_i", "Shape_i"]),
        "csc_from_dense": ([w], sp.csc_from_dense(w), ["SparseFromDense", "Shape_i", "Shape_i"]),
        "sp_sum": ([x], sp.sp_sum(x), ["CAReduce"]),
        "sp_sum 0": ([x], sp.sp_sum(x, axis=0), ["SpSum"]),
        "sp_sum 1": ([xc], sp.sp_sum(xc, axis=1), ["SpSum"]),
        "mul_s_d": ([x, w], S.mul_s_d(x, w), ["MulSD"]),
        "neg": ([x], -x, ["Elemwise"]),
        "structured_sigmoid": ([x], sp.structured_sigmoid(x), ["Elemwise"]),
    }
    for what, (ins, out, ops) in built.items():
        plan = lowered(ae, ins, out)
        assert [n.op for n in plan.nodes] == ops, (what, [n.op for n in plan.nodes])
    p = lowered(ae, [xc, w], sp.structured_dot(xc, w)).nodes[0].params
    assert p == {"format": "csc", "sparse_first": True, "name": "xc"}
    p = lowered(ae, [x, w], sp.dot(w.T, x)).nodes[-1].params
    assert p == {"format": "csr", "sparse_first": False, "name": "x"}
    assert lowered(ae, [x], sp.sp_sum(x, axis=0)).nodes[0].params == {"format": "csr", "axis": 0, "name": "x"}


@needs_reference
def test_relabelling_ops_add_no_node(ae):
    import aesara.sparse as sp
    x = sp.csr_matrix("x", "float32")
    d, i, p, shp = sp.csm_properties(x)
    plan = lowered(ae, [x], [d * 2, i + 1, p + 1])
    assert {n.op for n in plan.nodes} <= {"Elemwise", "DimShuffle"}   # (CSMProperties itself is no node)
    assert set(plan.inputs[:3]) <= {v for n in plan.nodes for v in n.inputs}
    plan = lowered(ae, [x], sp.CSR(d, i, p, shp))
    assert [n.op for n in plan.nodes] == ["DeepCopyOp"] * 3          # (an output that is an input is copied)
    plan = lowered(ae, [x], sp.structured_dot(x.T, sp.dense_from_sparse(x)))
    assert [n.op for n in plan.nodes] == ["DenseFromSparse", "StructuredDot"]
    dot = plan.nodes[1]
    assert dot.params["format"] == "csc" and dot.inputs[:3] == plan.inputs[:3]
    assert dot.inputs[3:5] == [plan.inputs[4], plan.inputs[3]]        # the extents, swapped
    plan = lowered(ae, [x], [x.shape[0], x.shape[1]])
    assert plan.nodes == [] and plan.outputs == plan.inputs[3:5]
    assert [n.op for n in lowered(ae, [x], x.shape).nodes] == ["MakeVector"]


@needs_reference
def test_gradient_graphs_lower_completely(ae):
    import aesara.sparse as sp
    import aesara.tensor as at
    for fmt, ctor in (("csr", sp.csr_matrix), ("csc", sp.csc_matrix)):
        x, w = ctor("x", "float32"), at.fmatrix("w")
        y = sp.structured_dot(x, w)
        plan = lowered(ae, [x, w], [y] + ae.grad(y.sum(), [x, w]))
        ops = [n.op for n in plan.nodes]
        assert ops.count("StructuredDot") == 2 and ops.count("SampledDot") == 1, ops
        assert plan.sparse == {"inputs": [[0, fmt, 0]], "outputs": [[1, fmt, 1]]}
        gw = ae.grad(sp.dot(x, w).sum(), w)
        assert "StructuredDot" in [n.op for n in lowered(ae, [x, w], gw).nodes]
        gx = ae.grad((sp.dense_from_sparse(x) ** 2).sum(), x)
        ops = [n.op for n in lowered(ae, [x], gx).nodes]
        assert "MulSD" in ops and "DenseFromSparse" in ops, ops


@needs_reference
def test_the_boundary_field_lists_the_right_positions(ae):
    import aesara.sparse as sp
    import aesara.tensor as at
    from aesara_amd.plan import Plan
    a, x, b, xc = at.dmatrix("a"), sp.csr_matrix("x", "float64"), at.dvector("b"), sp.csc_matrix("xc", "float64")
    plan = lowered(ae, [a, x, b, xc], [sp.dot(x, b), -xc, a.sum(), x.T])
    assert plan.sparse == {"inputs": [[1, "csr", 1], [3, "csc", 7]], "outputs": [[1, "csc", 1], [3, "csc", 7]]}
    assert len(plan.inputs) == 12 and len(plan.outputs) == 12
    members = plan.inputs[1:6]
    assert [plan.vars[v].dtype for v in members] == ["float64", "int32", "int32", "int64", "int64"]
    assert [len(plan.vars[v].shape) for v in members] == [1, 1, 1, 0, 0]
    again = Plan.loads(plan.dumps())
    assert again.sparse == plan.sparse and again.dumps() == plan.dumps()
    # a graph without sparse values serialises as before: no such key
    dense = lowered(ae, [a, b], at.dot(a, b))
    assert dense.sparse is None and "sparse" not in dense.to_json()


@needs_reference
def test_a_sparse_constant_becomes_plan_constants(ae):
    import aesara.sparse as sp
    import aesara.tensor as at
    m = scipy.sparse.csr_matrix(np.array([[0, 2.0, 0], [1.0, 0, 3.0]]))
    w = at.dmatrix("w")
    plan = lowered(ae, [w], sp.structured_dot(sp.as_sparse_variable(m), w))
    node = [n for n in plan.nodes if n.op == "StructuredDot"][0]
    consts = [plan.vars[v].const_value() for v in node.inputs[:5]]
    assert np.array_equal(consts[0], m.data) and np.array_equal(consts[1], m.indices)
    assert np.array_equal(consts[2], m.indptr) and [int(c) for c in consts[3:]] == [2, 3]
    assert plan.sparse is None


@needs_reference
def test_the_tested_plans_are_what_the_linker_lowers(gen):
    bad = [(name, dt) for name in CASES for dt in sparse_util.case_dtypes(name)
           if not sparse_util.same_lowering(gen.lower(*gen.op_graph(name, dt), name), sparse_util.op_plan(name, dt))]
    assert not bad, bad
    assert {(c["name"], c["dtype"]) for c in sparse_util.load_cases()} == \
        {(n, dt) for n in CASES for dt in sparse_util.case_dtypes(n)}


@needs_reference
def test_mixed_float_operands_go_to_the_declared_dtype_through_a_cast(ae):
    import aesara.sparse as sp
    import aesara.tensor as at
    x, w = sp.csr_matrix("x", "float32"), at.dmatrix("w")
    plan = lowered(ae, [x, w], sp.structured_dot(x, w))
    assert [n.op for n in plan.nodes] == ["Elemwise", "StructuredDot"]
    dot = plan.nodes[1]
    assert plan.vars[dot.inputs[0]].dtype == "float64" and plan.vars[dot.outputs[0]].dtype == "float64"


@needs_reference
def test_the_rest_of_the_family_is_refused_by_name(ae):
    import aesara.sparse as sp
    import aesara.tensor as at
    from aesara.sparse import basic as S
    from aesara.sparse.type import SparseTensorType
    from aesara_amd.lower import UnsupportedOp
    x, y = sp.csr_matrix("x", "float64"), sp.csc_matrix("y", "float64")
    w, v = at.dmatrix("w"), at.dvector("v")
    two = {"StructuredDot": lambda: sp.structured_dot(x, y), "Dot": lambda: S._dot(x, y)}
    for opname, build in two.items():
        with pytest.raises(UnsupportedOp, match=rf"^{opname} has no HIP lowering for two sparse operands"):
            lowered(ae, [x, y], build())
    refused = {
        "AddSS": lambda: S.add_s_s(x, x), "MulSS": lambda: S.mul_s_s(x, x), "AddSD(_ccode)?": lambda: S.add_s_d(x, w),
        "MulSV": lambda: S.mul_s_v(x, v), "StructuredAddSV": lambda: S.structured_add_s_v(x, v),
        "ColScaleCSC": lambda: S.col_scale(y, v), "RowScaleCSC": lambda: S.row_scale(y, v),
        "Usmm": lambda: S.usmm(at.constant(2.0), x, w, w), "HStack": lambda: S.hstack([x, x]),
        "VStack": lambda: S.vstack([x, x]), "GetItem2d": lambda: x[0:1, 0:1], "GetItemScalar": lambda: x[0, 0],
        "Remove0": lambda: S.remove0(x), "EnsureSortedIndices": lambda: S.ensure_sorted_indices(x),
        "Diag": lambda: S.diag(x), "SquareDiagonal": lambda: S.square_diagonal(v),
        "Cast": lambda: S.cast(x, "float32"), "TrueDot": lambda: S.true_dot(x, y),
        "SamplingDot": lambda: S.sampling_dot(w, w, x), "LessThanSS": lambda: S.lt(x, x),
    }
    for opname, build in refused.items():
        with pytest.raises(UnsupportedOp, match=rf"^{opname} has no HIP lowering"):
            lowered(ae, [x, y, w, v], build())
    for fmt, dt in (("bsr", "float64"), ("csr", "int32"), ("csc", "complex128")):        # (no float16 SparseTensorType)
        bad = SparseTensorType(fmt, dt)("b")
        with pytest.raises(UnsupportedOp, match=rf"has no HIP lowering for a sparse value of format {fmt} and dtype {dt}"):
            lowered(ae, [bad, w], S._structured_dot(bad, w))
    # a sparse value where a dense tensor is expected (an Op with a dense handler only)
    with pytest.raises(UnsupportedOp, match="non-tensor variable type Sparse"):
        import aesara
        vs = at.dmatrix("vs")
        out, _ = aesara.map(lambda row: sp.dot(x, row), [vs])
        lowered(ae, [x, vs], out)


# ------------------------------------------------------------------ dry runs ----------
@pytest.mark.parametrize("name,calls", [
    ("sdot_lens_csr_n65", ["ahip_csr_spmm"]),
    ("sdot_lens_csc_n65", ["ahip_sort_rows", "ahip_csr_flip_finish", "ahip_csr_spmm"]),
    ("dotr_r130_csr_n65", ["ahip_sort_rows", "ahip_csr_flip_finish", "ahip_csr_spmm"]),
    ("dotr_r130_csc_n65", ["ahip_csr_spmm"]),
    ("sdg_lens_csc_n65", ["ahip_csr_sddmm"]),
    ("dfs_lens_csr", ["ahip_fill", "ahip_csr_to_dense"]),
    ("sum_lens_csr_a1", ["ahip_csr_spmm"]),
    ("sum_lens_csr_a0", ["ahip_sort_rows", "ahip_csr_flip_finish", "ahip_csr_spmm"]),
    ("mul_lens_csc", ["ahip_csr_mul_dense"]),
    ("sfd_lens_csr", ["ahip_fill", "ahip_dense_count_rows", "ahip_cumulative", "ahip_dense_fill_csr"]),
])
def test_a_dry_run_touches_only_the_expected_entry_points(name, calls):
    for dt in sparse_util.DTYPES:
        xs = sparse_util.operands(name, dt)
        ex, res = dry(sparse_util.op_plan(name, dt), *xs)
        assert ex.trace == calls, ex.trace
        if CASES[name]["op"] != "sfd":
            z = np.load(sparse_util.case_file(name, dt))
            assert tuple(res[0].shape) == z["out"].shape and res[0].dtype == dt


def test_a_long_index_list_takes_the_large_sort():
    from aesara_amd import _lib
    n = int(_lib.lib.ahip_sort_max_row(_lib.DTYPE_CODES["int32"])) + 1
    xs = [np.zeros(n, "float32"), np.zeros(n, "int32"), np.array([0, n], "int32"), np.asarray(1, "int64"),
          np.asarray(3, "int64")]
    ex, (out,) = dry(sparse_util.op_plan("sum_lens_csr_a0", "float32"), *xs)
    assert ex.trace == ["ahip_sort_rows_large", "ahip_csr_flip_finish", "ahip_csr_spmm"] and tuple(out.shape) == (3,)


def test_host_errors_are_raised_in_the_offending_call():
    plan = sparse_util.op_plan("sdot_r65_csr_n2", "float32")
    xs = sparse_util.operands("sdot_r65_csr_n2", "float32")
    with pytest.raises(ValueError, match="shape mismatch in StructuredDot.perform") as ei:
        dry(plan, *(xs[:5] + [np.zeros((41, 2), "float32")]))
    assert ei.value.args[1] == ((65, 40), (41, 2)) and "[HIP step" in str(ei.value)
    with pytest.raises(ValueError, match="do not make a csr matrix of shape"):
        dry(plan, *([xs[0], xs[1], xs[2][:-1]] + xs[3:]))
    with pytest.raises(TypeError, match="input dtype int64 does not match int32"):
        dry(plan, *([xs[0], xs[1].astype("int64"), xs[2]] + xs[3:]))
    with pytest.raises(ValueError, match="dimension mismatch"):
        dry(sparse_util.op_plan("dot_r65_csr_vec", "float32"), *(xs[:5] + [np.zeros(39, "float32")]))


def test_info_words_become_value_errors_naming_the_operand():
    from aesara_amd.exec_linalg import is_linalg_code
    from aesara_amd.exec_sparse import BAD_INDEX, BAD_INDPTR, INFO_TAG, MALFORMED, is_sparse_code, sparse_error
    code = INFO_TAG | (MALFORMED << 32) | BAD_INDEX
    assert is_sparse_code(code) and not is_linalg_code(code)
    assert not is_sparse_code(5) and not is_sparse_code(-3) and not is_sparse_code(2 ** 63 - 1)
    assert not is_sparse_code(INFO_TAG | (2 << 32) | 7)              # a singular matrix of the dense solves
    e = sparse_error(code, "StructuredDot", "x")
    assert isinstance(e, ValueError) and str(e).startswith("StructuredDot: malformed sparse operand x: an index")
    assert "indptr" in str(sparse_error(INFO_TAG | (MALFORMED << 32) | BAD_INDPTR, "SpSum", "x"))


def test_the_new_plan_ops_are_replicated_when_a_plan_is_sharded():
    from aesara_amd import dist
    from aesara_amd.exec_sparse import SPARSE_OPS
    assert set(SPARSE_OPS) <= dist._VIEW_REP_ONLY


# ------------------------------------------------------------------ boundary ----------
def test_device_sparse_round_trips_and_checks_its_members():
    import torch
    from aesara_amd.sparse import DeviceSparse, check_argument, expand_args, split_scipy
    for fmt in ("csr", "csc"):
        m = scipy.sparse.random(7, 5, 0.4, format=fmt, dtype="float32", random_state=3)
        d = DeviceSparse.from_scipy(m, device="cpu")
        assert d.format == fmt and d.shape == (7, 5) and d.dtype == "float32" and d.nnz == m.nnz
        back = d.to_scipy()
        assert back.format == fmt and back.dtype == m.dtype and (back != m).nnz == 0
        assert np.array_equal(back.indices, m.indices) and np.array_equal(back.indptr, m.indptr)
        assert check_argument(d, fmt, "float32") is d and check_argument(m, fmt, "float32") is m
        other = "csc" if fmt == "csr" else "csr"
        with pytest.raises(TypeError, match=f"a {fmt} matrix with float32 data where the graph has {other}"):
            check_argument(d, other, "float32")
        with pytest.raises(TypeError, match="where the graph has"):
            check_argument(d, fmt, "float64")
        # the members handed to the executor are the matrix's own arrays, call after call
        a, b = expand_args([1, m], [[1, fmt, 1]]), expand_args([1, m], [[1, fmt, 1]])
        assert len(a) == 6 and all(x is y for x, y in zip(a[1:4], b[1:4])) and [int(x) for x in a[4:]] == [7, 5]
        with pytest.raises(TypeError, match=f"a {fmt} matrix where the graph has {other}"):
            expand_args([m], [[0, other, 0]])
    big = scipy.sparse.csr_matrix(np.eye(3))
    big.indices, big.indptr = big.indices.astype("int64"), big.indptr.astype("int64")
    with pytest.raises(TypeError, match="64-bit index arrays are not supported"):
        split_scipy(big)
    with pytest.raises(TypeError, match="64-bit"):
        DeviceSparse("csr", torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), (3, 3))
    with pytest.raises(TypeError, match="float32 / float64 only"):
        DeviceSparse("csr", torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                     torch.zeros(4, dtype=torch.int32), (3, 3))
    with pytest.raises(TypeError, match="format 'bsr'"):
        DeviceSparse("bsr", torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), (3, 3))
    with pytest.raises(ValueError, match="do not make a csr matrix"):
        DeviceSparse("csr", torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), (3, 3))


@needs_reference
def test_the_cell_filter_takes_a_device_sparse_and_rejects_a_wrong_one(ae):
    import aesara.sparse as sp
    from aesara_amd.devcell import DeviceFilterType
    from aesara_amd.sparse import DeviceSparse
    t = DeviceFilterType(sp.csr_matrix("x", "float32").type)
    m = scipy.sparse.random(4, 6, 0.5, format="csr", dtype="float32", random_state=1)
    d = DeviceSparse.from_scipy(m, device="cpu")
    assert t.filter(d) is d and t.filter(m, strict=True) is m
    with pytest.raises(TypeError, match="where the graph has csr / float32"):
        t.filter(DeviceSparse.from_scipy(m.tocsc(), device="cpu"))
    with pytest.raises(TypeError, match="where the graph has csr / float32"):
        t.filter(DeviceSparse.from_scipy(m.astype("float64"), device="cpu"))
    with pytest.raises(TypeError):
        t.filter(m.tocsc(), strict=True)


@needs_reference
def test_the_linker_splits_arguments_and_joins_results(ae):
    """A stand-in executor that computes with SciPy sees the members and hands members back."""
    import aesara.sparse as sp
    import aesara.tensor as at
    from aesara_amd.sparse import DeviceSparse
    seen = []

    def factory(plan):
        def run(data, indices, indptr, rows, cols, w):
            seen.append((data, indices, indptr))
            m = scipy.sparse.csr_matrix((data, indices, indptr), shape=(int(rows), int(cols)))
            return [m @ w, -data, indices, indptr, cols, rows]
        return run
    x, w = sp.csr_matrix("x", "float64"), at.dmatrix("w")
    m = scipy.sparse.random(6, 4, 0.5, format="csr", dtype="float64", random_state=2)
    W = np.arange(8.0).reshape(4, 2)
    for return_numpy in (False, True):
        f = ae.function([x, w], [sp.dot(x, w), (-x).T], mode=dummy_mode(factory, return_numpy=return_numpy))
        assert f.maker.linker.plan.sparse == {"inputs": [[0, "csr", 0]], "outputs": [[1, "csc", 1]]}
        y, xt = f(m, W)
        assert np.allclose(y, m @ W)
        if return_numpy:
            assert scipy.sparse.issparse(xt) and xt.format == "csc"
        else:
            assert isinstance(xt, DeviceSparse) and xt.format == "csc"
            xt = xt.to_scipy()
        assert xt.shape == (4, 6) and abs(xt + m.T).sum() == 0
        y2, _ = f(DeviceSparse.from_scipy(m, device="cpu"), W)
        assert np.allclose(y2, m @ W)
    assert seen[0][0] is m.data and seen[0][1] is m.indices and seen[0][2] is m.indptr
    big = m.copy()
    big.indices = big.indices.astype("int64")
    with pytest.raises(TypeError, match="64-bit index arrays are not supported"):
        f(big, W)


# ------------------------------------------------------------------ fixtures ----------
def test_every_stored_reference_output_is_inside_its_bar():
    worst = 0.0
    for c in sparse_util.load_cases():
        name, dt = c["name"], c["dtype"]
        z = np.load(sparse_util.case_file(name, dt))
        xs = sparse_util.load_inputs(z)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(xs, sparse_util.operands(name, dt))), name
        r = sparse_util.ratio(name, dt, z["out"], xs, z)
        assert r <= 1.0, (name, dt, r)
        worst = max(worst, r)
    assert 0.0 < worst <= 1.0
    # the bars catch a wrong summand: one entry of a row left out of a float32 product
    name = "sdot_lens_csr_n3"
    z = np.load(sparse_util.case_file(name, "float32"))
    xs = sparse_util.load_inputs(z)
    wrong = z["out"].copy()
    k = int(xs[2][7]) - 1                                   # the last entry of the 257-entry row
    wrong[6] -= xs[0][k] * xs[5][xs[1][k]]
    assert sparse_util.ratio(name, "float32", wrong, xs, z) > 1.0
