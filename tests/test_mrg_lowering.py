"""``MRG_RandomStream`` through the rewrite query, the lowering and the executor's host logic (no GPU):
``uniform`` / ``binomial`` / ``normal`` / ``multinomial`` / ``choice`` lower to the one-node plans of
tests/mrg_util.py plus Ops that already have kernels, float16 samples and ``replace=True`` are refused
by name, the host power routine reproduces the reference's jump matrices, the jump table for one step
per piece is one step, and a dry run raises the host errors and calls C-ABI entry points only."""
import numpy as np
import pytest

import mrg_util
import ref_overlay

needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="reference Aesara not present (GPU box)")
GOLDEN = mrg_util.load_mrg_golden()


@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    mrg_util.python_dot_modulo()
    return ae


def lower(ae, ins, outs):
    from aesara.compile.mode import Mode
    from aesara_amd.linker import HIP_QUERY, HipLinker
    mode = Mode(HipLinker(executor_factory=lambda plan: (lambda *a: None)), HIP_QUERY)
    # (the stream's ``default_update`` makes the new state an output of the plan next to the sample)
    return ae.function(ins, outs, mode=mode, on_unused_input="ignore").maker.linker.plan


def _stream(ae):
    from aesara.sandbox.rng_mrg import MRG_RandomStream
    return MRG_RandomStream(234)


def _ops(plan):
    return [n.op for n in plan.nodes]


# ------------------------------------------------------------------ lowering ----------
@needs_reference
@pytest.mark.parametrize("dtype", mrg_util.DTYPES)
def test_uniform_lowers_to_the_committed_plan(ae, dtype):
    srng = _stream(ae)
    plan = lower(ae, [], srng.uniform((7, 33), dtype=dtype, nstreams=20))
    assert _ops(plan).count("MrgUniform") == 1
    assert mrg_util.same_lowering(plan, mrg_util.uniform_plan(2, dtype, (7, 33))), plan.pretty()
    node = next(n for n in plan.nodes if n.op == "MrgUniform")
    # the default update: the new state is an output of the plan next to the sample
    assert node.outputs[0] in plan.outputs and node.inputs[0] in plan.inputs
    assert plan.vars[node.inputs[1]].const_value().tolist() == [7, 33]


@needs_reference
def test_uniform_with_bounds_and_a_symbolic_size(ae):
    import aesara.tensor as at
    srng = _stream(ae)
    x = at.matrix("x", dtype="float32")
    plan = lower(ae, [x], srng.uniform(x.shape, low=-1.0, high=3.0, dtype="float32", nstreams=20))
    assert mrg_util.same_lowering(plan, mrg_util.uniform_plan(2, "float32", None)), plan.pretty()
    assert set(_ops(plan)) <= {"MrgUniform", "Elemwise", "Shape", "Shape_i", "MakeVector", "DimShuffle"}, _ops(plan)


@needs_reference
def test_binomial_and_normal_are_graphs_over_uniform(ae):
    import aesara.tensor as at
    srng = _stream(ae)
    x = at.matrix("x", dtype="float32")
    plan = lower(ae, [x], srng.binomial(size=x.shape, p=0.5, dtype="float32", nstreams=12) * x)
    assert _ops(plan).count("MrgUniform") == 1
    assert mrg_util.same_lowering(plan, mrg_util.uniform_plan(2, "float64", None)), plan.pretty()
    for dtype in mrg_util.DTYPES:
        plan = lower(ae, [], srng.normal((1001,), dtype=dtype, nstreams=30))
        assert _ops(plan).count("MrgUniform") == 1
        assert mrg_util.same_lowering(plan, mrg_util.uniform_plan(1, dtype, (1002,))), plan.pretty()


@needs_reference
@pytest.mark.parametrize("dtype", mrg_util.DTYPES)
def test_multinomial_and_choice_lower_to_the_committed_plans(ae, dtype):
    import aesara.tensor as at
    srng = _stream(ae)
    p = at.matrix("p", dtype=dtype)
    plan = lower(ae, [p], srng.multinomial(pvals=p, nstreams=9))
    assert _ops(plan).count("MrgUniform") == 1 and _ops(plan).count("MultinomialFromUniform") == 1
    assert mrg_util.same_lowering(plan, mrg_util.op_plan("MultinomialFromUniform", dtype, "float64", "int64", n=1))
    plan = lower(ae, [p], srng.choice(size=2, replace=False, p=p, nstreams=9))
    assert _ops(plan).count("MrgUniform") == 1 and _ops(plan).count("ChoiceFromUniform") == 1
    assert mrg_util.same_lowering(plan, mrg_util.op_plan("ChoiceFromUniform", dtype, "float64", "int64", n=2))


@needs_reference
def test_float16_samples_and_replacement_are_refused_by_name(ae):
    import aesara.tensor as at
    from aesara.sandbox.multinomial import ChoiceFromUniform
    from aesara_amd.lower import UnsupportedOp
    srng = _stream(ae)
    with pytest.raises(UnsupportedOp, match=r"^mrg_uniform has no HIP lowering.*float16"):
        lower(ae, [], srng.uniform((4,), dtype="float16", nstreams=2))
    p, u = at.matrix("p", dtype="float32"), at.vector("u", dtype="float32")
    with pytest.raises(UnsupportedOp, match=r"^ChoiceFromUniform has no HIP lowering.*replace=True"):
        lower(ae, [p, u], ChoiceFromUniform("int64", replace=True)(p, u, 2))


# ------------------------------------------------------------------ jump-ahead --------
def test_the_power_routine_reproduces_the_stored_matrices():
    from aesara_amd.exec_rng import A1, A2, M1, M2, mat_pow_mod
    m = GOLDEN["matrices"]
    assert [list(r) for r in mat_pow_mod(A1, 1 << 72, M1)] == m["A1p72"]
    assert [list(r) for r in mat_pow_mod(A2, 1 << 72, M2)] == m["A2p72"]
    assert [list(r) for r in mat_pow_mod(A1, 1 << 134, M1)] == m["A1p134"]
    assert [list(r) for r in mat_pow_mod(A2, 1 << 134, M2)] == m["A2p134"]
    assert (M1, M2) == (mrg_util.M1, mrg_util.M2)


def test_the_jump_table_for_one_step_per_piece_is_one_step():
    """Row p of the ``[parts, 18]`` table with c = 1 applied to a state is p steps of the generator,
    on ordinary and on the hand-picked edge states; row 0 is the identity."""
    from aesara_amd.exec_rng import A1, A2, mrg_jump_table
    tab = mrg_jump_table(5, 1)
    assert tab.shape == (5, 18) and tab.dtype == np.int64
    assert tab[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] * 2
    assert tab[1].tolist() == [v for row in A1 for v in row] + [v for row in A2 for v in row]
    rows = [list(r) for r in mrg_util.EDGE_STATES] + mrg_util.substream_states(3).tolist()
    for row in rows:
        cur = list(row)
        for p in range(1, 5):
            cur, _ = mrg_util.step(cur)
            t = tab[p].tolist()
            assert cur == mrg_util.mat_vec([t[0:3], t[3:6], t[6:9]], [t[9:12], t[12:15], t[15:18]], row), (row, p)


@pytest.mark.parametrize("parts,c", [(1, 7), (2, 1), (7, 3), (64, 1), (1000, 481)])
def test_jump_table_rows_are_the_matrix_powers(parts, c):
    from aesara_amd.exec_rng import A1, A2, M1, M2, mat_pow_mod, mrg_jump_table
    tab = mrg_jump_table(parts, c)
    for p in sorted({0, min(1, parts - 1), parts // 2, parts - 1}):
        want = [v for r in mat_pow_mod(A1, p * c, M1) for v in r] + [v for r in mat_pow_mod(A2, p * c, M2) for v in r]
        assert tab[p].tolist() == want, (parts, c, p)
    assert tab.min() >= 0 and tab.max() < 1 << 31


def test_the_choice_of_parts():
    from aesara_amd.exec_rng import mrg_parts
    assert mrg_parts(15360, 1 << 24) == 18                  # ceil(256 * 16 * 64 / 15360)
    assert mrg_parts(1 << 20, 1 << 24) == 1
    assert mrg_parts(5, 6) == 2 and mrg_parts(5, 5) == 1    # at most one piece per sample
    assert mrg_parts(5, 188, forced=64) == 64


# ------------------------------------------------------------------ host logic --------
def test_dry_runs_call_the_c_abi_only_and_raise_the_host_errors(monkeypatch):
    from aesara_amd.executor import PlanExecutor
    st = mrg_util.case_state("s5_188")
    monkeypatch.setenv("AESARA_HIP_MRG_PARTS", "3")
    ex = PlanExecutor(mrg_util.uniform_plan(1, "float32", (188,)), dry_run=True)
    new, sample = ex(st)
    assert ex.trace == ["ahip_mrg_uniform"] and new.shape == (5, 6) and sample.shape == (188,)
    ex = PlanExecutor(mrg_util.uniform_plan(2, "float64", (3, 0)), dry_run=True)
    ex(st)
    assert "ahip_mrg_uniform" not in ex.trace
    with pytest.raises(ValueError, match=r"size must have length 1 \(not 2\)"):
        PlanExecutor(mrg_util.uniform_plan(1, "float32", None), dry_run=True)(st, np.asarray([2, 3], "int64"))
    with pytest.raises(ValueError, match="rstate must have 6 columns"):
        PlanExecutor(mrg_util.uniform_plan(1, "float32", (4,)), dry_run=True)(np.zeros((5, 7), "int32"))
    p, u, n = mrg_util.choice_inputs("c65_7_2", "float32")
    ex = PlanExecutor(mrg_util.op_plan("ChoiceFromUniform", "float32", "float32", "auto", n=n), dry_run=True)
    (out,) = ex(p, u)
    assert ex.trace == ["ahip_copy_strided", "ahip_choice_from_uniform"] and out.shape == (65, 2) and out.dtype == "int64"
    with pytest.raises(ValueError, match="Cannot sample without replacement"):
        PlanExecutor(mrg_util.op_plan("ChoiceFromUniform", "float32", "float32", "auto", n=8), dry_run=True)(
            p, np.zeros(65 * 8, "float32"))


def test_fixtures_stay_small():
    import glob
    import os
    sizes = {p: os.path.getsize(p) for p in glob.glob(os.path.join(mrg_util.MRG_GOLDEN, "*"))}
    assert sizes and max(sizes.values()) <= 200_000, max(sizes.items(), key=lambda kv: kv[1])
