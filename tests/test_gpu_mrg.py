"""``MrgUniform``, ``MultinomialFromUniform`` and ``ChoiceFromUniform`` on the device: the committed
one-node plans of tests/mrg_util.py through the real PlanExecutor against the stored results of the
reference's C bodies (tests/golden/mrg, tools/gen_mrg_golden.py).  Every comparison is
``np.array_equal``, on the samples AND on the returned state; every uniform case runs for ``parts`` in
{1, 2, 3, 16, 64} through ``AESARA_HIP_MRG_PARTS`` (lanes with empty ranges, more pieces than samples)
and once with the executor's own choice."""
import numpy as np
import pytest

import mrg_util
from mrg_util import CHOICE_CASES, DTYPES, MULTINOMIAL_CASES, PARTS, UNIFORM_CASES, same_bits

pytestmark = pytest.mark.gpu

GOLDEN = mrg_util.load_mrg_golden()
_CACHE = {}


def arrays(name):
    if name not in _CACHE:
        _CACHE[name] = mrg_util.load_arrays(name)
    return _CACHE[name]


def states(name):
    """The stored new states of a uniform case (kept once, in the float32 file)."""
    return arrays(f"u_{name}_float32")


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _executor(plan, **kw):
    from aesara_amd.executor import PlanExecutor
    return PlanExecutor(plan, **kw)


def _set_parts(monkeypatch, parts):
    if parts:
        monkeypatch.setenv("AESARA_HIP_MRG_PARTS", str(parts))
    else:
        monkeypatch.delenv("AESARA_HIP_MRG_PARTS", raising=False)


def test_fixture_states_reach_every_branch_of_the_step():
    assert GOLDEN["corrections"] == {"outcomes_hit": 14, "of": 14}


@pytest.mark.parametrize("parts", (0,) + PARTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [n for n, c in UNIFORM_CASES.items() if not c[2].get("inplace")])
def test_mrg_uniform_has_the_bits_of_the_reference(monkeypatch, name, dtype, parts):
    _set_parts(monkeypatch, parts)
    n_streams, size, opt = UNIFORM_CASES[name]
    z = arrays(f"u_{name}_{dtype}")
    sym = bool(opt.get("symbolic"))
    ex = _executor(mrg_util.uniform_plan(len(size), dtype, None if sym else size))
    state = mrg_util.case_state(name)
    extra = [np.asarray(size, "int64")] if sym else []
    launches = 0
    for k in range(opt.get("calls", 1)):
        new, sample = ex(state, *extra)
        launches = ex.trace.count("ahip_mrg_uniform")
        new, sample = _np(new), _np(sample)
        assert same_bits(sample, z[f"sample{k}"]), (name, dtype, parts, k)
        assert same_bits(new, states(name)[f"state{k}"]), (name, dtype, parts, k)
        state = new
    if name == "zero":
        assert launches == 0 and same_bits(state, mrg_util.case_state(name))     # no launch, unchanged state
    if name == "s5_3":
        assert same_bits(state[3:], mrg_util.case_state(name)[3:])               # untouched streams


@pytest.mark.parametrize("use_graph", (False, True))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ("s5_188", "s65_131"))
def test_three_calls_feed_the_state_back_on_the_device(monkeypatch, name, dtype, use_graph):
    """Draws 1-3 of the reference from ONE executor, the returned device state handed back; with
    ``use_graph`` the second and third call replay the recorded launch list."""
    _set_parts(monkeypatch, 0)
    n_streams, size, _ = UNIFORM_CASES[name]
    z = arrays(f"u_{name}_{dtype}")
    ex = _executor(mrg_util.uniform_plan(len(size), dtype, size), use_graph=use_graph)
    import torch
    state = torch.from_numpy(mrg_util.case_state(name)).cuda()
    for k in range(3):
        state, sample = ex(state)
        assert hasattr(state, "is_cuda") and state.is_cuda
        assert same_bits(_np(sample), z[f"sample{k}"]) and same_bits(_np(state), states(name)[f"state{k}"]), (name, k)


@pytest.mark.parametrize("parts", (1, 3))
@pytest.mark.parametrize("dtype", DTYPES)
def test_inplace_overwrites_the_given_state_buffer(monkeypatch, dtype, parts):
    import torch
    _set_parts(monkeypatch, parts)
    n_streams, size, _ = UNIFORM_CASES["inplace"]
    z = arrays(f"u_inplace_{dtype}")
    ex = _executor(mrg_util.uniform_plan(len(size), dtype, size, inplace=True))
    buf = torch.from_numpy(mrg_util.case_state("inplace")).cuda()
    new, sample = ex(buf)
    assert new.data_ptr() == buf.data_ptr()
    assert same_bits(_np(buf), states("inplace")["state0"]) and same_bits(_np(sample), z["sample0"])


@pytest.mark.parametrize("use_graph", (False, True))
def test_inplace_calls_advance_the_buffer_once_each(monkeypatch, use_graph):
    """Three calls on ONE buffer (the operands of case s5_188): after call k it holds the reference's
    state k — also with ``use_graph``, where an in-place plan stays on the eager path."""
    import torch
    _set_parts(monkeypatch, 0)
    n_streams, size, _ = UNIFORM_CASES["s5_188"]
    z = arrays("u_s5_188_float32")
    ex = _executor(mrg_util.uniform_plan(len(size), "float32", size, inplace=True), use_graph=use_graph)
    buf = torch.from_numpy(mrg_util.case_state("s5_188")).cuda()
    for k in range(3):
        _, sample = ex(buf)
        assert same_bits(_np(sample), z[f"sample{k}"]) and same_bits(_np(buf), z[f"state{k}"]), k


@pytest.mark.parametrize("parts", (1, 5))
def test_the_reference_sample_file_is_reproduced_exactly(monkeypatch, parts):
    """12 streams x 7 substreams x 5 samples from seed 12345 (``test_consistency_cpu_serial`` of the
    reference: stream i 2^134 steps after stream i-1, substream j 2^72 steps after j-1), one state
    row per substream, float64: the file's values, bit for bit."""
    _set_parts(monkeypatch, parts)
    ex = _executor(mrg_util.uniform_plan(1, "float64", (420,)))
    _, sample = ex(mrg_util.sample_file_states())
    got = _np(sample).reshape(5, 84).T.reshape(-1)
    assert same_bits(got, mrg_util.load_sample_file())


def test_host_side_refusals_carry_the_words_of_the_reference():
    st = mrg_util.case_state("s5_5")
    with pytest.raises(ValueError, match="size must be vector"):
        _executor(mrg_util.uniform_plan(2, "float32", None, size_ndim=2))(st, np.ones((1, 2), "int64"))
    with pytest.raises(ValueError, match=r"size must have length 2 \(not 3\)"):
        _executor(mrg_util.uniform_plan(2, "float32", None))(st, np.asarray([2, 3, 4], "int64"))
    with pytest.raises(ValueError, match="rstate must be matrix"):
        _executor(mrg_util.uniform_plan(1, "float32", (4,), rstate_ndim=1))(st[0])
    with pytest.raises(ValueError, match="rstate must have 6 columns"):
        _executor(mrg_util.uniform_plan(1, "float32", (4,)))(np.ascontiguousarray(st[:, :5]))
    with pytest.raises(ValueError, match="rstate must be int32"):
        _executor(mrg_util.uniform_plan(1, "float32", (4,), rstate_dtype="int64"))(st.astype("int64"))
    with pytest.raises(ValueError, match=r"\(2\*\*31 -1\) samples"):
        _executor(mrg_util.uniform_plan(2, "float32", None))(st, np.asarray([1 << 16, 1 << 15], "int64"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(MULTINOMIAL_CASES))
def test_multinomial_from_uniform(name, dtype):
    pvals, unis, n = mrg_util.multinomial_inputs(name, dtype)
    od = MULTINOMIAL_CASES[name][3]
    want = arrays(f"{name}_{dtype}")["out"]
    # n as a constant, and as a run-time scalar input
    (got,) = _executor(mrg_util.op_plan("MultinomialFromUniform", dtype, dtype, od, n=n))(pvals, unis)
    assert same_bits(_np(got), want), (name, dtype)
    (got,) = _executor(mrg_util.op_plan("MultinomialFromUniform", dtype, dtype, od))(pvals, unis, np.asarray(n, "int64"))
    assert same_bits(_np(got), want), (name, dtype)


@pytest.mark.parametrize("udtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_multinomial_rows_on_the_seams(dtype, udtype):
    """u exactly a partial sum (strict ``>``), u equal to the total (a row of zeros, where the
    reference's ``perform`` raises and its C body writes zeros), the row [-2, 2, 0]."""
    pvals, unis, n = mrg_util.multinomial_special(dtype, udtype)
    (got,) = _executor(mrg_util.op_plan("MultinomialFromUniform", dtype, udtype, "int64", n=n))(pvals, unis)
    assert same_bits(_np(got), arrays(f"mspecial_{dtype}_{udtype}")["out"])
    assert _np(got).tolist() == [[0, 1, 1], [1, 0, 0], [0, 0, 0], [0, 1, 1]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CHOICE_CASES))
def test_choice_from_uniform(name, dtype):
    pvals, unis, n = mrg_util.choice_inputs(name, dtype)
    od = CHOICE_CASES[name][3]
    keep = pvals.copy()
    (got,) = _executor(mrg_util.op_plan("ChoiceFromUniform", dtype, dtype, od))(pvals, unis, np.asarray(n, "int64"))
    assert same_bits(_np(got), arrays(f"{name}_{dtype}")["out"]), (name, dtype)
    assert np.array_equal(pvals, keep)
    # a strided view of pvals gives the same draws
    wide = np.zeros((pvals.shape[0], 2 * pvals.shape[1]), dtype)
    wide[:, ::2] = pvals
    import torch
    (got,) = _executor(mrg_util.op_plan("ChoiceFromUniform", dtype, dtype, od, n=n))(torch.from_numpy(wide).cuda()[:, ::2],
                                                                                    unis)
    assert same_bits(_np(got), arrays(f"{name}_{dtype}")["out"]), (name, dtype, "strided")


def test_multinomial_refusals():
    p, u = np.full((3, 4), 0.25, "float32"), np.full(6, 0.5, "float32")
    with pytest.raises(ValueError, match=r"unis.shape\[0\] != pvals.shape\[0\] \* n"):
        _executor(mrg_util.op_plan("MultinomialFromUniform", "float32", "float32", "int64", n=1))(p, u)
    with pytest.raises(ValueError, match=r"unis.shape\[0\] != pvals.shape\[0\] \* n"):
        _executor(mrg_util.op_plan("ChoiceFromUniform", "float32", "float32", "int64", n=1))(p, u)
    with pytest.raises(ValueError, match="Cannot sample without replacement n samples bigger than the size"):
        _executor(mrg_util.op_plan("ChoiceFromUniform", "float32", "float32", "int64", n=5))(p, np.full(15, 0.5, "float32"))
    with pytest.raises(TypeError, match="pvals ndim should be 2"):
        _executor(mrg_util.op_plan("MultinomialFromUniform", "float32", "float32", "int64", n=2, pvals_ndim=1))(p[0], u)
    with pytest.raises(TypeError, match="unis ndim should be 2"):
        _executor(mrg_util.op_plan("ChoiceFromUniform", "float32", "float32", "int64", n=2, unis_ndim=2))(p, u.reshape(3, 2))
