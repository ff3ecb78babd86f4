"""``at.convolve`` through the lowering and the executor's host logic (no GPU): one ``Convolve`` node with its
mode, a cast in front of a mixed pair, refusals by name, dry-run shapes for the three modes, NumPy's words for
an empty operand, and the split workspace from the shapes alone."""
import numpy as np
import pytest

from test_eigvalsh_lowering import dry, dummy_mode
from test_expm_lowering import ae, needs_reference  # noqa: F401
from test_gpu_convolve import MODES, SPLIT, plan_of


@needs_reference
@pytest.mark.parametrize("mode", MODES)
def test_convolve_lowers_to_one_node(ae, mode):
    """Without the lowering the compile raises ``UnsupportedOp: Convolve has no HIP lowering``."""
    import aesara.tensor as at
    a, v, w = at.vector("a", dtype="float32"), at.vector("v", dtype="float32"), at.vector("w", dtype="float64")
    plan = ae.function([a, v], at.convolve(a, v, mode), mode=dummy_mode()).maker.linker.plan
    assert [(n.op, n.params) for n in plan.nodes] == [("Convolve", {"mode": mode})]
    plan = ae.function([a, w], at.convolve(a, w, mode), mode=dummy_mode()).maker.linker.plan
    assert [n.op for n in plan.nodes] == ["Elemwise", "Convolve"]
    assert [plan.vars[x].dtype for x in plan.nodes[1].inputs + plan.nodes[1].outputs] == ["float64"] * 3


@needs_reference
@pytest.mark.parametrize("dtype", ["bool", "complex128", "float16"])
def test_other_dtypes_are_refused_by_name(ae, dtype):
    """(a constant operand: a complex or float16 graph INPUT is refused earlier, in the plan boundary's own words)"""
    import aesara.tensor as at
    from aesara_amd.lower import UnsupportedOp
    a, v = at.constant(np.ones(3, dtype)), at.vector("v", dtype="float32")
    with pytest.raises(UnsupportedOp, match=rf"^Convolve has no HIP lowering for operands of dtypes.*{dtype}"):
        ae.function([v], at.convolve(a, v), mode=dummy_mode())


@pytest.mark.parametrize("m,n", [(9, 4), (4, 9), (8, 8), (1, 1)])
@pytest.mark.parametrize("mode", MODES)
def test_dry_run_shapes(m, n, mode):
    from aesara_amd import dist
    assert "Convolve" in dist._VIEW_REP_ONLY                                 # replicated under sharding
    ex, (out,) = dry(plan_of("int16", mode), np.zeros(m, "int16"), np.zeros(n, "int16"))
    assert tuple(out.shape) == np.convolve(np.zeros(m), np.zeros(n), mode).shape and out.dtype == "int16"
    assert ex.trace == ["ahip_convolve"]


@pytest.mark.parametrize("m,n,words", [(0, 3, "v cannot be empty"), (3, 0, "v cannot be empty"),
                                       (0, 0, "a cannot be empty")])
def test_an_empty_operand_raises_numpys_words(m, n, words):
    with pytest.raises(ValueError, match=words):
        dry(plan_of("float32", "full"), np.zeros(m, "float32"), np.zeros(n, "float32"))


def test_the_split_workspace_follows_from_the_shapes():
    """No split from 256 tiles on; one tile and 17 chunks of taps: 17 rows; never more splits than chunks (2)."""
    from aesara_amd._lib import DTYPE_CODES, lib
    from aesara_amd.exec_convolve import TAP_CHUNK, TILE_OUT, window
    f32, f64 = DTYPE_CODES["float32"], DTYPE_CODES["float64"]
    m, n = 256 * TILE_OUT, 64 * TAP_CHUNK
    assert lib.ahip_convolve_ws_bytes(f32, m, n, *window("same", m, n)) == 0
    m, n = SPLIT
    assert lib.ahip_convolve_ws_bytes(f32, m, n, *window("valid", m, n)) == 17 * 3 * 4
    assert lib.ahip_convolve_ws_bytes(f64, m, n, *window("valid", m, n)) == 17 * 3 * 8
    assert lib.ahip_convolve_ws_bytes(f32, 6000, 300, 0, 6299) == 2 * 6299 * 4
