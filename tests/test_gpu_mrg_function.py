"""``aesara.sandbox.rng_mrg.MRG_RandomStream`` under ``aesara.function(..., mode="HIP")``: the
reference's front end (from the packed overlay, like tests/test_gpu_pool_function.py) over the real
PlanExecutor, compared with the stored draws of the reference (tests/golden/mrg, the builders of
tools/gen_mrg_golden.py).  Call k of a function returns the reference's k-th draw, bit for bit; the
state stays a device tensor between calls; ``seed()`` restarts the sequence.  Skipped where the
overlay is not packed."""
import os
import sys

import numpy as np
import pytest

import mrg_util
import ref_overlay
from conv_util import graph_cap, rel_l2
from golden_inputs import make_input

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_overlay.available(),
                                 reason="no reference front end (oracle/_ref overlay not packed)")]

GOLDEN = mrg_util.load_mrg_golden()
CASES = {c["name"]: c for c in GOLDEN["function"]}


@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    import aesara_amd
    aesara_amd.get_mode()            # registers linker "hip" / mode "HIP" with the reference
    return ae


@pytest.fixture(scope="module")
def gen(ae):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_mrg_golden
    return gen_mrg_golden


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


@pytest.mark.parametrize("dtype", mrg_util.DTYPES)
@pytest.mark.parametrize("kind", ["uniform", "dropout", "multinomial", "choice"])
def test_three_draws_then_a_reseed(ae, gen, kind, dtype):
    """Calls 1-3 are draws 1-3 of the reference (the second and third are replays of the recorded
    launch list, which must advance the state), the state cell holds a device tensor after the first
    call, and ``srng.seed(...)`` (``set_value`` of host states) restarts the sequence."""
    c = CASES[f"fn_{kind}_{dtype}"]
    z = mrg_util.load_arrays(c["name"])
    f, srng, specs = gen.FUNCTIONS[kind](dtype, "HIP")
    assert specs == c["inputs"]
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert ops.count("MrgUniform") == 1, ops
    if kind in ("multinomial", "choice"):
        assert ops.count({"multinomial": "MultinomialFromUniform", "choice": "ChoiceFromUniform"}[kind]) == 1, ops
    xs = [make_input(s) for s in specs]
    state = srng.state_updates[0][0]
    for k in range(c["calls"]):
        got = _np(f(*xs))
        assert mrg_util.same_bits(got, z[f"draw{k}"]), (c["name"], k)
        cell = state.container.storage[0]
        assert hasattr(cell, "is_cuda") and cell.is_cuda, type(cell)
    srng.seed(GOLDEN["reseed"])
    assert mrg_util.same_bits(_np(f(*xs)), z["reseeded"]), c["name"]
    srng.seed(GOLDEN["fn_seed"])      # (the stream's own state has moved on: not the first sequence)
    assert not np.array_equal(_np(f(*xs)), z["reseeded"])


@pytest.mark.parametrize("dtype", mrg_util.DTYPES)
def test_mlp_step_with_dropout_and_its_gradients(ae, gen, dtype):
    """loss, dW1, dW2 at ``conv_util.graph_cap`` (relative L2 <= max(4 x the reference's own float32
    error against its float64 graph, K * eps)); the dropout mask itself is exact."""
    c = CASES[f"fn_mlp_{dtype}"]
    z = mrg_util.load_arrays(c["name"])
    f, _, specs = gen.fn_mlp(dtype, "HIP")
    assert specs == c["inputs"]
    got = [_np(g) for g in f(*[make_input(s) for s in specs])]
    assert len(got) == c["n_out"]
    assert mrg_util.same_bits(got[3], z["out3"])
    f32 = dtype == "float32"
    for k in range(3):
        ref = z[f"out{k}"]
        assert got[k].shape == ref.shape and got[k].dtype == ref.dtype, (k, got[k].shape, got[k].dtype)
        err, cap = rel_l2(got[k], z[f"exact{k}"] if f32 else ref), graph_cap(c, k)
        print(f"{c['name']} output {k}: rel L2 {err:.3e}, {err / cap:.4f} of the cap {cap:.3e}")
        assert err <= cap, (c["name"], k, err, cap)


@pytest.mark.parametrize("dtype", mrg_util.DTYPES)
def test_normal_of_an_odd_count(ae, gen, dtype):
    """``srng.normal((1001,))``: the uniforms under it are exact, so only the element-wise ``log``,
    ``sqrt``, ``cos`` and ``sin`` differ.  ``exact`` is the Box-Muller formulas in ``longdouble`` on
    the stored uniforms; the bar is 4 x the reference's own relative L2 error against it (both sides
    carry a rounding of the same size: the margin of the graph-level bars)."""
    c = CASES[f"fn_normal_{dtype}"]
    z = mrg_util.load_arrays(c["name"])
    f, _, _ = gen.fn_normal(dtype, "HIP")
    got = _np(f())
    assert got.shape == (1001,) and got.dtype == np.dtype(dtype)
    exact = z["exact_hi"].astype(np.longdouble) + z["exact_lo"].astype(np.longdouble)
    err, bar = rel_l2(got, exact), 4 * c["ref_err"]
    print(f"{c['name']}: rel L2 {err:.3e}, {err / bar:.4f} of the bar {bar:.3e} (reference: {c['ref_err']:.3e})")
    assert err <= bar, (err, bar)
