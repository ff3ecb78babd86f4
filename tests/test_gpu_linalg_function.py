"""``solve`` / ``solve_triangular`` / ``matrix_inverse`` / ``det`` and ``aesara.grad`` through them, a
Gaussian negative log-likelihood with its gradient, and ``aesara.map`` over solves under
``aesara.function(..., mode="HIP")``: the reference's front end (from the packed overlay, like
tests/test_gpu_pool_function.py) over the real PlanExecutor, compared with the stored reference
outputs of tests/golden/linalg at the graph caps of tests/linalg_util.py.  Skipped where the overlay
is not packed."""
import os
import sys

import numpy as np
import pytest

import linalg_util
import ref_overlay

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_overlay.available(),
                                 reason="no reference front end (oracle/_ref overlay not packed)")]


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
    import gen_linalg_golden
    return gen_linalg_golden


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def _graph(ae, gen, gname, dtype):
    c = linalg_util.load_graph_cases()[gname, dtype]
    ins, outs = gen.GRAPHS[gname](dtype)
    f = ae.function(ins, outs, mode="HIP")
    ops = [n.op for n in f.maker.linker.plan.nodes]
    for k, cnt in linalg_util.GRAPHS[gname][0].items():
        assert ops.count(k) >= cnt, (gname, k, ops)
    z = np.load(linalg_util.graph_file(gname, dtype))
    xs = linalg_util.graph_values(gname, dtype)
    f32 = dtype == "float32"
    for call in range(3):                # the second and third calls replay the recorded launch list
        got = [_np(g) for g in f(*xs)]
        assert len(got) == c["n_out"]
        for k, g in enumerate(got):
            ref = z[f"out{k}"]
            assert g.shape == ref.shape and g.dtype == ref.dtype, (k, g.shape, g.dtype)
            err = linalg_util.rel_max(g, z[f"exact{k}"] if f32 else ref)
            cap = linalg_util.graph_cap(gname, k, dtype, c["kappa"], c["n"])
            print(f"{gname} {dtype} output {k}, call {call}: {err:.3e}, {err / cap:.4f} of the cap {cap:.3e}")
            assert err <= cap, (gname, dtype, k, call, err, cap)
    return f


@pytest.mark.parametrize("dtype", linalg_util.DTYPES)
def test_solve_and_its_gradients(ae, gen, dtype):
    """x = solve(A, b) and the gradients of sum(x * w) with respect to A and b (SolveBase.L_op: a
    second Solve on A.T, then an outer product)."""
    _graph(ae, gen, "g_solve", dtype)


@pytest.mark.parametrize("dtype", linalg_util.DTYPES)
def test_solve_triangular_and_its_gradients(ae, gen, dtype):
    _graph(ae, gen, "g_tri", dtype)


@pytest.mark.parametrize("dtype", linalg_util.DTYPES)
def test_matrix_inverse_and_det_and_their_gradients(ae, gen, dtype):
    _graph(ae, gen, "g_inv_det", dtype)


@pytest.mark.parametrize("dtype", linalg_util.DTYPES)
def test_gaussian_negative_log_likelihood_and_its_gradient(ae, gen, dtype):
    """1/2 r^T S^-1 r + 1/2 log |det S| with S = L L^T + I at n = NB + 1, and d / dL."""
    _graph(ae, gen, "g_nll", dtype)


@pytest.mark.parametrize("dtype", linalg_util.DTYPES)
def test_map_of_solve_over_three_systems(ae, gen, dtype):
    f = _graph(ae, gen, "g_map", dtype)
    modes = f.maker.linker.executor.scan_modes if hasattr(f.maker.linker, "executor") else {}
    assert all(m.startswith("launch-list") for m in modes.values()), modes


def test_a_singular_matrix_raises_through_the_function(ae):
    import aesara.tensor as at
    from aesara.tensor import slinalg
    A, b = at.dmatrix("A"), at.dvector("b")
    f = ae.function([A, b], slinalg.solve(A, b), mode="HIP")
    assert np.allclose(_np(f(np.array([[1.0, 2.0], [3.0, 4.0]]), np.ones(2))), [-1.0, 1.0])
    with pytest.raises(np.linalg.LinAlgError, match="Matrix is singular"):
        f(np.array([[1.0, 2.0], [2.0, 4.0]]), np.ones(2))
