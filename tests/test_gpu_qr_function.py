"""``nlinalg.qr`` under ``aesara.function(..., mode="HIP")``: the reference's front end (from the packed
overlay, like tests/test_gpu_linalg_function.py) over the real PlanExecutor — a least-squares solve
``solve_triangular(R, Q.T @ b)`` that never leaves the device, and ``qr(A, "r")`` alone — compared with
the stored float64 reference outputs of tests/golden/qr at the caps of tests/qr_util.py.  Skipped
where the overlay is not packed."""
import os
import sys

import numpy as np
import pytest

import qr_util
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
    import gen_qr_golden
    return gen_qr_golden


def _np(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


@pytest.mark.parametrize("dtype", qr_util.DTYPES)
def test_least_squares_through_qr_and_a_triangular_solve(ae, gen, dtype):
    """x = solve_triangular(R, Q^T b), Q, R = qr(A), on a 130 x 66 matrix with b = A x0."""
    f = ae.function(*gen.lstsq_graph(dtype), mode="HIP")
    ops = [n.op for n in f.maker.linker.plan.nodes]
    assert "QR" in ops and "SolveTriangular" in ops, ops
    z = np.load(qr_util.graph_file("g_lstsq", dtype))
    cap = qr_util.lstsq_cap(z, dtype)
    A, b = qr_util.lstsq_values(dtype)
    got = []
    for call in range(3):                # the second and third calls replay the recorded launch list
        x = _np(f(A, b)[0])
        assert x.shape == (qr_util.LSTSQ_N,) and x.dtype == np.dtype(dtype)
        err = qr_util._rel(x, z["x64"])
        print(f"g_lstsq {dtype}, call {call}: {err:.3e}, {err / cap:.4f} of the cap {cap:.3e}")
        assert err <= cap, (dtype, call, err, cap)
        got.append(x)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize("dtype", qr_util.DTYPES)
def test_r_alone(ae, gen, dtype):
    f = ae.function(*gen.r_graph(dtype), mode="HIP")
    assert [n.op for n in f.maker.linker.plan.nodes] == ["QR"]
    z = np.load(qr_util.graph_file("g_r", dtype))
    A, _ = qr_util.lstsq_values(dtype)
    fbar = 2.0 * np.sqrt(2.0) * float(z["kappa2"]) * qr_util.res_bar(z, dtype)
    for call in range(3):
        R = _np(f(A)[0])
        assert R.shape == (qr_util.LSTSQ_N, qr_util.LSTSQ_N) and R.dtype == np.dtype(dtype)
        err = qr_util._rel(R, z["R64"])
        print(f"g_r {dtype}, call {call}: {err:.3e}, {err / fbar:.4f} of the bar {fbar:.3e}")
        assert err <= fbar and not np.any(np.tril(R, -1))
        assert np.array_equal(np.sign(np.diag(R)), np.sign(np.diag(z["R64"])))
