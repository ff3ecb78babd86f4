"""Det / MatrixInverse / Eigvalsh / Expm of a STACK of small matrices on the device (csrc/linalg_tile.hip and the
``batched`` routes of exec_linalg.py, exec_eig.py, exec_expm.py): one-node plans on ``[T, n, n]`` operands, and
``aesara.map`` under ``mode="HIP"`` for the map rule of scan_rewrite.batch_map_step.

The reference is NumPy / SciPy in float64, matrix by matrix.  Every matrix of a stack is judged with the bars
tests/linalg_util.py applies to the single-matrix ``inv`` / ``det`` case (``E`` = P |L| |U| of SciPy's float64 LU,
``kappa`` and ``S`` from it as tools/gen_linalg_golden.py computes them); eigenvalues and exponentials with the bars of
tests/test_gpu_eigvalsh.py and tests/test_gpu_expm.py.  The sizes are the edges of the kernel: one wavefront a matrix
up to 32 rows, one workgroup up to 64, the host loop above; T = 5 and 257 leave the last workgroup ragged."""
import functools

import numpy as np
import pytest
import scipy.linalg
import torch

import linalg_util
import ref_overlay
import test_gpu_eigvalsh as eig
import test_gpu_expm as expm
from aesara_amd.plan import Node, Plan
from linalg_util import DTYPES

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_overlay.available(),
                                     reason="no reference front end (oracle/_ref overlay not packed)")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def executor(op, dtype):
    from aesara_amd.executor import PlanExecutor
    plan = Plan(f"stack_{op}_{dtype}", {}, [], [], [])
    a, out = plan.new_var(dtype, [None] * 3, "A"), plan.new_var(dtype, [None] * (1 if op == "Det" else 3))
    plan.inputs, plan.outputs = [a], [out]
    plan.nodes.append(Node(op, [a], [out], {"batched": True}))
    return PlanExecutor(plan, use_graph=True)


def run2(op, dtype, a):
    """The result of the recording call; the replay must repeat its bits."""
    ex = executor(op, dtype)
    first, second = (ex(a)[0].cpu().numpy() for _ in range(2))
    assert len(ex._graphs) == 1 and not ex._no_replay and first.dtype == np.dtype(dtype)
    assert np.array_equal(first, second, equal_nan=True)
    return first


@functools.lru_cache(maxsize=None)
def stack(n, T, dtype, reverse=False):
    """(the stack as float64 values exact in ``dtype``; per matrix: E, kappa, S, the float64 inverse and det).
    ``reverse``: a diagonally dominant matrix with its rows reversed, every pivot out of place."""
    mats, refs = [np.zeros((0, n, n))], []
    for t in range(T):
        if reverse:
            M = (linalg_util._gauss(n, n, 8000 + t, dtype) / n + 2.0 * np.eye(n))[::-1]
        else:                        # (halved: |det| stays inside the float32 range, linalg_util.matrix)
            M = linalg_util._well(n, 7000 + 31 * n + t, dtype) * 0.5
        M = M.astype(dtype).astype("float64")
        P, L, U = scipy.linalg.lu(M)
        E, Minv = (P @ (np.abs(L) @ np.abs(U))) * (1.0 + 1e-6), np.linalg.inv(M)
        refs.append((E, float(np.max(np.sum(np.abs(Minv) @ E, axis=1))), float(np.sum(np.abs(Minv).T * E)),
                     Minv, np.linalg.det(M)))
        mats.append(M[None])
    return np.concatenate(mats), refs


def check(n, T, dtype, dets, invs, reverse=False, skip=()):
    A, refs = stack(n, T, dtype, reverse)
    assert dets.shape == (T,) and invs.shape == (T, n, n)
    for t, (E, kappa, S, x64, d64) in enumerate(refs):
        r = {"det": linalg_util.det_ratio(dets[t], d64, S, n, dtype),
             "residual": linalg_util.residual_ratio(A[t], E, invs[t], np.eye(n), 6 * n, dtype),
             "forward": linalg_util.forward_ratio(invs[t], x64, kappa, 6 * n, dtype)}
        print(f"n={n} T={T} {dtype} matrix {t}: " + ", ".join(f"{k} at {v:.3f} of its bar" for k, v in r.items()))
        assert t in skip or all(v <= 1.0 for v in r.values()), (n, T, dtype, t, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 5, 257])
@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 31, 32, 33, 63, 64, 65])
def test_det_and_inverse_of_every_matrix_of_a_stack(n, T, dtype):
    a = dev(stack(n, T, dtype)[0].astype(dtype))
    check(n, T, dtype, run2("Det", dtype, a), run2("MatrixInverse", dtype, a))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("variant", ["transposed", "every_second", "reversed_rows"])
def test_views_and_pivoting(variant, n, dtype):
    reverse = variant == "reversed_rows"
    A = stack(n, 5, dtype, reverse)[0].astype(dtype)
    if variant == "transposed":              # a_rs and a_cs swapped
        a = dev(A.transpose(0, 2, 1)).transpose(1, 2)
    else:                                    # a_bs doubled (the matrices between hold NaN)
        a = torch.full((10, n, n), float("nan"), dtype=dev(A).dtype, device="cuda")[::2]
        a.copy_(dev(A))
    assert not a.is_contiguous()
    check(n, 5, dtype, run2("Det", dtype, a), run2("MatrixInverse", dtype, a), reverse)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [17, 40])
def test_a_singular_member(n, dtype):
    """Matrix 2 has two equal rows: the second one cancels exactly when the first becomes a pivot."""
    good = stack(n, 5, dtype)[0].astype(dtype)
    bad = good.copy()
    bad[2, n - 1] = bad[2, 0]
    dets = run2("Det", dtype, dev(bad))
    assert dets[2] == 0.0
    check(n, 5, dtype, dets, run2("MatrixInverse", dtype, dev(good)), skip=(2,))
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):          # in a recording call
        executor("MatrixInverse", dtype)(dev(bad))
    ex, a = executor("MatrixInverse", dtype), dev(good)
    first = ex(a)[0].cpu().numpy()
    a.copy_(dev(bad))
    with pytest.raises(np.linalg.LinAlgError, match="Singular matrix"):          # in a replay
        ex(a)
    a.copy_(dev(good))
    assert np.array_equal(ex(a)[0].cpu().numpy(), first) and len(ex._graphs) == 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n", [(0, 4), (3, 0)])
def test_empty_extents(T, n, dtype):
    a = dev(np.zeros((T, n, n), dtype))
    dets, invs = (executor(op, dtype)(a)[0].cpu().numpy() for op in ("Det", "MatrixInverse"))
    assert invs.shape == (T, n, n) and invs.dtype == dets.dtype == np.dtype(dtype)
    assert np.array_equal(dets, np.ones(T, dtype))


# ------------------------------------------------------------------ through aesara.map ----
@pytest.fixture(scope="module")
def ae():
    ae = ref_overlay.import_reference()
    import aesara_amd
    aesara_amd.get_mode()            # registers linker "hip" / mode "HIP" with the reference
    return ae


def run_map(ae, fn, A, dtype, wrt=False):
    """The map of ``fn`` over the stack ``A`` (or the gradient of sum log |.| of it) under mode="HIP"."""
    import aesara
    import aesara.tensor as at
    As = at.tensor3("As", dtype=dtype)
    ys, _ = aesara.map(fn, [As])
    f = ae.function([As], aesara.grad(at.sum(at.log(abs(ys))), As) if wrt else ys, mode="HIP")
    got = f(A.astype(dtype))
    modes = f.maker.linker.executor.scan_modes
    assert modes and set(modes.values()) == {"all-rows"}, modes
    return got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)


@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op,n", [("eigvalsh", 8), ("eigvalsh", 64), ("expm", 8), ("expm", 48)])
def test_map_of_eigvalsh_and_expm(ae, op, n, dtype):
    from aesara.tensor import slinalg
    from aesara.tensor.type_other import NoneConst
    if op == "eigvalsh":
        Ms = [eig.symmetric("gauss", n, dtype, seed=t) for t in range(5)]
        got = run_map(ae, lambda a: slinalg.eigvalsh(a, NoneConst), np.stack(Ms), dtype)
    else:
        Ms = [expm.gaussian(n, 0.9, seed=t) for t in range(5)]
        got = run_map(ae, slinalg.expm, np.stack(Ms), dtype)
    assert got.shape == (5, n) + ((n,) if op == "expm" else ())
    for t, M in enumerate(Ms):
        if op == "eigvalsh":
            eig.check(got[t], M, dtype, f"map eigvalsh n={n} t={t} {dtype}")
        else:
            expm.check(got[t], *expm.reference(M), dtype, f"map expm n={n} t={t}")


@needs_reference
def test_gradient_of_a_map_of_det(ae):
    """d / dA sum log |det A_t| = inv(A_t)^T: the gradient Scan is a map over MatrixInverse, Det and element-wise
    nodes and goes through the same rule.  Three stages of the single-matrix forward limit (det, inverse, their
    product), linalg_util.graph_cap's form, float64 against float64 at twice that."""
    from aesara.tensor import nlinalg
    n, T = 17, 5
    A, refs = stack(n, T, "float64")
    got = run_map(ae, nlinalg.det, A, "float64", wrt=True)
    assert got.shape == (T, n, n)
    for t, (_E, kappa, _S, x64, _d) in enumerate(refs):
        err, cap = linalg_util.rel_max(got[t], x64.T), 2.0 * 3 * 6 * n * linalg_util.eps("float64") * kappa
        print(f"grad t={t}: {err:.3e}, {err / cap:.4f} of the cap {cap:.3e}")
        assert err <= cap, (t, err, cap)
