"""The executor's launchers of the GEMM, the GEMV and the strided copy (no GPU): each is the one place
that writes the argument tuple of its C-ABI entry point, so the exact tuple is asserted here, in dry
runs, at the smallest shapes that exercise each convention."""
import ctypes as C

import numpy as np
import pytest

from aesara_amd._lib import lib
from aesara_amd.device import ITEMSIZE, DevArray, contiguous_strides, dtype_code
from aesara_amd.exec_common import _FakeBuf, neutral_strides
from aesara_amd.exec_conv import ConvMixin
from aesara_amd.executor import PlanExecutor
from aesara_amd.plan import Plan

F32, F64 = dtype_code("float32"), dtype_code("float64")


def fake(shape, dtype="float32"):
    return DevArray(_FakeBuf(max(int(np.prod(shape)), 1), dtype), 0, tuple(shape), contiguous_strides(shape), dtype)


def decode(a):
    if hasattr(a, "_obj"):
        return a._obj.value
    if isinstance(a, C.Array):
        return list(a)
    return a.value if isinstance(a, C._SimpleCData) else a


@pytest.fixture
def ex():
    """A dry-run executor that records (entry point, decoded arguments) and its allocations."""
    e = PlanExecutor(Plan("launchers", {}, [], [], []), dry_run=True)
    e.launches, e.allocs = [], []
    alloc = e.alloc
    e._launch = lambda name, args: e.launches.append((name, [decode(a) for a in args]))

    def recording_alloc(shape, dtype):
        e.allocs.append(alloc(shape, dtype))
        return e.allocs[-1]
    e.alloc = recording_alloc
    return e


def test_launch_gemm_2d_passes_pointers_and_strides_of_the_views(ex):
    """3x2 @ 2x4: A a transposed view, the result a sub-block at element 8 of a 5x6 buffer."""
    a = fake((2, 3))
    A = a.view((3, 2), (1, 3))
    B = fake((2, 4))
    big = fake((5, 6))
    out = big.view((3, 4), big.strides, 1 * 6 + 2)
    assert out.ptr == big.buf.data_ptr() + 8 * 4
    ex._launch_gemm(2.0, A, B, 1.0, out, out)               # beta accumulates in place: Cin is out
    z = fake((3, 4))
    ex._launch_gemm(-1.0, A, B, 0.5, z, out)
    assert not ex.allocs
    assert ex.launches == [
        ("ahip_gemm", [F32, 3, 4, 2, 2.0, a.ptr, 1, 3, B.ptr, 4, 1, 1.0, out.ptr, 6, 1, out.ptr, 6, 1, None]),
        ("ahip_gemm", [F32, 3, 4, 2, -1.0, a.ptr, 1, 3, B.ptr, 4, 1, 0.5, z.ptr, 4, 1, out.ptr, 6, 1, None])]


def test_launch_gemm_3d_is_the_batched_entry_point_with_all_nine_strides(ex):
    """Two products: A broadcast over the batch (stride 0), B in padded slots of 12 > K * N = 8
    elements (the convolution's ``slot``), float64."""
    a, b, out = fake((3, 2), "float64"), fake((2 * 12,), "float64"), fake((2, 3, 4), "float64")
    A = a.view((2, 3, 2), (0, 2, 1))
    B = b.view((2, 2, 4), (12, 4, 1), 3)
    ex._launch_gemm(1.0, A, B, 0.0, out, out)
    assert not ex.allocs
    assert ex.launches == [("ahip_gemm_batched", [F64, 2, 3, 4, 2, 1.0, a.ptr, 0, 2, 1, b.ptr + 3 * 8, 12, 4, 1,
                                                  0.0, out.ptr, 12, 4, 1, out.ptr, 12, 4, 1, None])]


def test_launch_gemm_refuses_views_that_do_not_fit(ex):
    A, B, out = fake((3, 2)), fake((2, 4)), fake((3, 4))
    for bad in ((A, B, out, fake((2, 3, 4))), (A, fake((3, 4)), out, out), (A, B, fake((4, 3)), out),
                (fake((1, 1, 3, 2)), fake((1, 1, 2, 4)), fake((1, 1, 3, 4)), fake((1, 1, 3, 4)))):
        with pytest.raises(ValueError, match="GEMM views"):
            ex._launch_gemm(1.0, bad[0], bad[1], 0.0, bad[2], bad[3])
    assert not ex.launches


@pytest.mark.parametrize("M,N", [(1, 3), (3, 1), (3, 2)])
def test_launch_gemv_stride_conventions_and_its_one_workspace(ex, M, N):
    """A strided matrix (every second row, every third column), a strided x, y updated in place."""
    a, xb, yb = fake((2 * M, 3 * N)), fake((2 * N,)), fake((3 * M,))
    A = a.view((M, N), (6 * N, 3))
    x, y = xb.view((N,), (2,)), yb.view((M,), (3,), 1)
    ex._launch_gemv(-1.0, A, x, 1.0, y, y)
    ws_bytes = int(lib.ahip_gemv_ws_bytes(F32, M, N))
    (ws,) = ex.allocs                                        # exactly one allocation: the workspace
    assert ws.shape == (max(ws_bytes // 4, 1),) and ws.dtype == "float32"
    incy = 3 if M != 1 else 1
    assert ex.launches == [("ahip_gemv", [
        F32, M, N, -1.0, a.ptr,
        6 * N if M != 1 else 0,                              # row stride of A: 0 for one row
        3 if N != 1 else 1,                                  # column stride of A: 1 for one column
        xb.ptr, 2 if N != 1 else 1,                          # incx: 1 for one column
        1.0, yb.ptr + 4, incy, yb.ptr + 4, incy,             # incy / out: the view's stride, 1 for one row
        ws.ptr, ws_bytes, None])]


def test_copy_strided_passes_negative_strides_the_flag_and_skips_empty_results(ex):
    k = fake((2, 1, 2, 3))
    flipped = ConvMixin._conv_flipped(k)                     # the convolution's flipped kernel
    assert flipped.strides == (6, 6, -3, -1) and flipped.ptr == k.ptr + 5 * 4
    dst = fake((2, 1, 2, 3))
    ex._copy_strided(dst, flipped.strides, flipped)
    ex._copy_strided(dst, flipped.strides, flipped, accumulate=True)
    ex._copy_strided(fake((0, 3)), (3, 1), fake((0, 3)))     # an empty destination: no launch
    s0, d0 = fake(()), fake(())
    ex._copy_strided(d0, (), s0)                             # 0-d: one dimension of extent 1
    want = [F32, 4, [2, 1, 2, 3], k.ptr + 20, [6, 6, -3, -1], dst.ptr, [6, 6, 3, 1]]
    assert ex.launches == [("ahip_copy_strided", want + [0, None]), ("ahip_copy_strided", want + [1, None]),
                           ("ahip_copy_strided", [F32, 1, [1], s0.ptr, [0], d0.ptr, [0], 0, None])]
    assert not ex.allocs


def test_copy_into_ends_in_the_same_launch(ex):
    src, dst = fake((3,)), fake((2, 3))
    ex.copy_into(dst, src, accumulate=True)                  # broadcast over the rows
    assert ex.launches == [("ahip_copy_strided", [F32, 2, [2, 3], src.ptr, [0, 1], dst.ptr, [3, 1], 1, None])]


def test_gemm_neutralises_extent_one_strides_and_the_launcher_does_not(ex):
    """1x3 @ 3x1 on views whose extent-1 dimensions carry strides: ``_gemm`` zeroes them for A and
    B, a direct ``_launch_gemm`` hands them on (the convolution passes Kc, not 0, for one filter)."""
    A = fake((7, 3)).view((1, 3), (7, 1))
    B = fake((3, 5)).view((3, 1), (5, 9))
    assert neutral_strides(A).strides == (0, 1) and neutral_strides(B).strides == (5, 0)
    out = ex._gemm(1.0, A, B, 0.0, None)
    assert ex.allocs == [out] and out.shape == (1, 1)
    ex._launch_gemm(1.0, A, B, 0.0, out, out)
    head = [F32, 1, 1, 3, 1.0, A.ptr]
    tail = [0.0, out.ptr, 1, 1, out.ptr, 1, 1, None]
    assert ex.launches == [("ahip_gemm", head + [0, 1, B.ptr, 5, 0] + tail),
                           ("ahip_gemm", head + [7, 1, B.ptr, 5, 9] + tail)]
