"""Every instantiation of aesara_amd/csrc/gemm.hip run at its smallest shape, straight through the
C-ABI (``ahip_gemm`` / ``ahip_gemm_batched`` / ``ahip_gemm_splitk``), so that the test owns C, Cin
and their strides — the executor always hands the kernels a fresh contiguous output.

tests/gemm_util.py holds the case table and explains the buffers (NaN everywhere outside the
views, a full tile of margin), the two value regimes (A: small integers, bit-exact; B: normal
values against the derived element-wise bar) and the route names.  Each case forces the
dispatcher's parameters, asserts that ``ahip_gemm_last_route()`` is the instantiation it was written
for, that nothing outside ``C[0:M, 0:N]`` changed, that the view holds no NaN, and the values in
both regimes.  tests/test_gemm_route_table.py checks without a device that the table names every
instantiation.
"""
import collections

import pytest

import gemm_util as gu

pytestmark = pytest.mark.gpu

_worst = collections.defaultdict(float)     # route -> worst regime-B ratio seen in this session


@pytest.fixture(autouse=True)
def default_params():
    """Whatever a case forced, the dispatcher's defaults are back after it."""
    try:
        yield
    finally:
        gu.set_params({})


def _run(case):
    for regime in ("A", "B"):
        ratio = gu.run_case(case, regime)
        if regime == "B":
            _worst[case.route] = max(_worst[case.route], ratio)
            print("%s  %s  worst |got - exact| / bar = %.3f (route worst %.3f)"
                  % (case.id, case.route, ratio, _worst[case.route]))


def _param(*families):
    cases = gu.cases_of(*families)
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


@_param("big_e0", "big_e2", "big_e1")
def test_big_tile_vector_staged(case):
    """128x128 tile, both operands vector-staged, all four layouts: interior tiles over one, two,
    three and five slabs (the two-deep prefetch has a special case for each), ragged M / N through
    the bounded descriptors (e2), ragged K fully predicated (e1)."""
    _run(case)


@_param("big_scalar")
def test_big_tile_scalar_staged(case):
    """128x128 tile with a scalar-staged operand (always the predicated instantiation): made by an
    odd row pitch, a base pointer off by one element, an odd K and reversed rows."""
    _run(case)


@_param("big_fold")
def test_big_tile_chunked_fold(case):
    """float32, K > 2048: the accumulators are folded into C every 64 slabs; the first fold adds
    beta * Cin (with strides of its own, or aliasing C), the later ones the partial already in C."""
    _run(case)


@_param("big_walk", "big_batch")
def test_big_tile_walk_and_batch(case):
    """The workgroup walk over 10 x 3 tiles for groups of 1, 2 and 8 tile-rows (every tile is
    visited once: no NaN, nothing outside), and batched calls: ordinary strides, a broadcast A, and
    a batch stride that takes A to scalar staging."""
    _run(case)


@_param("half_e0", "half_e2", "half_ks1", "half_walk", "half_batch")
def test_half_tile(case):
    """64x64 tile: interior and ragged, 1, 2 and 4 K groups per workgroup chosen by the case, all four
    layouts, one and three slabs, the tile walk and a batched call."""
    _run(case)


@_param("skinny")
def test_skinny(case):
    """16-row vector-load kernel: tile widths 1, 2, 4, B along n or along k, 4, 8 and 16 wavefronts
    over K (the last ones with an empty range at K = 1024 + VEC), the all-loads-first path."""
    _run(case)


@_param("tn", "small", "scale")
def test_tn_small_scale(case):
    """The weight-gradient kernel, the scalar-load 16x16 kernel, and C = beta * Cin for K == 0 or
    alpha == 0."""
    _run(case)


@_param("none")
def test_zero_extent_launches_nothing(case):
    """M, N or batch zero: no launch, the C buffer untouched."""
    _run(case)


@_param("splitk")
def test_splitk(case):
    """K slices of the big kernel into a workspace and the ordered reduction; a workspace one byte
    too small is exactly ``ahip_gemm``."""
    _run(case)
