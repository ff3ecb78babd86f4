"""The patch extractor of a PlanExecutor: ``Images2Neibs`` (reference: tensor/nnet/neighbours.py:23, perform
:194) on the kernel of csrc/neibs.hip.

``ten4`` is ``(N, C, H, W)``; the result has one row per ``r x c`` patch, ``z_row = b + grid_c (a + grid_r (s +
C n))``, whose element ``(i, j)`` is ``ten4[n, s, a step_r + i + off_r, b step_c + j + off_c]``.  The five modes
differ in the grid and in the offset of patch ``(0, 0)`` only (:func:`neibs_geometry`):

    valid, ignore_borders   offset (0, 0)                      grid 1 + (H - r) // step_r
    half                    offset (-(r // 2), -(c // 2))      grid 1 + (H - r % 2) // step_r, zero outside
    full                    offset (-(r - 1), -(c - 1))        grid 1 + (H + r - 2) // step_r, zero outside
    wrap_centered           offset (-(r // 2), -(c // 2))      grid ceil(H / step_r), indices wrapped

``neib_shape`` / ``neib_step`` are operands: host integer vectors, constant or not, read at run time like the
``ws`` / ``stride`` / ``pad`` of exec_pool.py.  Geometry and launch shape follow from their values and the image's
shape alone, so a call records and replays; the reference's errors are raised on the host, in the call.  The image
is read through its strides; the kernel moves bytes, so every dtype of a plan is served by its item size.

:func:`band_split` sizes the LDS-staged bands of the kernel (csrc/neibs.hip checks what it is handed).

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_convolve.py)."""
from __future__ import annotations

import collections

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401
from .exec_pool import _int_vector

MODES = ("valid", "half", "full", "wrap_centered", "ignore_borders")
LDS_BYTES = 32768               # AHIP_NEIBS_LDS_BYTES: LDS of a workgroup (five workgroups share a compute unit's)
MAX_BAND = 32                   # patch rows a workgroup at most: enough to make the re-read halo small
BANKS = 64                      # four-byte LDS banks the row pitch is chosen for

NeibsGeo = collections.namedtuple("NeibsGeo", "grid out_shape offset patch step wrap")


def neibs_geometry(x_shape, neib_shape, neib_step, mode):
    """``NeibsGeo``: the grid ``(grid_r, grid_c)``, the output shape ``(N C grid_r grid_c, r c)`` and the offset of
    patch ``(0, 0)`` in the image; raises what ``Images2Neibs.perform`` raises (neighbours.py:217-299)."""
    if mode not in MODES:
        raise TypeError(f"Images2Neibs: unknown mode '{mode}'")
    if len(x_shape) != 4:
        raise TypeError(f"Images2Neibs: ten4 of {len(x_shape)} dimensions (4 only)")
    N, C, H, W = (int(s) for s in x_shape)
    r, c = _int_vector("neib_shape", neib_shape, 2)
    sr, sc = _int_vector("neib_step", neib_step, 2)
    if sr <= 0 or sc <= 0:
        raise ValueError("neib_step wrong step ; values <= 0. Got " + str(np.asarray(neib_step)))
    if r <= 0 or c <= 0:
        raise ValueError("neib_shape values <=0. Got " + str(np.asarray(neib_shape)))
    off = (0, 0)
    if mode == "wrap_centered":
        if r % 2 != 1 or c % 2 != 1:
            raise TypeError("Images2Neibs: in mode wrap_centered need patch with odd shapes")
        if H < r or W < c:
            raise TypeError("Images2Neibs: in wrap_centered mode, don't support image shapes smaller then the patch "
                            f"shapes: neib_shape=({r},{c}), ten4[2:]=[{H},{W}]")
        grid, off = (-(-H // sr), -(-W // sc)), (-(r // 2), -(c // 2))
    elif mode == "ignore_borders":
        grid = (max(1 + (H - r) // sr, 0), max(1 + (W - c) // sc, 0))
    else:
        # the extent the patches tile exactly: the image (valid), or the image padded by r // 2 (half) or r - 1 (full)
        # on both sides, less the patch
        er, ec = {"valid": (H - r, W - c), "half": (H - r % 2, W - c % 2), "full": (H + r - 2, W + c - 2)}[mode]
        for k, (X, w, s, e) in enumerate(((H, r, sr, er), (W, c, sc, ec))):
            if X < w or e % s != 0:
                raise TypeError(f"neib_shape[{k}]={w}, neib_step[{k}]={s} and ten4.shape[{k + 2}]={X} not consistent")
        grid = (1 + er // sr, 1 + ec // sc)
        off = {"valid": (0, 0), "half": (-(r // 2), -(c // 2)), "full": (-(r - 1), -(c - 1))}[mode]
    return NeibsGeo(grid, (N * C * grid[0] * grid[1], r * c), off, (r, c), (sr, sc), mode == "wrap_centered")


def row_pitch(itemsize, cols, r, c, step_c):
    """LDS row pitch in elements for ``cols`` staged columns: whole 16-byte words, and — where the 64 lanes of one
    store instruction gather from several LDS rows (``r c`` below the elements of 64 words) — congruent modulo the
    banks to the words they read in ONE row, so that the next row's words start on the banks behind them."""
    V = 16 // itemsize
    words = -(-cols // V) * 4
    if r * c < 64 * V:
        span = min(cols, (64 * V // (r * c) + 1) * step_c + c)
        span = min(BANKS, -(-span * itemsize // 16) * 4)
        while words % BANKS != span % BANKS:
            words += 4
    return words * 4 // itemsize


def band_split(itemsize, r, c, step_r, step_c, grid_r, grid_c):
    """``(band, tile, pitch)``: patch rows a workgroup, patch columns a workgroup (``grid_c`` unless one patch row's
    image rows do not fit: then ``band`` is 1) and the LDS row pitch.  ``band`` 0: not even one patch fits."""
    V, elems = 16 // itemsize, LDS_BYTES // itemsize
    # columns of r staged rows left for further patch columns: behind the words row_pitch may add (fewer than
    # BANKS), the up to V - 1 elements in front of an unaligned first column, and the first patch
    room = elems // r // V * V - 4 * BANKS // itemsize - (V - 1) - c
    if room < 0:
        return 0, 0, 0
    tile = min(room // step_c + 1, grid_c)
    pitch = row_pitch(itemsize, V - 1 + (tile - 1) * (step_c if tile > 1 else 0) + c, r, c, step_c)
    if tile < grid_c:
        return 1, tile, pitch
    return min(MAX_BAND, (elems // pitch - r) // min(step_r, r) + 1, grid_r), grid_c, pitch


class NeibsMixin:

    def _op_Images2Neibs(self, node, args):
        """reference: neighbours.py:194 Images2Neibs.perform."""
        x = self.to_device(args[0])
        dt = self.plan.vars[node.outputs[0]].dtype
        if x.dtype != dt:
            raise TypeError(f"{node.op}: an image of dtype {x.dtype} for a {dt} result")
        g = neibs_geometry(x.shape, self.host_array(args[1]), self.host_array(args[2]), node.params["mode"])
        out = self.alloc(g.out_shape, dt)
        if out.size == 0:
            return [out]
        split = band_split(ITEMSIZE[dt], *g.patch, *g.step, *g.grid)
        geo = _i64arr([*g.patch, *g.step, *g.grid, *g.offset, int(g.wrap), *split])
        self._launch("ahip_images2neibs", (dtype_code(dt), _VP(x.ptr), _i64arr(x.shape), _i64arr(x.strides), geo,
                                           _VP(out.ptr), self._stream()))
        return [out]
