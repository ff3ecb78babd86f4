"""The 2-d convolution Ops of a PlanExecutor: ``Conv2d``, ``Conv2dGradW``, ``Conv2dGradI`` (reference:
tensor/nnet/abstract_conv.py AbstractConv2d :2646, AbstractConv2d_gradWeights :2990,
AbstractConv2d_gradInputs :3361) as im2col / col2im (csrc/conv.hip) around the MFMA GEMM — the
algorithm of the reference's own compiled path (tensor/nnet/c_code/corr_gemm.c), restated.

With ``Kc = (C/G)*kh*kw``, ``P = OH*OW`` and ``col[n][(c, i, j)][(oh, ow)]`` the unfolded image:

* ``Conv2d``:      ``Y[n, g]  (O/G x P)  = W_g (O/G x Kc) @ col[n, g] (Kc x P)``, batched over n;
* ``Conv2dGradW``: ``dW_g    (O/G x Kc) = sum_n dY[n, g] (O/G x P) @ col[n, g].T``: a batched product
  into a workspace [n][O][Kc], then one ordered sum over n (a row of ones times the workspace, on
  the same GEMM: deterministic; images in groups of as many as fit into 64 MiB, later groups added
  with ``beta = 1``, so the order follows from the shapes alone, not from the chunking);
* ``Conv2dGradI``: ``col[n, g] (Kc x P)  = W_g.T @ dY[n, g]``, batched over n, then col2im.

``filter_flip`` touches the kernel tensor only: a flipped contiguous copy of it (tiny) goes into
the products, the weight gradient is flipped back.  The image is never flipped, padded or dilated
in memory.  ``col`` is kh*kw times the image: the batch runs in chunks of as many images as fit
into ``AESARA_HIP_CONV_WS_MB`` — a function of the shapes and the switch only, so a recorded
launch list is the same on every machine.

Part of :class:`aesara_amd.executor.PlanExecutor` (a mixin, like exec_ops.py)."""
from __future__ import annotations

from .exec_common import *  # noqa: F401,F403
from .exec_common import (_I64, _VP, _i64arr, _Kernels, _FakeBuf, _CAST_SCALARS, _prod, _Arena, _os, _time)  # noqa: F401
from .lower_conv import resolve_pad


class _Geo:
    """Sizes of one convolution, checked the way the reference's perform() checks them."""
    __slots__ = ("N", "C", "H", "W", "O", "Cg", "kh", "kw", "G", "Og", "Kc", "pt", "pl", "sh", "sw",
                 "dh", "dw", "OH", "OW", "P", "flip")


def conv_geometry(params, N, C, H, W, O, Cg, kh, kw):       # noqa: N803
    g = _Geo()
    g.N, g.C, g.H, g.W, g.O, g.Cg, g.kh, g.kw = (int(v) for v in (N, C, H, W, O, Cg, kh, kw))
    g.G = int(params["num_groups"])
    (g.sh, g.sw), (g.dh, g.dw) = params["subsample"], params["filter_dilation"]
    g.flip = bool(params["filter_flip"])
    # abstract_conv.py:2329-2337 (BaseAbstractConv.conv)
    if g.C % g.G != 0:
        raise ValueError("number of input channels must be divible by num_groups")
    if g.O % g.G != 0:
        raise ValueError("number of filters must be divisible by num_groups")
    if g.C // g.G != g.Cg:
        raise ValueError("the number of input channels in the kernel should specify the number of "
                         "channels of 1 group")
    if g.kh < 1 or g.kw < 1:
        raise ValueError(f"convolution kernel of size ({g.kh}, {g.kw})")
    dil = ((g.kh - 1) * g.dh + 1, (g.kw - 1) * g.dw + 1)
    (g.pt, pb), (g.pl, pr) = resolve_pad(params["border_mode"], dil)
    if min(g.pt, pb, g.pl, pr) < 0:
        raise ValueError("border_mode must be >= 0")            # get_conv_shape_1axis :152
    # get_conv_shape_1axis :156-163
    g.OH = (g.H + g.pt + pb - dil[0]) // g.sh + 1
    g.OW = (g.W + g.pl + pr - dil[1]) // g.sw + 1
    if g.OH < 0 or g.OW < 0:
        raise ValueError("negative dimensions are not allowed")   # np.zeros(out_shape) in conv()
    g.Og, g.Kc, g.P = g.O // g.G, g.Cg * g.kh * g.kw, g.OH * g.OW
    return g


class ConvMixin:
    CONV_PARTS_BYTES = 64 << 20     # per-image weight-gradient products held before they are summed

    def _conv_operands(self, node, a, b):
        (a, b), dt = self._float_operands(node, (a, b))
        if a.ndim != 4 or b.ndim != 4:
            raise TypeError(f"{node.op}: operands must be 4D tensors, got {a.ndim}D and {b.ndim}D")
        return a, b, dt

    def _conv_chunk(self, g, dt):
        """(images per chunk, elements between two images of ``col``).  The distance is rounded up
        to 16 bytes so that the GEMM sees the same operand alignment for every image, whatever the
        chunking; the chunk depends on the shapes and the switch only."""
        slot = -(-(g.C * g.kh * g.kw * g.P) // 4) * 4
        budget = int(float(knobs.get("CONV_WS_MB")) * (1 << 20))
        return max(1, min(g.N, budget // max(slot * ITEMSIZE[dt], 1))), slot

    @staticmethod
    def _conv_flipped(k: DevArray) -> DevArray:
        s = k.strides
        return k.view(k.shape, (s[0], s[1], -s[2], -s[3]),
                      k.offset + (k.shape[2] - 1) * s[2] + (k.shape[3] - 1) * s[3])

    def _conv_kernel_matrix(self, kern, flip):
        """The kernel as the contiguous [O][Cg*kh*kw] matrix of the products, in correlation
        orientation (flipped when ``filter_flip``: AbstractConv.perform convolves, :2536)."""
        if not flip and kern.is_contiguous():
            return kern
        src = self._conv_flipped(kern) if flip else kern
        wm = self.alloc(src.shape, src.dtype)
        self._copy_strided(wm, src.strides, src)
        return wm

    def _conv_pixels(self, t: DevArray):
        """``t`` (N, O, OH, OW) with one element stride over its (oh, ow) pixels (a copy if the
        two spatial strides do not fold into one); returns (array, that stride)."""
        sh, st = collapse_dims(list(t.shape[2:]), [list(t.strides[2:])])
        if len(sh) != 1:
            packed = self.alloc(t.shape, t.dtype)
            self._copy_strided(packed, t.strides, t)
            return packed, 1
        return t, st[0][0]

    def _conv_cols(self, name, g, dt, x_or_out, n0, nb, col, slot):
        """im2col of images n0 .. n0+nb-1 into ``col`` / col2im of ``col`` into them: one launch
        when the images of ``col`` lie back to back, else one per image."""
        tight = slot == g.C * g.kh * g.kw * g.P
        for k0, kn in ([(0, nb)] if tight or nb == 1 else [(k, 1) for k in range(nb)]):
            a = x_or_out
            ptr = a.ptr + (n0 + k0) * a.strides[0] * a.itemsize
            cptr = col.ptr + k0 * slot * col.itemsize
            geo = (kn, g.C, g.H, g.W, g.kh, g.kw, g.pt, g.pl, g.sh, g.sw, g.dh, g.dw, g.OH, g.OW)
            if name == "ahip_im2col2d":
                self._launch(name, (dtype_code(dt), _VP(ptr), _i64arr(a.strides)) + geo
                             + (_VP(cptr), self._stream()))
            else:
                self._launch(name, (dtype_code(dt), _VP(cptr)) + geo + (_VP(ptr), self._stream()))

    def _op_Conv2d(self, node, args):
        """reference: abstract_conv.py:2501 AbstractConv.perform."""
        img, kern, dt = self._conv_operands(node, args[0], args[1])
        g = conv_geometry(node.params, *img.shape, *kern.shape)
        out = self.alloc((g.N, g.O, g.OH, g.OW), dt)
        if out.size == 0:
            return [out]
        if g.Kc == 0:
            self.fill_zero(out)
            return [out]
        wm = self._conv_kernel_matrix(kern, g.flip)
        nb, slot = self._conv_chunk(g, dt)
        col = self.alloc((nb * slot,), dt)
        for n0 in range(0, g.N, nb):
            n = min(nb, g.N - n0)
            self._conv_cols("ahip_im2col2d", g, dt, img, n0, n, col, slot)
            for grp in range(g.G):
                y = out.view((n, g.Og, g.P), (g.O * g.P, g.P, 1), out.offset + (n0 * g.O + grp * g.Og) * g.P)
                self._launch_gemm(1.0, wm.view((n, g.Og, g.Kc), (0, g.Kc, 1), wm.offset + grp * g.Og * g.Kc),
                                  col.view((n, g.Kc, g.P), (slot, g.P, 1), col.offset + grp * g.Kc * g.P),
                                  0.0, y, y)
        return [out]

    def _op_Conv2dGradW(self, node, args):
        """reference: abstract_conv.py:2834 AbstractConv_gradWeights.perform; ``shape`` = (kh, kw)."""
        img, top, dt = self._conv_operands(node, args[0], args[1])
        shape = [int(v) for v in self.host_array(args[2]).reshape(-1)]
        if len(shape) != 2:
            raise ValueError(f"{node.op}: shape must have 2 entries (kernel rows, columns), got {len(shape)}")
        G = int(node.params["num_groups"])
        N, Cc = img.shape[:2]
        if Cc % G != 0:
            raise ValueError("number of input channels must be divible by num_groups")
        g = conv_geometry(node.params, *img.shape, top.shape[1], Cc // G, *shape)
        if tuple(top.shape) != (g.N, g.O, g.OH, g.OW):
            raise ValueError(f"{node.op}: an image of shape {tuple(img.shape)} and a kernel of "
                             f"{tuple(shape)} produce an output of shape {(g.N, g.O, g.OH, g.OW)}, but "
                             f"the given topgrad has shape {tuple(top.shape)}")
        out = self.alloc((g.O, g.Cg, g.kh, g.kw), dt)
        if out.size == 0:
            return [out]
        if g.N == 0 or g.P == 0:
            self.fill_zero(out)
            return [out]
        top, sp = self._conv_pixels(top)
        dwm = self.alloc(out.shape, dt) if g.flip else out
        nb, slot = self._conv_chunk(g, dt)
        col = self.alloc((nb * slot,), dt)
        # per-image products into ``parts`` [R][O][Kc], then ONE ordered sum over the R images of a
        # group: a row of ones times ``parts`` on the same GEMM (beta = 1 from the second group on).
        # R follows from the shapes alone, so the order of the sum does not depend on the chunking.
        wsz = g.O * g.Kc
        R = max(1, min(g.N, self.CONV_PARTS_BYTES // (wsz * ITEMSIZE[dt])))
        parts = self.alloc((R * wsz,), dt)
        ones = self.alloc((R,), dt)
        one = float_scalar(dt, 1.0)
        self._launch("ahip_fill", (dtype_code(dt), C.byref(one), _VP(ones.ptr), R, self._stream()))
        ts = top.strides
        w = dwm.view((1, wsz), (wsz, 1))
        for n0 in range(0, g.N, nb):
            n = min(nb, g.N - n0)
            self._conv_cols("ahip_im2col2d", g, dt, img, n0, n, col, slot)
            k = 0
            while k < n:
                first = (n0 + k) % R
                m = min(n - k, R - first)
                for grp in range(g.G):
                    c = parts.view((m, g.Og, g.Kc), (wsz, g.Kc, 1), parts.offset + first * wsz + grp * g.Og * g.Kc)
                    self._launch_gemm(
                        1.0, top.view((m, g.Og, g.P), (ts[0], ts[1], sp),
                                      top.offset + (n0 + k) * ts[0] + grp * g.Og * ts[1]),
                        col.view((m, g.P, g.Kc), (slot, 1, g.P), col.offset + k * slot + grp * g.Kc * g.P),
                        0.0, c, c)
                k += m
                if first + m == R or n0 + k == g.N:
                    r = first + m
                    self._launch_gemm(1.0, ones.view((1, r), (r, 1)), parts.view((r, wsz), (wsz, 1)),
                                      0.0 if n0 + k <= R else 1.0, w, w)
        if g.flip:
            flipped = self._conv_flipped(dwm)
            self._copy_strided(out, flipped.strides, flipped)
        return [out]

    def _op_Conv2dGradI(self, node, args):
        """reference: abstract_conv.py:3191 AbstractConv_gradInputs.perform; ``shape`` = (H, W)."""
        kern, top, dt = self._conv_operands(node, args[0], args[1])
        shape = [int(v) for v in self.host_array(args[2]).reshape(-1)]
        if len(shape) != 2:
            raise ValueError(f"{node.op}: shape must have 2 entries (image rows, columns), got {len(shape)}")
        if shape[0] < 0 or shape[1] < 0:
            raise ValueError("negative dimensions are not allowed")
        G = int(node.params["num_groups"])
        g = conv_geometry(node.params, top.shape[0], kern.shape[1] * G, *shape, *kern.shape)
        if tuple(top.shape) != (g.N, g.O, g.OH, g.OW):           # :3216-3226
            raise ValueError(
                "invalid input_shape for gradInputs: the given input_shape would produce an output of "
                f"shape {(g.N, g.O, g.OH, g.OW)}, but the given topgrad has shape {tuple(top.shape)}")
        out = self.alloc((g.N, g.C, g.H, g.W), dt)
        if out.size == 0:
            return [out]
        if g.Og == 0 or g.P == 0:
            self.fill_zero(out)
            return [out]
        wm = self._conv_kernel_matrix(kern, g.flip)
        top, sp = self._conv_pixels(top)
        nb, slot = self._conv_chunk(g, dt)
        col = self.alloc((nb * slot,), dt)
        ts = top.strides
        for n0 in range(0, g.N, nb):
            n = min(nb, g.N - n0)
            for grp in range(g.G):
                c = col.view((n, g.Kc, g.P), (slot, g.P, 1), col.offset + grp * g.Kc * g.P)
                self._launch_gemm(
                    1.0, wm.view((n, g.Kc, g.Og), (0, 1, g.Kc), wm.offset + grp * g.Og * g.Kc),
                    top.view((n, g.Og, g.P), (ts[0], ts[1], sp), top.offset + n0 * ts[0] + grp * g.Og * ts[1]),
                    0.0, c, c)
            self._conv_cols("ahip_col2im2d", g, dt, out, n0, n, col, slot)
        return [out]
