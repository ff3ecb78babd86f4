// K15 — the two data-movement kernels of the 2-d convolution: im2col and col2im.
//
// Replaces the layout half of tensor/nnet/abstract_conv.py:2501 AbstractConv.perform, :2834
// AbstractConv_gradWeights.perform and :3191 AbstractConv_gradInputs.perform (padding into a new
// image, SciPy's convolve2d per channel pair, strided slicing of the result): the image is
// unfolded into col[n][(c, i, j)][(oh, ow)] so that the three Ops become products on the MFMA
// GEMM (the algorithm of tensor/nnet/c_code/corr_gemm.c, restated for the device: padding,
// subsampling and dilation are index arithmetic here, nothing is padded or dilated in memory).
//
//   col[n][(c*kh + i)*kw + j][oh*OW + ow] = x[n, c, oh*sh - pad_top + i*dh, ow*sw - pad_left + j*dw]
//
// (zero where that position lies in the padding).  Both kernels are pure streams: im2col writes
// kh*kw times what it reads, col2im reads it.
#include "common.h"

namespace {

struct ColArgs {
  const void* x;   // im2col: the image, read through xs[]; col2im: unused
  void* col;       // [N][C*kh*kw][P] contiguous
  void* dst;       // col2im: the image, [N][C][H][W] contiguous
  int64_t xs[4];   // element strides of x (n, c, h, w)
  int64_t N, C, units;
  int H, W, kh, kw, pt, pl, sh, sw, dh, dw, OH, OW;
  int P, chunks;   // P = OH*OW (im2col) / H*W (col2im) pixels of a row, in `chunks` pieces per row
};
AHIP_PTRS_BEGIN(ColArgs) AHIP_PTR1(x) AHIP_PTR1(col) AHIP_PTR1(dst) AHIP_PTRS_END

template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };

// One unit = 256 * VEC consecutive output pixels of one (n, c, i, j) row of col: the unit's
// coordinates are uniform over the workgroup (scalar arithmetic), a lane divides once to find
// (oh, ow) of its first pixel and walks on from there.  Consecutive lanes hold consecutive pixels:
// the stores are contiguous (16 bytes per lane when ALIGNED: P a multiple of VEC and col 16-byte
// aligned) and the loads are unit-stride wherever sw == 1 and x's last stride is 1.
template <typename T, int VEC, bool ALIGNED>
__global__ __launch_bounds__(256) void im2col_kernel(ColArgs a) {
  const T* __restrict__ x = static_cast<const T*>(a.x);
  T* __restrict__ col = static_cast<T*>(a.col);
  const int64_t rows = a.C * a.kh * a.kw;
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t nr = u / a.chunks;
    const int chunk = (int)(u - nr * a.chunks);
    const int64_t n = nr / rows, row = nr - n * rows;
    const int64_t c = row / (a.kh * a.kw);
    const int tap = (int)(row - c * (a.kh * a.kw));
    const int i = tap / a.kw, j = tap - i * a.kw;
    const int64_t p0 = ((int64_t)chunk * 256 + threadIdx.x) * VEC;
    if (p0 >= a.P) continue;
    int oh = (int)p0 / a.OW, ow = (int)p0 - oh * a.OW;
    const int64_t xbase = n * a.xs[0] + c * a.xs[1];
    const int h0 = i * a.dh - a.pt, w0 = j * a.dw - a.pl;
    T* out = col + nr * (int64_t)a.P + p0;
    Pack<T, VEC> v;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int h = oh * a.sh + h0, w = ow * a.sw + w0;
      const bool inside = p0 + e < a.P && h >= 0 && h < a.H && w >= 0 && w < a.W;
      v.v[e] = inside ? x[xbase + (int64_t)h * a.xs[2] + (int64_t)w * a.xs[3]] : (T)0;
      if (++ow == a.OW) { ow = 0; ++oh; }
    }
    if constexpr (ALIGNED) {
      *reinterpret_cast<Pack<T, VEC>*>(out) = v;
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (p0 + e < a.P) out[e] = v.v[e];
    }
  }
}

// The inverse as a gather: one lane per image element (n, c, h, w) adds, for i = 0 .. kh-1 and
// j = 0 .. kw-1 in that order, the entry of col whose tap (i, j) lies on it — the output pixel
// (oh, ow) with oh*sh + i*dh == h + pad_top and ow*sw + j*dw == w + pad_left, if there is one.
// No atomics, one fixed order: deterministic.  Positions in the padding are never gathered.
template <typename T>
__global__ __launch_bounds__(256) void col2im_kernel(ColArgs a) {
  const T* __restrict__ col = static_cast<const T*>(a.col);
  T* __restrict__ dst = static_cast<T*>(a.dst);
  const int64_t PO = (int64_t)a.OH * a.OW;
  for (int64_t u = blockIdx.x; u < a.units; u += gridDim.x) {
    const int64_t nc = u / a.chunks;                  // n * C + c
    const int chunk = (int)(u - nc * a.chunks);
    const int64_t p = (int64_t)chunk * 256 + threadIdx.x;
    if (p >= a.P) continue;
    const int h = (int)p / a.W, w = (int)p - h * a.W;
    const T* crow = col + nc * (a.kh * a.kw) * PO;    // rows (c, 0, 0) .. of image n
    T sum = (T)0;
    for (int i = 0; i < a.kh; ++i) {
      const int th = h + a.pt - i * a.dh;
      if (th < 0) break;                              // larger i only moves further up
      const int oh = th / a.sh;
      if (oh * a.sh != th || oh >= a.OH) continue;
      for (int j = 0; j < a.kw; ++j) {
        const int tw = w + a.pl - j * a.dw;
        if (tw < 0) break;
        const int ow = tw / a.sw;
        if (ow * a.sw != tw || ow >= a.OW) continue;
        sum += crow[(int64_t)(i * a.kw + j) * PO + (int64_t)oh * a.OW + ow];
      }
    }
    dst[nc * (int64_t)a.P + p] = sum;
  }
}

unsigned unit_grid(int64_t units) {
  int64_t cap = (int64_t)ahip_cu_count() * 8;   // copy.hip's stream grid: 8 workgroups per CU
  if (cap < 1) cap = 1;
  return (unsigned)(units < cap ? units : cap);
}

int fill_args(ColArgs& a, int64_t N, int64_t C, int64_t H, int64_t W, int64_t kh, int64_t kw,
              int64_t pt, int64_t pl, int64_t sh, int64_t sw, int64_t dh, int64_t dw, int64_t OH,
              int64_t OW) {
  AHIP_REQUIRE(N >= 0 && C >= 0 && H >= 0 && W >= 0 && OH >= 0 && OW >= 0, "negative extent");
  AHIP_REQUIRE(kh >= 1 && kw >= 1 && sh >= 1 && sw >= 1 && dh >= 1 && dw >= 1,
               "kernel size, subsample and dilation must be positive");
  AHIP_REQUIRE(pt >= 0 && pl >= 0, "border_mode must be >= 0");
  // pixel coordinates are 32-bit (element offsets are not): keep every intermediate inside int
  const int64_t lim = 1LL << 30;
  AHIP_REQUIRE(H * W < lim && OH * OW < lim && kh * kw < lim && (kh - 1) * dh + pt < lim &&
               (kw - 1) * dw + pl < lim && OH * sh < lim && OW * sw < lim,
               "image plane or kernel too large for the convolution kernels (2^30 pixels)");
  memset(&a, 0, sizeof(a));
  a.N = N; a.C = C;
  a.H = (int)H; a.W = (int)W; a.kh = (int)kh; a.kw = (int)kw; a.pt = (int)pt; a.pl = (int)pl;
  a.sh = (int)sh; a.sw = (int)sw; a.dh = (int)dh; a.dw = (int)dw; a.OH = (int)OH; a.OW = (int)OW;
  return AHIP_OK;
}

template <typename T>
int launch_im2col(ColArgs& a, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  const int64_t per = 256 * VEC;
  a.chunks = (int)((a.P + per - 1) / per);
  a.units = a.N * a.C * a.kh * a.kw * a.chunks;
  const unsigned grid = unit_grid(a.units);
  if (a.P % VEC == 0 && reinterpret_cast<uintptr_t>(a.col) % 16 == 0)
    AHIP_LAUNCH((im2col_kernel<T, VEC, true>), dim3(grid), dim3(256), 0, s, a);
  else
    AHIP_LAUNCH((im2col_kernel<T, VEC, false>), dim3(grid), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // namespace

extern "C" {

int ahip_im2col2d(int dtype, const void* x, const int64_t* x_strides, int64_t N, int64_t C,
                  int64_t H, int64_t W, int64_t kh, int64_t kw, int64_t pad_top, int64_t pad_left,
                  int64_t sh, int64_t sw, int64_t dh, int64_t dw, int64_t OH, int64_t OW, void* col,
                  void* stream) {
  AHIP_REQUIRE(dtype == AHIP_F32 || dtype == AHIP_F64, "im2col: float32 / float64 only, got dtype %d",
               dtype);
  AHIP_REQUIRE(x_strides != nullptr, "null strides");
  ColArgs a;
  int rc = fill_args(a, N, C, H, W, kh, kw, pad_top, pad_left, sh, sw, dh, dw, OH, OW);
  if (rc) return rc;
  if (N * C * OH * OW == 0) return AHIP_OK;
  AHIP_REQUIRE(col != nullptr && (x != nullptr || H * W == 0), "null pointer");
  for (int d = 0; d < 4; ++d) a.xs[d] = x_strides[d];
  a.x = x; a.col = col;
  a.P = (int)(OH * OW);
  hipStream_t s = as_stream(stream);
  return dtype == AHIP_F32 ? launch_im2col<float>(a, s) : launch_im2col<double>(a, s);
}

int ahip_col2im2d(int dtype, const void* col, int64_t N, int64_t C, int64_t H, int64_t W,
                  int64_t kh, int64_t kw, int64_t pad_top, int64_t pad_left, int64_t sh, int64_t sw,
                  int64_t dh, int64_t dw, int64_t OH, int64_t OW, void* out, void* stream) {
  AHIP_REQUIRE(dtype == AHIP_F32 || dtype == AHIP_F64, "col2im: float32 / float64 only, got dtype %d",
               dtype);
  ColArgs a;
  int rc = fill_args(a, N, C, H, W, kh, kw, pad_top, pad_left, sh, sw, dh, dw, OH, OW);
  if (rc) return rc;
  if (N * C * H * W == 0) return AHIP_OK;
  AHIP_REQUIRE(out != nullptr && (col != nullptr || OH * OW == 0), "null pointer");
  a.col = const_cast<void*>(col); a.dst = out;
  a.P = (int)(H * W);
  a.chunks = (a.P + 255) / 256;
  a.units = N * C * a.chunks;
  hipStream_t s = as_stream(stream);
  const unsigned grid = unit_grid(a.units);
  if (dtype == AHIP_F32) AHIP_LAUNCH((col2im_kernel<float>), dim3(grid), dim3(256), 0, s, a);
  else AHIP_LAUNCH((col2im_kernel<double>), dim3(grid), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // extern "C"
