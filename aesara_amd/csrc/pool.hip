// K16 — pooling: Pool, MaxPoolGrad, AveragePoolGrad and DownsampleFactorMaxGradGrad of
// tensor/signal/pool.py (:283, :1162, :1490, :1834), restated for the device.
//
// One kernel family over three pooled dimensions (d, h, w); a 2-d or 1-d pool has window 1 /
// stride 1 / pad 0 in the missing leading ones.  With image extent X, window w, stride s and pad p
// of one dimension, window j covers, in image coordinates,
//
//     [max(j*s - p, 0), min(j*s + w - p, X))
//
// — the region of the reference's C loops (Pool.c_code :840-848 and the same lines of the three
// gradient Ops), which is what every Op here uses: the forward windows.  `average_inc_pad` counts
// the padding cells of a window (divisor min(j*s + w, X + 2p) - j*s per dimension), `average_exc_pad`
// the cells above only, `sum` divides by nothing.
//
// All four kernels are streams bound by HBM: a handful of integer divisions and at most w_d*w_h*w_w
// compares or adds per element moved.  No LDS, no atomics, one lane per element of the result:
//
//   * forward / grad-of-grad: one lane per OUTPUT element walks its window in row-major order (the
//     order of the reference's loop); the image is read through its strides.
//   * both gradients: one lane per INPUT cell gathers, in ascending (d, h, w) window order, from
//     the windows that cover it, j in [ceil((c + p - w + 1) / s), floor((c + p) / s)] clipped to
//     [0, out) — the order in which the reference adds into gx, so the sums have its bits; a cell
//     under no window gets the 0 the lane starts from.
//
// Two special forms carry the common layers at several elements per lane (the general forms keep
// 16 bytes or less in flight per lane): pool_fwd_tile_kernel for windows that
// tile a 2-d image exactly, pool_grad_disjoint_kernel for gradients of non-overlapping windows.
// Both meet the values in the general kernels' order and give their bits.
#include "common.h"

namespace {

enum { POOL_MAX = 0, POOL_SUM = 1, POOL_AVG_INC = 2, POOL_AVG_EXC = 3 };

struct PoolArgs {
  const void* x;   // the image, read through xl[] / xs[] (unused by the average gradient)
  const void* m;   // maxout, contiguous [lead][O]          (max gradient, grad-of-grad)
  const void* g;   // gz, contiguous [lead][O] (gradients) / ggx, contiguous [lead][X] (grad-of-grad)
  void* out;       // contiguous: [lead][O] (forward, grad-of-grad) / [lead][X] (gradients)
  int64_t xl[3];   // element strides of x over its (up to three, collapsed) leading dimensions
  int64_t xs[3];   // ... and over the pooled ones
  int64_t L[3];    // leading extents, 1 where unused
  int64_t total;   // elements of `out`
  int X[3], O[3], w[3], s[3], p[3];
  int mode, nlead;
};
AHIP_PTRS_BEGIN(PoolArgs) AHIP_PTR1(x) AHIP_PTR1(m) AHIP_PTR1(g) AHIP_PTR1(out) AHIP_PTRS_END

struct Pos {
  int c[3];        // coordinates in the pooled dimensions
  int64_t lead;    // flat index over the leading dimensions
  int64_t xbase;   // element offset of that leading index in x
};

// Flat index i over [lead][D0][D1][D2] -> coordinates.  I is 32-bit whenever every count fits.
template <typename I>
__device__ __forceinline__ Pos locate(const PoolArgs& a, I i, const int* D) {
  Pos r;
  I q = i / (I)D[2];
  r.c[2] = (int)(i - q * (I)D[2]);
  I q1 = q / (I)D[1];
  r.c[1] = (int)(q - q1 * (I)D[1]);
  if (D[0] == 1) {
    r.c[0] = 0;
  } else {
    q = q1 / (I)D[0];
    r.c[0] = (int)(q1 - q * (I)D[0]);
    q1 = q;
  }
  r.lead = (int64_t)q1;
  if (a.nlead <= 1) {
    r.xbase = r.lead * a.xl[2];
  } else {
    const int64_t u = r.lead / a.L[2], l2 = r.lead - u * a.L[2];
    const int64_t l0 = u / a.L[1], l1 = u - l0 * a.L[1];
    r.xbase = l0 * a.xl[0] + l1 * a.xl[1] + l2 * a.xl[2];
  }
  return r;
}

// np.max of the window: a NaN anywhere in it wins (the reference's C loop keeps or drops a NaN
// depending on where it sits; its perform does this)
template <typename T>
__device__ __forceinline__ T nan_max(T acc, T v) { return (v != v || v > acc) ? v : acc; }

// Forward.  WV > 0: x's innermost stride is 1, stride_w == ws_w == WV, pad_w == 0 and every
// window row is WV*sizeof(T)-aligned — a whole window row is one 8- or 16-byte load, a wave reads
// 64 of them back to back, every byte of x once; NT: with non-temporal loads (read-once operand
// beyond the memory-side cache, the streaming policy of the copy kernel).
template <typename T, typename I, int WV, bool NT, bool ISMAX>
__global__ __launch_bounds__(256) void pool_fwd_kernel(PoolArgs a) {
  const T* __restrict__ x = static_cast<const T*>(a.x);
  T* __restrict__ z = static_cast<T*>(a.out);
  const I total = (I)a.total, step = (I)gridDim.x * 256;
  for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const Pos P = locate<I>(a, i, a.O);
    int st[3], en[3];
    int64_t size = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int b = P.c[k] * a.s[k];
      st[k] = max(b - a.p[k], 0);
      en[k] = min(b + a.w[k] - a.p[k], a.X[k]);
      size *= a.mode == POOL_AVG_INC ? min(b + a.w[k], a.X[k] + 2 * a.p[k]) - b : en[k] - st[k];
    }
    const T* xb = x + P.xbase;
    T acc = ISMAX ? xb[st[0] * a.xs[0] + st[1] * a.xs[1] + st[2] * a.xs[2]] : (T)0;
    for (int d = st[0]; d < en[0]; ++d) {
      for (int h = st[1]; h < en[1]; ++h) {
        const T* row = xb + d * a.xs[0] + h * a.xs[1];
        if constexpr (WV > 0) {
          if (en[2] - st[2] == WV) {
            typedef T vec_t __attribute__((ext_vector_type(WV)));
            const vec_t* src = reinterpret_cast<const vec_t*>(row + st[2]);
            const vec_t v = NT ? __builtin_nontemporal_load(src) : *src;
#pragma unroll
            for (int e = 0; e < WV; ++e) acc = ISMAX ? nan_max(acc, v[e]) : acc + v[e];
            continue;
          }
        }
        for (int c = st[2]; c < en[2]; ++c) {
          const T v = row[c * a.xs[2]];
          acc = ISMAX ? nan_max(acc, v) : acc + v;
        }
      }
    }
    if (a.mode >= POOL_AVG_INC) acc = acc / (T)size;
    z[i] = acc;
  }
}

__device__ __forceinline__ int64_t lead_offset(const PoolArgs& a, int64_t lead) {
  if (a.nlead <= 1) return lead * a.xl[2];
  const int64_t u = lead / a.L[2], l2 = lead - u * a.L[2];
  const int64_t l0 = u / a.L[1], l1 = u - l0 * a.L[1];
  return l0 * a.xl[0] + l1 * a.xl[1] + l2 * a.xl[2];
}

// Forward, the usual CNN layer: a 2-d pool whose windows (WH rows of WV columns) tile the image
// exactly (stride == window, no padding, no partial window) over aligned unit-stride rows.  A lane
// takes 16 bytes of each of its WH rows — NOUT = 16 / (WV * sizeof(T)) neighbouring windows — with
// all loads issued before the first use, and stores its NOUT results side by side: four times the
// bytes in flight per lane of the general kernel, a quarter of its index arithmetic per byte.  The
// values meet in the general kernel's order (row-major per window): the same bits.
template <typename T, int WV, int WH, bool NT, bool ISMAX>
__global__ __launch_bounds__(256) void pool_fwd_tile_kernel(PoolArgs a) {
  constexpr int LV = 16 / sizeof(T), NOUT = LV / WV;
  typedef T vec_t __attribute__((ext_vector_type(LV)));
  const T* __restrict__ x = static_cast<const T*>(a.x);
  T* __restrict__ z = static_cast<T*>(a.out);
  const uint32_t per_row = (uint32_t)a.O[2] / NOUT;
  const uint32_t groups = (uint32_t)(a.total / NOUT), step = gridDim.x * 256u;
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < groups; g += step) {
    const uint32_t q = g / per_row, og = g - q * per_row;
    const uint32_t lead = q / (uint32_t)a.O[1], oh = q - lead * (uint32_t)a.O[1];
    const T* row = x + lead_offset(a, lead) + (int64_t)(oh * WH) * a.xs[1] + og * LV;
    vec_t v[WH];
#pragma unroll
    for (int r = 0; r < WH; ++r) {
      const vec_t* src = reinterpret_cast<const vec_t*>(row + r * a.xs[1]);
      v[r] = NT ? __builtin_nontemporal_load(src) : *src;
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      T acc = ISMAX ? v[0][o * WV] : (T)0;
#pragma unroll
      for (int r = 0; r < WH; ++r)
#pragma unroll
        for (int e = 0; e < WV; ++e) acc = ISMAX ? nan_max(acc, v[r][o * WV + e]) : acc + v[r][o * WV + e];
      if (a.mode >= POOL_AVG_INC) acc = acc / (T)(int64_t)(WV * WH);
      z[(int64_t)g * NOUT + o] = acc;
    }
  }
}

// Both gradients where no two windows overlap (stride >= window in every dimension): a cell lies
// in at most one window, so there is nothing to loop over.  A lane takes 16 bytes of cells of one
// image row; the loads of all of them are issued together.  Same sums as pool_grad_kernel (0 + the
// one term), hence the same bits.  XV: x is read with one 16-byte load.
template <typename T, bool MAXG, bool XV>
__global__ __launch_bounds__(256) void pool_grad_disjoint_kernel(PoolArgs a) {
  constexpr int VC = 16 / sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(VC)));
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ mo = static_cast<const T*>(a.m);
  const T* __restrict__ gz = static_cast<const T*>(a.g);
  T* __restrict__ gx = static_cast<T*>(a.out);
  const uint32_t per_row = (uint32_t)a.X[2] / VC;
  const uint32_t groups = (uint32_t)(a.total / VC), step = gridDim.x * 256u;
  for (uint32_t g = blockIdx.x * 256u + threadIdx.x; g < groups; g += step) {
    uint32_t q = g / per_row;
    const int c2 = (int)(g - q * per_row) * VC;
    uint32_t q1 = q / (uint32_t)a.X[1];
    const int c1 = (int)(q - q1 * (uint32_t)a.X[1]);
    int c0 = 0;
    if (a.X[0] != 1) {
      q = q1 / (uint32_t)a.X[0];
      c0 = (int)(q1 - q * (uint32_t)a.X[0]);
      q1 = q;
    }
    const int64_t lead = q1;
    const int pc0 = c0 + a.p[0], pc1 = c1 + a.p[1];
    const int j0 = pc0 / a.s[0], j1 = pc1 / a.s[1];
    const bool ok01 = j0 < a.O[0] && pc0 - j0 * a.s[0] < a.w[0] && j1 < a.O[1] && pc1 - j1 * a.s[1] < a.w[1];
    const int64_t rb = (lead * a.O[0] + j0) * ((int64_t)a.O[1] * a.O[2]) + (int64_t)j1 * a.O[2];
    int64_t size01 = 1;
    if (!MAXG && a.mode != POOL_SUM) {
      const int j[2] = {j0, j1};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int b = j[k] * a.s[k];
        size01 *= a.mode == POOL_AVG_INC ? min(b + a.w[k], a.X[k] + 2 * a.p[k]) - b
                                         : min(b + a.w[k] - a.p[k], a.X[k]) - max(b - a.p[k], 0);
      }
    }
    T xv[VC];
    if constexpr (MAXG) {
      const T* xp = x + lead_offset(a, lead) + c0 * a.xs[0] + c1 * a.xs[1] + c2 * a.xs[2];
      if constexpr (XV) {
        const vec_t v = *reinterpret_cast<const vec_t*>(xp);
#pragma unroll
        for (int e = 0; e < VC; ++e) xv[e] = v[e];
      } else {
#pragma unroll
        for (int e = 0; e < VC; ++e) xv[e] = xp[e * a.xs[2]];
      }
    }
    vec_t res;
#pragma unroll
    for (int e = 0; e < VC; ++e) {
      const int pc2 = c2 + e + a.p[2], j2 = pc2 / a.s[2];
      const bool ok = ok01 && j2 < a.O[2] && pc2 - j2 * a.s[2] < a.w[2];
      // unconditional loads (element 0 where the cell lies under no window: the launcher sends
      // empty outputs elsewhere), so that all of a lane's loads are in flight together
      const int64_t at = ok ? rb + j2 : 0;
      T v = gz[at];
      bool take = ok;
      if constexpr (MAXG) {
        take = ok && mo[at] == xv[e];
      } else if (a.mode != POOL_SUM) {
        const int b = ok ? j2 * a.s[2] : 0;
        const int64_t size2 = a.mode == POOL_AVG_INC
                                  ? min(b + a.w[2], a.X[2] + 2 * a.p[2]) - b
                                  : min(b + a.w[2] - a.p[2], a.X[2]) - max(b - a.p[2], 0);
        v = v / (T)(ok ? size01 * size2 : 1);
      }
      res[e] = take ? (T)0 + v : (T)0;
    }
    *reinterpret_cast<vec_t*>(gx + (int64_t)g * VC) = res;
  }
}

// ggz[r] = sum of ggx[c] over the cells c of window r with x[c] == maxout[r]
// (DownsampleFactorMaxGradGrad.c_code :2066-2122)
template <typename T, typename I>
__global__ __launch_bounds__(256) void maxpool_gradgrad_kernel(PoolArgs a) {
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ mo = static_cast<const T*>(a.m);
  const T* __restrict__ ggx = static_cast<const T*>(a.g);
  T* __restrict__ z = static_cast<T*>(a.out);
  const I total = (I)a.total, step = (I)gridDim.x * 256;
  for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const Pos P = locate<I>(a, i, a.O);
    int st[3], en[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int b = P.c[k] * a.s[k];
      st[k] = max(b - a.p[k], 0);
      en[k] = min(b + a.w[k] - a.p[k], a.X[k]);
    }
    const T* xb = x + P.xbase;
    const T* gb = ggx + P.lead * ((int64_t)a.X[0] * a.X[1] * a.X[2]);
    const T top = mo[i];
    T acc = (T)0;
    for (int d = st[0]; d < en[0]; ++d)
      for (int h = st[1]; h < en[1]; ++h)
        for (int c = st[2]; c < en[2]; ++c)
          if (xb[d * a.xs[0] + h * a.xs[1] + c * a.xs[2]] == top)
            acc += gb[((int64_t)d * a.X[1] + h) * a.X[2] + c];
    z[i] = acc;
  }
}

// Both gradients: MAXG — gx[c] = sum of gz[r] over the windows r that hold c and have
// maxout[r] == x[c] (MaxPoolGrad.c_code :1413-1469); else gx[c] = sum of gz[r] / size(r), `sum`
// without the division (AveragePoolGrad.c_code :1751-1813: the quotient is formed per window, then
// added).
template <typename T, typename I, bool MAXG>
__global__ __launch_bounds__(256) void pool_grad_kernel(PoolArgs a) {
  const T* __restrict__ x = static_cast<const T*>(a.x);
  const T* __restrict__ mo = static_cast<const T*>(a.m);
  const T* __restrict__ gz = static_cast<const T*>(a.g);
  T* __restrict__ gx = static_cast<T*>(a.out);
  const I total = (I)a.total, step = (I)gridDim.x * 256;
  for (I i = (I)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const Pos P = locate<I>(a, i, a.X);
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int pc = P.c[k] + a.p[k], t = pc - a.w[k] + 1;
      lo[k] = t <= 0 ? 0 : (t + a.s[k] - 1) / a.s[k];
      hi[k] = min(pc / a.s[k], a.O[k] - 1);
    }
    T xv = (T)0;
    if constexpr (MAXG) xv = x[P.xbase + P.c[0] * a.xs[0] + P.c[1] * a.xs[1] + P.c[2] * a.xs[2]];
    const int64_t ob = P.lead * ((int64_t)a.O[0] * a.O[1] * a.O[2]);
    T acc = (T)0;
    for (int jd = lo[0]; jd <= hi[0]; ++jd) {
      for (int jh = lo[1]; jh <= hi[1]; ++jh) {
        const int64_t rb = ob + ((int64_t)jd * a.O[1] + jh) * a.O[2];
        for (int jw = lo[2]; jw <= hi[2]; ++jw) {
          if constexpr (MAXG) {
            if (mo[rb + jw] == xv) acc += gz[rb + jw];
          } else {
            T v = gz[rb + jw];
            if (a.mode != POOL_SUM) {
              const int j[3] = {jd, jh, jw};
              int64_t size = 1;
#pragma unroll
              for (int k = 0; k < 3; ++k) {
                const int b = j[k] * a.s[k];
                size *= a.mode == POOL_AVG_INC
                            ? min(b + a.w[k], a.X[k] + 2 * a.p[k]) - b
                            : min(b + a.w[k] - a.p[k], a.X[k]) - max(b - a.p[k], 0);
              }
              v = v / (T)size;
            }
            acc += v;
          }
        }
      }
    }
    gx[i] = acc;
  }
}

unsigned lane_grid(int64_t total) {
  int64_t cap = (int64_t)ahip_cu_count() * 8;   // copy.hip's stream grid: 8 workgroups per CU
  if (cap < 1) cap = 1;
  const int64_t want = (total + 255) / 256;
  return (unsigned)(want < cap ? want : cap);
}

// geo = lead[3], X[3], O[3], ws[3], stride[3], pad[3].  Everything a kernel relies on to stay in
// bounds is checked here, whatever the caller computed.
int fill_args(PoolArgs& a, const int64_t* geo, const int64_t* x_strides) {
  AHIP_REQUIRE(geo != nullptr, "null geometry");
  memset(&a, 0, sizeof(a));
  const int64_t lim = 1LL << 30;
  int64_t planeX = 1, planeO = 1, lead = 1;
  a.nlead = 0;
  for (int k = 0; k < 3; ++k) {
    const int64_t L = geo[k], X = geo[3 + k], O = geo[6 + k], w = geo[9 + k], s = geo[12 + k],
                  p = geo[15 + k];
    AHIP_REQUIRE(L >= 0 && X >= 0 && O >= 0, "pool: negative extent");
    AHIP_REQUIRE(w >= 1 && s >= 1, "pool: window and stride must be positive");
    AHIP_REQUIRE(p >= 0 && p < w, "pool: padding must be non-negative and smaller than the window");
    AHIP_REQUIRE(X < lim && O < lim && w < lim && s < lim && O * s < lim && X + 2 * p + w < lim,
                 "pool: pooled extent, window or stride too large (2^30)");
    // every window holds at least one cell of the image
    AHIP_REQUIRE(O == 0 || (X > 0 && (O - 1) * s - p < X), "pool: output extent %lld of dimension %d has a "
                 "window outside the image", (long long)O, k);
    a.L[k] = L; a.X[k] = (int)X; a.O[k] = (int)O; a.w[k] = (int)w; a.s[k] = (int)s; a.p[k] = (int)p;
    planeX *= X; planeO *= O; lead *= L;
    AHIP_REQUIRE(planeX < lim && planeO < lim, "pool: pooled plane too large (2^30 elements)");
    if (L != 1) ++a.nlead;
    if (x_strides) { a.xl[k] = x_strides[k]; a.xs[k] = x_strides[3 + k]; }
  }
  if (a.L[0] != 1 || a.L[1] != 1) a.nlead = 2;     // the decomposition of the leading index is needed
  AHIP_REQUIRE(lead < (1LL << 62) / lim, "pool: too many elements");
  return AHIP_OK;
}

int64_t elements(const PoolArgs& a, const int* D) {
  return a.L[0] * a.L[1] * a.L[2] * D[0] * D[1] * D[2];
}

bool small(const PoolArgs& a) {   // every flat index (and the stride of the loop on top) fits 32 bits
  const int64_t lim = 1LL << 31;
  return elements(a, a.X) < lim && elements(a, a.O) < lim;
}

bool float_dtype(int dtype) { return dtype == AHIP_F32 || dtype == AHIP_F64; }

template <typename T, int WV, bool ISMAX>
int launch_fwd_wv(PoolArgs& a, bool nt, hipStream_t s) {
  const unsigned grid = lane_grid(a.total);
  if (small(a)) {
    if (WV > 0 && nt) AHIP_LAUNCH((pool_fwd_kernel<T, uint32_t, WV, (WV > 0), ISMAX>), dim3(grid), dim3(256), 0, s, a);
    else AHIP_LAUNCH((pool_fwd_kernel<T, uint32_t, WV, false, ISMAX>), dim3(grid), dim3(256), 0, s, a);
  } else {
    if (WV > 0 && nt) AHIP_LAUNCH((pool_fwd_kernel<T, uint64_t, WV, (WV > 0), ISMAX>), dim3(grid), dim3(256), 0, s, a);
    else AHIP_LAUNCH((pool_fwd_kernel<T, uint64_t, WV, false, ISMAX>), dim3(grid), dim3(256), 0, s, a);
  }
  return AHIP_OK;
}

// x's rows have unit stride and x and every row start lie on a multiple of n elements
template <typename T>
bool rows_aligned(const PoolArgs& a, int n) {
  if (a.xs[2] != 1 || reinterpret_cast<uintptr_t>(a.x) % (n * sizeof(T)) != 0) return false;
  for (int k = 0; k < 3; ++k) {
    if (a.L[k] > 1 && a.xl[k] % n != 0) return false;
    if (k < 2 && a.X[k] > 1 && a.xs[k] % n != 0) return false;
  }
  return true;
}

template <typename T, int WV, bool ISMAX>
int launch_fwd_tile(PoolArgs& a, bool nt, hipStream_t s) {
  constexpr int NOUT = 16 / (int)sizeof(T) / WV;
  const unsigned grid = lane_grid(a.total / NOUT);
#define AHIP_POOL_TILE(WH)                                                                                   \
  if (nt) AHIP_LAUNCH((pool_fwd_tile_kernel<T, WV, WH, true, ISMAX>), dim3(grid), dim3(256), 0, s, a);     \
  else AHIP_LAUNCH((pool_fwd_tile_kernel<T, WV, WH, false, ISMAX>), dim3(grid), dim3(256), 0, s, a);       \
  return AHIP_OK;
  switch (a.w[1]) {
    case 1: AHIP_POOL_TILE(1)
    case 2: AHIP_POOL_TILE(2)
    default: AHIP_POOL_TILE(4)
  }
#undef AHIP_POOL_TILE
}

template <typename T, bool ISMAX>
int launch_fwd(PoolArgs& a, bool nt, hipStream_t s) {
  const int wv = a.w[2];
  constexpr int LV = 16 / (int)sizeof(T);
  // windows that tile a 2-d image exactly: see pool_fwd_tile_kernel
  const bool tile = small(a) && a.X[0] == 1 && a.w[0] == 1 && a.s[0] == 1 && a.p[0] == 0 && a.p[1] == 0 &&
                    a.p[2] == 0 && a.s[1] == a.w[1] && a.s[2] == wv && (a.w[1] == 1 || a.w[1] == 2 || a.w[1] == 4) &&
                    (wv == 2 || wv == 4) && wv <= LV && a.X[2] % LV == 0 && a.O[2] * wv == a.X[2] &&
                    a.O[1] * a.w[1] == a.X[1] && rows_aligned<T>(a, LV);
  if (tile && wv == 2) return launch_fwd_tile<T, 2, ISMAX>(a, nt, s);
  if constexpr (sizeof(T) == 4)
    if (tile && wv == 4) return launch_fwd_tile<T, 4, ISMAX>(a, nt, s);
  // a window row as one load: see pool_fwd_kernel
  const bool wide = a.s[2] == wv && a.p[2] == 0 && (wv == 2 || wv == 4) && wv <= LV && rows_aligned<T>(a, wv);
  if (wide && wv == 2) return launch_fwd_wv<T, 2, ISMAX>(a, nt, s);
  if constexpr (sizeof(T) == 4)
    if (wide && wv == 4) return launch_fwd_wv<T, 4, ISMAX>(a, nt, s);
  return launch_fwd_wv<T, 0, ISMAX>(a, false, s);
}

template <typename T, bool MAXG>
int launch_grad(PoolArgs& a, hipStream_t s) {
  constexpr int VC = 16 / (int)sizeof(T);
  // no two windows overlap: see pool_grad_disjoint_kernel
  if (small(a) && elements(a, a.O) > 0 && a.s[0] >= a.w[0] && a.s[1] >= a.w[1] && a.s[2] >= a.w[2] && a.X[2] % VC == 0 &&
      reinterpret_cast<uintptr_t>(a.out) % 16 == 0) {
    const unsigned grid = lane_grid(a.total / VC);
    if (MAXG && rows_aligned<T>(a, VC))
      AHIP_LAUNCH((pool_grad_disjoint_kernel<T, MAXG, MAXG>), dim3(grid), dim3(256), 0, s, a);
    else
      AHIP_LAUNCH((pool_grad_disjoint_kernel<T, MAXG, false>), dim3(grid), dim3(256), 0, s, a);
    return AHIP_OK;
  }
  const unsigned grid = lane_grid(a.total);
  if (small(a)) AHIP_LAUNCH((pool_grad_kernel<T, uint32_t, MAXG>), dim3(grid), dim3(256), 0, s, a);
  else AHIP_LAUNCH((pool_grad_kernel<T, uint64_t, MAXG>), dim3(grid), dim3(256), 0, s, a);
  return AHIP_OK;
}

template <typename T>
int launch_gradgrad(PoolArgs& a, hipStream_t s) {
  const unsigned grid = lane_grid(a.total);
  if (small(a)) AHIP_LAUNCH((maxpool_gradgrad_kernel<T, uint32_t>), dim3(grid), dim3(256), 0, s, a);
  else AHIP_LAUNCH((maxpool_gradgrad_kernel<T, uint64_t>), dim3(grid), dim3(256), 0, s, a);
  return AHIP_OK;
}

}  // namespace

extern "C" {

int ahip_pool_fwd(int dtype, int mode, int streaming, const int64_t* geo, const void* x,
                  const int64_t* x_strides, void* z, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "pool: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(mode >= POOL_MAX && mode <= POOL_AVG_EXC, "pool: unknown mode %d", mode);
  AHIP_REQUIRE(x_strides != nullptr, "null strides");
  PoolArgs a;
  int rc = fill_args(a, geo, x_strides);
  if (rc) return rc;
  a.total = elements(a, a.O);
  if (a.total == 0) return AHIP_OK;
  AHIP_REQUIRE(x != nullptr && z != nullptr, "null pointer");
  a.x = x; a.out = z; a.mode = mode;
  hipStream_t s = as_stream(stream);
  const bool nt = streaming != 0;
  if (dtype == AHIP_F32)
    return mode == POOL_MAX ? launch_fwd<float, true>(a, nt, s) : launch_fwd<float, false>(a, nt, s);
  return mode == POOL_MAX ? launch_fwd<double, true>(a, nt, s) : launch_fwd<double, false>(a, nt, s);
}

int ahip_maxpool_grad(int dtype, const int64_t* geo, const void* x, const int64_t* x_strides,
                      const void* maxout, const void* gz, void* gx, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "pool: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(x_strides != nullptr, "null strides");
  PoolArgs a;
  int rc = fill_args(a, geo, x_strides);
  if (rc) return rc;
  a.total = elements(a, a.X);
  if (a.total == 0) return AHIP_OK;
  AHIP_REQUIRE(x != nullptr && gx != nullptr && ((maxout != nullptr && gz != nullptr) ||
               elements(a, a.O) == 0), "null pointer");
  a.x = x; a.m = maxout; a.g = gz; a.out = gx; a.mode = POOL_MAX;
  hipStream_t s = as_stream(stream);
  return dtype == AHIP_F32 ? launch_grad<float, true>(a, s) : launch_grad<double, true>(a, s);
}

int ahip_avgpool_grad(int dtype, int mode, const int64_t* geo, const void* gz, void* gx,
                      void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "pool: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(mode >= POOL_SUM && mode <= POOL_AVG_EXC, "pool: mode %d has no average gradient", mode);
  PoolArgs a;
  int rc = fill_args(a, geo, nullptr);
  if (rc) return rc;
  a.total = elements(a, a.X);
  if (a.total == 0) return AHIP_OK;
  AHIP_REQUIRE(gx != nullptr && (gz != nullptr || elements(a, a.O) == 0), "null pointer");
  a.g = gz; a.out = gx; a.mode = mode;
  hipStream_t s = as_stream(stream);
  return dtype == AHIP_F32 ? launch_grad<float, false>(a, s) : launch_grad<double, false>(a, s);
}

int ahip_maxpool_gradgrad(int dtype, const int64_t* geo, const void* x, const int64_t* x_strides,
                          const void* maxout, const void* ggx, void* ggz, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "pool: float32 / float64 only, got dtype %d", dtype);
  AHIP_REQUIRE(x_strides != nullptr, "null strides");
  PoolArgs a;
  int rc = fill_args(a, geo, x_strides);
  if (rc) return rc;
  a.total = elements(a, a.O);
  if (a.total == 0) return AHIP_OK;
  AHIP_REQUIRE(x != nullptr && maxout != nullptr && ggx != nullptr && ggz != nullptr, "null pointer");
  a.x = x; a.m = maxout; a.g = ggx; a.out = ggz; a.mode = POOL_MAX;
  hipStream_t s = as_stream(stream);
  return dtype == AHIP_F32 ? launch_gradgrad<float>(a, s) : launch_gradgrad<double>(a, s);
}

}  // extern "C"
