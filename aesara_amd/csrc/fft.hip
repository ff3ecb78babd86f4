// K14 — batched one-axis Fourier transforms: real -> complex, complex <-> complex, complex -> real.
//
// Replaces tensor/fft.py:39 RFFTOp.perform (np.fft.rfftn) and :100 IRFFTOp.perform (np.fft.irfftn,
// with NumPy's 1/prod(s) multiplied back out): the executor runs one of these passes per transformed
// axis.  Complex values are interleaved (re, im) pairs of the real dtype (float32 / float64).
//
// A problem is [outer, n, inner] with element strides (in real scalars) for input and output; the
// `valid` leading entries of the input axis are read, the rest of the length-n transform is zero.
// One workgroup of 256 threads holds R = max(1, 1024 / m) transforms of m points in LDS (m = n for
// a power of two), so every element is read from HBM once and written once per axis pass:
//   * schedule: Stockham self-sorting decimation in frequency, radix-4 passes and one closing
//     radix-2 pass when log2 m is odd.  A pass reads its butterflies into registers, meets at a
//     barrier and writes them back in the sorted order, so one LDS image (not two) is enough;
//   * LDS layout: complex slot i lives at i + (i >> 5) (float32) / i + (i >> 4) (float64): one
//     slot of padding per 256-byte bank row, which spreads the power-of-two strides of the passes
//     over the banks;
//   * twiddles exp(-2 pi i t / m) come from a table in the caller's workspace, generated in float64
//     with sincospi of an exactly representable argument and rounded once to the working type;
//   * the inverse is conj(forward(conj(.))): the conjugations ride on the loads and stores.
// Real input is widened to complex in LDS only (no complex copy in HBM) and only bins 0 .. n/2 are
// written; complex -> real rebuilds the Hermitian half in LDS, ignoring Im of bin 0 and, for even
// n, of bin n/2 like np.fft.irfft.
// Every other n: Bluestein over the same transform, m = next_pow2(2n - 1): x[k] w[k] is convolved
// with conj(w) (w[k] = exp(-i pi k^2 / n), the angle reduced EXACTLY as (k^2 mod 2n) / n in integer
// arithmetic), i.e. three m-point transforms, one of them (the chirp's spectrum, scaled by 1/m)
// done once per call by a one-workgroup kernel into the workspace.
// Limits: powers of two up to 4096, other lengths up to 2048 (m = 4096): the float64 image of 4096
// points is 68 KiB of the 160 KiB LDS.  Longer axes need a four-step pass through HBM: AHIP_ENOSUP.
#include "common.h"

namespace {

constexpr int FFT_THREADS = 256;
constexpr int FFT_MAX_POW2 = 4096;
constexpr int FFT_MAX_OTHER = 2048;
constexpr int FFT_WG_SLOTS = 1024;    // a workgroup holds at least this many points (R short rows)

template <typename T> struct alignas(2 * sizeof(T)) Cx { T re, im; };
template <typename T> struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };

template <typename T> __device__ __forceinline__ Cx<T> cadd(Cx<T> a, Cx<T> b) { return {a.re + b.re, a.im + b.im}; }
template <typename T> __device__ __forceinline__ Cx<T> csub(Cx<T> a, Cx<T> b) { return {a.re - b.re, a.im - b.im}; }
template <typename T> __device__ __forceinline__ Cx<T> cmul(Cx<T> a, Cx<T> b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T> __device__ __forceinline__ Cx<T> conj_(Cx<T> a) { return {a.re, -a.im}; }
// LDS slot of complex element i (one slot of padding per 256-byte bank row)
template <typename T> __device__ __forceinline__ int pad(int i) { return i + (i >> (sizeof(T) == 4 ? 5 : 4)); }
template <typename T> constexpr size_t lds_bytes(int slots) {
  return (size_t)(slots + (slots >> (sizeof(T) == 4 ? 5 : 4)) + 1) * sizeof(Cx<T>);
}

struct FftArgs {
  const void* x; void* out;
  const void* W; const void* chirp; const void* bhat;    // tables in the workspace
  int64_t rows, inner, valid;                            // rows = outer * inner
  int64_t xso, xsn, xsi, oso, osn, osi;
  int n, m, logm, logR, inverse;
  int icx, ocx;     // complex input / output pairs are aligned to 2 * sizeof(T): one access per pair
  int ivec, ovec;   // 16-byte row forms (R == 1, inner == 1, unit stride along the axis)
};
AHIP_PTRS_BEGIN(FftArgs) AHIP_PTR1(x) AHIP_PTR1(out) AHIP_PTR1(W) AHIP_PTR1(chirp) AHIP_PTR1(bhat) AHIP_PTRS_END

struct TabArgs {
  void* W; void* chirp; void* bhat;
  int n, m, logm, blue;
};
AHIP_PTRS_BEGIN(TabArgs) AHIP_PTR1(W) AHIP_PTR1(chirp) AHIP_PTR1(bhat) AHIP_PTRS_END

// Forward transform of every length-m row of the `slots`-point LDS image (slots = R * m), in place.
// The caller has synchronised after filling the image; returns synchronised.
template <typename T, int ITER>
__device__ __forceinline__ void fft_lds(Cx<T>* lds, int slots, int m, int logm,
                                        const Cx<T>* __restrict__ W, int tid) {
  const int q4 = m >> 2, nb4 = slots >> 2;
  int logs = 0;
  for (int nn = m; nn >= 4; nn >>= 2, logs += 2) {
    Cx<T> v[ITER][4];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int B = tid + it * FFT_THREADS;
      if (B < nb4) {
        const int base = ((B >> (logm - 2)) << logm) + (B & (q4 - 1));
#pragma unroll
        for (int k = 0; k < 4; ++k) v[it][k] = lds[pad<T>(base + k * q4)];
      }
    }
    __syncthreads();
    const int s = 1 << logs;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int B = tid + it * FFT_THREADS;
      if (B < nb4) {
        const int b = B & (q4 - 1), q = b & (s - 1), t = b - q;     // t = p * s: twiddle index
        const int o = ((B >> (logm - 2)) << logm) + 4 * b - 3 * q;
        const Cx<T> apc = cadd(v[it][0], v[it][2]), amc = csub(v[it][0], v[it][2]);
        const Cx<T> bpd = cadd(v[it][1], v[it][3]), bmd = csub(v[it][1], v[it][3]);
        const Cx<T> jbmd = {-bmd.im, bmd.re};
        Cx<T> y1 = csub(amc, jbmd), y2 = csub(apc, bpd), y3 = cadd(amc, jbmd);
        if (t) {
          y1 = cmul(y1, W[t]);
          y2 = cmul(y2, W[2 * t]);
          y3 = cmul(y3, W[3 * t]);
        }
        lds[pad<T>(o)] = cadd(apc, bpd);
        lds[pad<T>(o + s)] = y1;
        lds[pad<T>(o + 2 * s)] = y2;
        lds[pad<T>(o + 3 * s)] = y3;
      }
    }
    __syncthreads();
  }
  if (logm & 1) {       // closing radix-2 pass (stride m / 2, no twiddles): every pair stays in place
    const int h = m >> 1, nb2 = slots >> 1;
    for (int B = tid; B < nb2; B += FFT_THREADS) {
      const int i0 = ((B >> (logm - 1)) << logm) + (B & (h - 1));
      const Cx<T> a = lds[pad<T>(i0)], b = lds[pad<T>(i0 + h)];
      lds[pad<T>(i0)] = cadd(a, b);
      lds[pad<T>(i0 + h)] = csub(a, b);
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(FFT_THREADS) void fft_tables_kernel(TabArgs t) {
  Cx<T>* W = static_cast<Cx<T>*>(t.W);
  Cx<T>* chirp = static_cast<Cx<T>*>(t.chirp);
  const int i = blockIdx.x * FFT_THREADS + threadIdx.x;
  double s, c;
  if (i < t.m) {
    sincospi(2.0 * (double)i / (double)t.m, &s, &c);        // the argument is exact (m = 2^k)
    W[i] = {(T)c, (T)-s};
  }
  if (t.blue && i < t.n) {
    const int64_t q = ((int64_t)i * i) % (2 * (int64_t)t.n);  // k^2 mod 2n: the angle never grows
    sincospi((double)q / (double)t.n, &s, &c);
    chirp[i] = {(T)c, (T)-s};
  }
}

// spectrum of the Bluestein kernel conj(w) laid out circularly on m points, scaled by 1/m
template <typename T, int ITER>
__global__ __launch_bounds__(FFT_THREADS) void fft_bhat_kernel(TabArgs t) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cx<T>* lds = reinterpret_cast<Cx<T>*>(smem);
  const Cx<T>* W = static_cast<const Cx<T>*>(t.W);
  const Cx<T>* chirp = static_cast<const Cx<T>*>(t.chirp);
  Cx<T>* bhat = static_cast<Cx<T>*>(t.bhat);
  const int tid = threadIdx.x, n = t.n, m = t.m;
  for (int e = tid; e < m; e += FFT_THREADS) lds[pad<T>(e)] = {(T)0, (T)0};
  __syncthreads();
  for (int k = tid; k < n; k += FFT_THREADS) {     // m >= 2n - 1: k and m - k never meet
    const Cx<T> c = conj_(chirp[k]);
    lds[pad<T>(k)] = c;
    if (k) lds[pad<T>(m - k)] = c;
  }
  __syncthreads();
  fft_lds<T, ITER>(lds, m, m, t.logm, W, tid);
  const T sc = (T)1 / (T)m;
  for (int e = tid; e < m; e += FFT_THREADS) {
    const Cx<T> z = lds[pad<T>(e)];
    bhat[e] = {z.re * sc, z.im * sc};
  }
}

// MODE 0: real -> complex (bins 0 .. n/2), 1: complex -> complex, 2: complex (bins 0 .. n/2) -> real
template <typename T, int ITER, int MODE, bool BLUE>
__global__ __launch_bounds__(FFT_THREADS) void fft_kernel(FftArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  Cx<T>* lds = reinterpret_cast<Cx<T>*>(smem);
  const T* __restrict__ x = static_cast<const T*>(a.x);
  T* __restrict__ out = static_cast<T*>(a.out);
  const Cx<T>* __restrict__ W = static_cast<const Cx<T>*>(a.W);
  const Cx<T>* __restrict__ chirp = static_cast<const Cx<T>*>(a.chirp);
  const Cx<T>* __restrict__ bhat = static_cast<const Cx<T>*>(a.bhat);
  const int tid = threadIdx.x;
  const int n = a.n, m = a.m, logm = a.logm, logR = a.logR, R = 1 << logR, slots = m << logR;
  const int half = n >> 1;
  const int nin = MODE == 2 ? half + 1 : n;        // input entries a transform can use
  const int nout = MODE == 0 ? half + 1 : n;       // output entries it writes
  const int nval = a.valid < nin ? (int)a.valid : nin;
  const bool rowfast = a.inner > 1;                // adjacent lanes on adjacent rows (unit stride there)
  const int64_t ngroups = (a.rows + R - 1) >> logR;
  const Cx<T> zero = {(T)0, (T)0};

  // entry k (raw value v, zero past the valid input) of row slot r goes into the LDS image
  auto put = [&](int r, int k, Cx<T> v) {
    const int base = r << logm;
    if (MODE == 2) {
      if (k <= half) {
        const bool edge = k == 0 || 2 * k == n;    // DC / Nyquist: the imaginary part is ignored
        if (edge) v.im = (T)0;
        Cx<T> lo = conj_(v), hi = v;               // conj(X[k]) at k, conj(X[n - k]) = X[k] at n - k
        if (BLUE) {
          lo = cmul(lo, chirp[k]);
          if (!edge) hi = cmul(hi, chirp[n - k]);
        }
        lds[pad<T>(base + k)] = lo;
        if (!edge) lds[pad<T>(base + n - k)] = hi;
      } else if (k >= n) {
        lds[pad<T>(base + k)] = zero;
      }
    } else {
      if (k >= n) v = zero;
      else {
        if (MODE == 1 && a.inverse) v = conj_(v);
        if (BLUE) v = cmul(v, chirp[k]);
      }
      lds[pad<T>(base + k)] = v;
    }
  };
  // transformed entry k of row slot r
  auto get = [&](int r, int k) -> Cx<T> {
    Cx<T> y = lds[pad<T>((r << logm) + k)];
    if (BLUE) y = cmul(conj_(y), chirp[k]);
    if (MODE == 1 && a.inverse) y = conj_(y);
    return y;
  };

  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t l0 = g << logR;
    // ------------------------------------------------------------------ load ----------
    if (a.ivec) {                                   // R == 1, inner == 1, unit stride, aligned rows
      const T* px = x + l0 * a.xso;
      if (MODE == 0) {
        constexpr int V = 16 / (int)sizeof(T);
        for (int k0 = tid * V; k0 < m; k0 += FFT_THREADS * V) {
          if (k0 + V <= nval) {
            const Vec16<T> p = *reinterpret_cast<const Vec16<T>*>(px + k0);
#pragma unroll
            for (int e = 0; e < V; ++e) put(0, k0 + e, Cx<T>{p.v[e], (T)0});
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const int k = k0 + e;
              put(0, k, k < nval ? Cx<T>{px[k], (T)0} : zero);
            }
          }
        }
      } else if constexpr (sizeof(T) == 4) {        // float32 pairs: two complex values per lane
        const int h = (int)((reinterpret_cast<uintptr_t>(px) >> 3) & 1);   // row starts mid-vector
        if (tid == 0 && h) put(0, 0, nval > 0 ? *reinterpret_cast<const Cx<T>*>(px) : zero);
        for (int k0 = h + 2 * tid; k0 < m; k0 += 2 * FFT_THREADS) {
          if (k0 + 2 <= nval) {
            const Vec16<T> p = *reinterpret_cast<const Vec16<T>*>(px + 2 * (int64_t)k0);
            put(0, k0, Cx<T>{p.v[0], p.v[1]});
            put(0, k0 + 1, Cx<T>{p.v[2], p.v[3]});
          } else {
            for (int k = k0; k < k0 + 2 && k < m; ++k)
              put(0, k, k < nval ? *reinterpret_cast<const Cx<T>*>(px + 2 * (int64_t)k) : zero);
          }
        }
      }
    } else {
      for (int e = tid; e < slots; e += FFT_THREADS) {
        const int r = rowfast ? (e & (R - 1)) : (e >> logm);
        const int k = rowfast ? (e >> logR) : (e & (m - 1));
        if (MODE == 2 && k > half && k < n) continue;       // written by its mirror
        const int64_t l = l0 + r;
        Cx<T> v = zero;
        if (k < nval && l < a.rows) {
          const int64_t o = rowfast ? l / a.inner : l, i = rowfast ? l - o * a.inner : 0;
          const T* p = x + o * a.xso + i * a.xsi + (int64_t)k * a.xsn;
          if (MODE == 0) v.re = p[0];
          else if (a.icx) v = *reinterpret_cast<const Cx<T>*>(p);
          else { v.re = p[0]; v.im = p[1]; }
        }
        put(r, k, v);
      }
    }
    __syncthreads();
    // ------------------------------------------------------------------ transform -----
    fft_lds<T, ITER>(lds, slots, m, logm, W, tid);
    if (BLUE) {
      for (int e = tid; e < slots; e += FFT_THREADS) {
        const int idx = pad<T>(e);
        lds[idx] = conj_(cmul(lds[idx], bhat[e & (m - 1)]));   // conj: the inverse is conj(F(conj(.)))
      }
      __syncthreads();
      fft_lds<T, ITER>(lds, slots, m, logm, W, tid);
    }
    // ------------------------------------------------------------------ store ---------
    if (a.ovec) {                                   // R == 1, inner == 1, unit stride, aligned rows
      T* po = out + l0 * a.oso;
      if (MODE == 2) {
        constexpr int V = 16 / (int)sizeof(T);
        for (int k0 = tid * V; k0 < n; k0 += FFT_THREADS * V) {
          if (k0 + V <= n) {
            Vec16<T> p;
#pragma unroll
            for (int e = 0; e < V; ++e) p.v[e] = get(0, k0 + e).re;
            *reinterpret_cast<Vec16<T>*>(po + k0) = p;
          } else {
            for (int k = k0; k < n; ++k) po[k] = get(0, k).re;
          }
        }
      } else if constexpr (sizeof(T) == 4) {        // float32 pairs
        const int h = (int)((reinterpret_cast<uintptr_t>(po) >> 3) & 1);
        if (tid == 0 && h) *reinterpret_cast<Cx<T>*>(po) = get(0, 0);
        for (int k0 = h + 2 * tid; k0 < nout; k0 += 2 * FFT_THREADS) {
          if (k0 + 2 <= nout) {
            const Cx<T> y0 = get(0, k0), y1 = get(0, k0 + 1);
            Vec16<T> p;
            p.v[0] = y0.re; p.v[1] = y0.im; p.v[2] = y1.re; p.v[3] = y1.im;
            *reinterpret_cast<Vec16<T>*>(po + 2 * (int64_t)k0) = p;
          } else {
            *reinterpret_cast<Cx<T>*>(po + 2 * (int64_t)k0) = get(0, k0);
          }
        }
      }
    } else {
      for (int e = tid; e < slots; e += FFT_THREADS) {
        const int r = rowfast ? (e & (R - 1)) : (e >> logm);
        const int k = rowfast ? (e >> logR) : (e & (m - 1));
        const int64_t l = l0 + r;
        if (k >= nout || l >= a.rows) continue;
        const int64_t o = rowfast ? l / a.inner : l, i = rowfast ? l - o * a.inner : 0;
        T* p = out + o * a.oso + i * a.osi + (int64_t)k * a.osn;
        const Cx<T> y = get(r, k);
        if (MODE == 2) p[0] = y.re;
        else if (a.ocx) *reinterpret_cast<Cx<T>*>(p) = y;
        else { p[0] = y.re; p[1] = y.im; }
      }
    }
    __syncthreads();                                // the image is refilled by the next group
  }
}

inline bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }
inline bool fft_supported(int64_t n) {
  return n >= 1 && (is_pow2(n) ? n <= FFT_MAX_POW2 : n <= FFT_MAX_OTHER);
}
// transform size behind an axis of n points
inline int fft_m(int64_t n) {
  if (is_pow2(n)) return (int)n;
  int m = 1;
  while (m < 2 * n - 1) m <<= 1;
  return m;
}
inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

template <typename K>
int allow_lds(K kernel, size_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    ahip_set_error("hipFuncSetAttribute: %s", hipGetErrorString(e));
    return AHIP_EHIP;
  }
  return AHIP_OK;
}

template <typename T, int ITER, int MODE, bool BLUE>
int launch_fft(const FftArgs& a, hipStream_t s) {
  constexpr size_t lds = lds_bytes<T>(FFT_WG_SLOTS * ITER);
  // (every launch: the attribute is per device, and a process may drive several)
  if (int rc = allow_lds(fft_kernel<T, ITER, MODE, BLUE>, lds)) return rc;
  const int R = 1 << a.logR;
  int64_t groups = (a.rows + R - 1) / R;          // any batch: the kernel strides over the groups
  const int64_t cap = (int64_t)ahip_cu_count() * 16;
  if (groups > cap) groups = cap;
  AHIP_LAUNCH((fft_kernel<T, ITER, MODE, BLUE>), dim3((unsigned)groups), dim3(FFT_THREADS), lds, s, a);
  return AHIP_OK;
}

template <typename T, int ITER>
int launch_bhat(const TabArgs& t, hipStream_t s) {
  constexpr size_t lds = lds_bytes<T>(FFT_WG_SLOTS * ITER);
  if (int rc = allow_lds(fft_bhat_kernel<T, ITER>, lds)) return rc;
  AHIP_LAUNCH((fft_bhat_kernel<T, ITER>), dim3(1), dim3(FFT_THREADS), lds, s, t);
  return AHIP_OK;
}

template <typename T, int MODE>
int run_fft(FftArgs a, void* ws, size_t ws_bytes, hipStream_t s) {
  const int n = a.n, m = fft_m(n);
  const bool blue = m != n;
  int logm = 0;
  while ((1 << logm) < m) ++logm;
  a.m = m; a.logm = logm;
  a.logR = 0;
  while ((m << a.logR) < FFT_WG_SLOTS) ++a.logR;
  const int iter = (m << a.logR) / FFT_WG_SLOTS;
  // workspace: twiddles [m], chirp [n], chirp spectrum [m]
  const size_t cb = sizeof(Cx<T>), offc = up256(m * cb), offb = offc + up256(n * cb);
  const size_t need = blue ? offb + up256(m * cb) : offc;
  AHIP_REQUIRE(ws != nullptr && ws_bytes >= need, "fft: workspace of %zu bytes needed", need);
  AHIP_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 16 == 0, "fft: workspace must be 16-byte aligned");
  char* w = static_cast<char*>(ws);
  TabArgs t{w, blue ? w + offc : nullptr, blue ? w + offb : nullptr, n, m, logm, blue ? 1 : 0};
  a.W = t.W; a.chirp = t.chirp; a.bhat = t.bhat;
  AHIP_LAUNCH((fft_tables_kernel<T>), dim3((unsigned)((m + FFT_THREADS - 1) / FFT_THREADS)),
              dim3(FFT_THREADS), 0, s, t);
  if (blue) {
    const int rc = m <= 1024 ? launch_bhat<T, 1>(t, s) : m == 2048 ? launch_bhat<T, 2>(t, s)
                                                                   : launch_bhat<T, 4>(t, s);
    if (rc) return rc;
  }
  // access forms
  const uintptr_t xa = reinterpret_cast<uintptr_t>(a.x), oa = reinterpret_cast<uintptr_t>(a.out);
  const size_t pair = 2 * sizeof(T);
  auto even = [](int64_t v) { return (v & 1) == 0; };
  a.icx = MODE != 0 && xa % pair == 0 && even(a.xso) && even(a.xsn) && even(a.xsi);
  a.ocx = MODE != 2 && oa % pair == 0 && even(a.oso) && even(a.osn) && even(a.osi);
  const bool row_form = a.logR == 0 && a.inner == 1;
  const int64_t V = 16 / (int64_t)sizeof(T);
  if (MODE == 0) a.ivec = row_form && a.xsn == 1 && xa % 16 == 0 && a.xso % V == 0;
  else a.ivec = row_form && sizeof(T) == 4 && a.icx && a.xsn == 2;
  if (MODE == 2) a.ovec = row_form && a.osn == 1 && oa % 16 == 0 && a.oso % V == 0;
  else a.ovec = row_form && sizeof(T) == 4 && a.ocx && a.osn == 2;
  switch (iter * 2 + (blue ? 1 : 0)) {
    case 2: return launch_fft<T, 1, MODE, false>(a, s);
    case 3: return launch_fft<T, 1, MODE, true>(a, s);
    case 4: return launch_fft<T, 2, MODE, false>(a, s);
    case 5: return launch_fft<T, 2, MODE, true>(a, s);
    case 8: return launch_fft<T, 4, MODE, false>(a, s);
    case 9: return launch_fft<T, 4, MODE, true>(a, s);
    default: ahip_set_error("fft: no kernel for %d points", m); return AHIP_EINVAL;
  }
}

template <int MODE>
int fft_entry(int dtype, int inverse, const void* x, int64_t outer, int64_t n, int64_t inner,
              int64_t valid, int64_t x_so, int64_t x_sn, int64_t x_si, void* out, int64_t o_so,
              int64_t o_sn, int64_t o_si, void* ws, size_t ws_bytes, void* stream) {
  AHIP_REQUIRE(n >= 1, "Invalid number of FFT data points (%lld) specified.", (long long)n);
  AHIP_REQUIRE(outer >= 0 && inner >= 0 && valid >= 0, "negative extent");
  if (!fft_supported(n)) {
    ahip_set_error("fft: axis of length %lld: one-workgroup transforms take powers of two up to %d "
                   "and other lengths up to %d", (long long)n, FFT_MAX_POW2, FFT_MAX_OTHER);
    return AHIP_ENOSUP;
  }
  if (outer == 0 || inner == 0) return AHIP_OK;
  AHIP_REQUIRE(x && out, "null argument");
  FftArgs a{};
  a.x = x; a.out = out;
  a.rows = outer * inner; a.inner = inner; a.valid = valid;
  a.xso = x_so; a.xsn = x_sn; a.xsi = x_si; a.oso = o_so; a.osn = o_sn; a.osi = o_si;
  a.n = (int)n; a.inverse = inverse ? 1 : 0;
  hipStream_t s = as_stream(stream);
  switch (dtype) {
    case AHIP_F32: return run_fft<float, MODE>(a, ws, ws_bytes, s);
    case AHIP_F64: return run_fft<double, MODE>(a, ws, ws_bytes, s);
    default: ahip_set_error("fft: dtype %d (float32 / float64 only)", dtype); return AHIP_EINVAL;
  }
}

}  // namespace

extern "C" {

size_t ahip_fft_ws_bytes(int dtype, int64_t n) {
  if ((dtype != AHIP_F32 && dtype != AHIP_F64) || !fft_supported(n)) return 0;
  const size_t cb = 2 * (size_t)ahip_itemsize(dtype);
  const size_t m = (size_t)fft_m(n);
  return m == (size_t)n ? up256(m * cb) : 2 * up256(m * cb) + up256((size_t)n * cb);
}

int ahip_fft_r2c(int dtype, const void* x, int64_t outer, int64_t n, int64_t inner, int64_t valid,
                 int64_t x_so, int64_t x_sn, int64_t x_si, void* out, int64_t o_so, int64_t o_sn,
                 int64_t o_si, void* ws, size_t ws_bytes, void* stream) {
  return fft_entry<0>(dtype, 0, x, outer, n, inner, valid, x_so, x_sn, x_si, out, o_so, o_sn, o_si,
                      ws, ws_bytes, stream);
}

int ahip_fft_c2c(int dtype, int inverse, const void* x, int64_t outer, int64_t n, int64_t inner,
                 int64_t valid, int64_t x_so, int64_t x_sn, int64_t x_si, void* out, int64_t o_so,
                 int64_t o_sn, int64_t o_si, void* ws, size_t ws_bytes, void* stream) {
  return fft_entry<1>(dtype, inverse, x, outer, n, inner, valid, x_so, x_sn, x_si, out, o_so, o_sn,
                      o_si, ws, ws_bytes, stream);
}

int ahip_fft_c2r(int dtype, const void* x, int64_t outer, int64_t n, int64_t inner, int64_t valid,
                 int64_t x_so, int64_t x_sn, int64_t x_si, void* out, int64_t o_so, int64_t o_sn,
                 int64_t o_si, void* ws, size_t ws_bytes, void* stream) {
  return fft_entry<2>(dtype, 1, x, outer, n, inner, valid, x_so, x_sn, x_si, out, o_so, o_sn, o_si,
                      ws, ws_bytes, stream);
}

}  // extern "C"
