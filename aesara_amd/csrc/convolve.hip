// K24: 1-D convolution, np.convolve in its three modes, as a direct LDS-tiled sliding window.
//
// Replaces tensor/math.py:3062 Convolve.perform (np.convolve(a, v, mode)).  With m = len(a) >= n = len(v)
// (the caller swaps):  full[j] = sum_k v[k] a[j - k],  j in [0, m + n - 1).  The caller names the window
// [lo, lo + len) of `full` it wants, which is all that tells the three modes apart.
//
// Split of the work.  A workgroup of 256 threads owns TILE_OUT = 256 R consecutive outputs (R = 8
// accumulators a thread, in registers) and walks the taps in chunks of TAP_CHUNK.  Per chunk [k0, k0 + C)
// it stages in LDS
//     tap[c] = v[k0 + C - 1 - c]            (reversed, zero past n)
//     win[i] = a[j0 - k0 - (C - 1) + i]     (TILE_OUT + C elements, zero outside [0, m))
// so that  out[j0 + o] += sum_c tap[c] win[o + c]:  a correlation whose window slides FORWARD with c.
//
// Thread-to-output mapping: 16-byte groups, interleaved.  With V = 16 / sizeof(element) (4 for the
// 4-byte types, 2 for the 8-byte ones) a thread owns the G = R / V groups q = t + 256 g, group q being the
// V consecutive outputs V q .. V q + V - 1.  For V taps a group needs win[V (q + s) .. V (q + s) + 2 V - 2]:
// the two aligned 16-byte words q + s and q + s + 1.  As s advances the second becomes the first, so each
// step costs ONE new 128-bit LDS read a group plus one 128-bit broadcast read of V taps (every lane the same
// address), for V V multiply-adds a group: R + U - 1 window values for R U products with U = V.
// Why this and not R consecutive outputs a thread: lane t reads the 16-byte word t + 256 g + s, so the 64
// lanes of a wave read 64 consecutive aligned words — no padding, no swizzle and nothing unaligned; R
// consecutive outputs a thread put the lanes 32 bytes apart, which needs a skewed window to spread over the
// banks.  Measured (SQ_LDS_BANK_CONFLICT over SQ_LDS_IDX_ACTIVE, profiles/convolve_probe.jsonl): 0 for the
// 8-byte types, whose words the compiler reads as two 64-bit halves, but 0.53 for the 4-byte types, read
// with one 128-bit instruction: consecutive words are NOT free of conflicts for that instruction on this
// LDS, and float32 is the slower for it (DESIGN 3.3n names the successor).  The staging writes (element
// t + 256 i) and the result stores (16 bytes a lane, consecutive lanes adjacent) are conflict-free and
// coalesced.
// A group whose outputs all lie behind the end of the window is skipped by its whole wave (the test is
// wave-uniform): a `valid` call with few outputs keeps one wave busy instead of four.
//
// Double buffering: the next chunk's global loads (nine window elements and one tap a thread) are issued
// into registers before the current chunk's products and stored to LDS behind them.
//
// Tap trimming: the tile [j0, j1) touches only taps k with 0 <= j - k < m for some j in it, that is
// max(0, j0 - m + 1) <= k < min(n, j1); only the chunks that meet this range are walked, and inside a chunk
// only the steps that hold such a tap (three taps cost one step, not TAP_CHUNK / V).
//
// Tap split: when the tiles are fewer than the compute units, gridDim.y = S > 1 workgroups share a tile,
// each taking a contiguous share of that tile's chunks and writing a partial row of ws[S][len]; a fold
// kernel adds the rows in split order.  No float atomics: the same bits on every call.  S comes from
// (m, n, lo, len) alone (splits() below), never from the device.
//
// Integers accumulate in the unsigned type (8- and 16-bit operands in 32 bits, truncated on the store):
// NumPy's wrap-around, bit for bit, for the signed types too.
//
// Matrix instructions do not fit: there is one output vector, so a Toeplitz operand built from `a` would
// be used for a single column — no second dimension to reuse the fragment over.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int R = 8;
constexpr int TILE_OUT = AHIP_CONVOLVE_TILE_OUT;
constexpr int TAP_CHUNK = AHIP_CONVOLVE_TAP_CHUNK;
constexpr int WIN = TILE_OUT + TAP_CHUNK;      // staged window elements a chunk (the last one is never multiplied)
constexpr int WIN_PER_THREAD = WIN / THREADS;
constexpr int64_t SPLIT_BELOW_TILES = 256;     // fewer tiles than this: split the taps ...
constexpr int64_t SPLIT_TARGET = 2048;         // ... until tiles * S reaches this (eight workgroups a CU)
static_assert(TILE_OUT == THREADS * R && WIN % THREADS == 0 && TAP_CHUNK == THREADS, "staging layout");

struct ConvArgs {
  const void* a;   // m elements, element stride sa (any sign)
  const void* v;   // n elements, element stride sv
  void* dst;       // out[len], or ws[S][len] when gridDim.y > 1
  int64_t m, n, sa, sv, lo, len;
};
AHIP_PTRS_BEGIN(ConvArgs) AHIP_PTR1(a) AHIP_PTR1(v) AHIP_PTR1(dst) AHIP_PTRS_END

struct FoldArgs {
  const void* ws;  // [S][len]
  void* out;       // [len]
  int64_t len;
  int S;
};
AHIP_PTRS_BEGIN(FoldArgs) AHIP_PTR1(ws) AHIP_PTR1(out) AHIP_PTRS_END

__device__ __forceinline__ float mad(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double mad(double a, double b, double c) { return fma(a, b, c); }
__device__ __forceinline__ uint32_t mad(uint32_t a, uint32_t b, uint32_t c) { return a * b + c; }
__device__ __forceinline__ uint64_t mad(uint64_t a, uint64_t b, uint64_t c) { return a * b + c; }

template <typename E>
struct alignas(16) Word {
  E x[16 / sizeof(E)];
};

// T: the element type in memory; E: the type of the LDS copies and the accumulators
template <typename T, typename E>
__global__ __launch_bounds__(THREADS) void convolve_kernel(ConvArgs p) {
  constexpr int V = 16 / sizeof(E), G = R / V;
  __shared__ Word<E> win_w[WIN / V];
  __shared__ Word<E> tap_w[TAP_CHUNK / V];
  E* win = reinterpret_cast<E*>(win_w);
  E* tap = reinterpret_cast<E*>(tap_w);
  const int t = threadIdx.x;
  const T* a = static_cast<const T*>(p.a);
  const T* v = static_cast<const T*>(p.v);

  const int64_t j0 = p.lo + (int64_t)blockIdx.x * TILE_OUT;
  const int64_t end = p.lo + p.len;
  const int64_t j1 = j0 + TILE_OUT < end ? j0 + TILE_OUT : end;
  // the taps this tile touches, then this split's share of their chunks
  const int64_t kmin = j0 - p.m + 1 > 0 ? j0 - p.m + 1 : 0;
  const int64_t kmax = p.n < j1 ? p.n : j1;
  const int64_t c_lo = kmin / TAP_CHUNK, nc = (kmax + TAP_CHUNK - 1) / TAP_CHUNK - c_lo;
  const int64_t c_beg = c_lo + nc * blockIdx.y / gridDim.y;
  const int64_t c_end = c_lo + nc * (blockIdx.y + 1) / gridDim.y;

  // groups of this thread with an output inside [j0, j1): decided by the wave's first lane
  const int64_t tile_len = j1 - j0;
  bool active[G];
#pragma unroll
  for (int g = 0; g < G; ++g) active[g] = (int64_t)V * ((t & ~63) + THREADS * g) < tile_len;

  E acc[G][V];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < V; ++i) acc[g][i] = E(0);

  E pre_w[WIN_PER_THREAD], pre_t;
  auto fetch = [&](int64_t c) {
    const int64_t k0 = c * TAP_CHUNK;
    const int64_t base = j0 - k0 - (TAP_CHUNK - 1);
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i) {
      const int64_t idx = base + t + THREADS * i;
      pre_w[i] = idx >= 0 && idx < p.m ? (E)a[idx * p.sa] : E(0);
    }
    const int64_t k = k0 + TAP_CHUNK - 1 - t;
    pre_t = k < p.n ? (E)v[k * p.sv] : E(0);
  };

  if (c_beg < c_end) fetch(c_beg);
  for (int64_t c = c_beg; c < c_end; ++c) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i) win[t + THREADS * i] = pre_w[i];
    tap[t] = pre_t;
    __syncthreads();
    if (c + 1 < c_end) fetch(c + 1);  // in flight while this chunk computes

    // the steps of this chunk that hold a tap of [kmin, kmax): tap[c] is tap k0 + C - 1 - c, so a short v
    // (or the ragged first and last chunk of a long one) sits at the END of the reversed chunk
    const int64_t k0 = c * TAP_CHUNK;
    const int taps_hi = (int)(kmax - k0 < TAP_CHUNK ? kmax - k0 : TAP_CHUNK);
    const int taps_lo = (int)(kmin > k0 ? kmin - k0 : 0);
    const int s_beg = (TAP_CHUNK - taps_hi) / V, s_end = (TAP_CHUNK - taps_lo + V - 1) / V;

    Word<E> cur[G];
#pragma unroll
    for (int g = 0; g < G; ++g)
      if (active[g]) cur[g] = win_w[t + THREADS * g + s_beg];
#pragma unroll 2
    for (int s = s_beg; s < s_end; ++s) {
      const Word<E> taps = tap_w[s];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (!active[g]) continue;
        const Word<E> nxt = win_w[t + THREADS * g + s + 1];
        E w[2 * V];
#pragma unroll
        for (int i = 0; i < V; ++i) { w[i] = cur[g].x[i]; w[V + i] = nxt.x[i]; }
#pragma unroll
        for (int u = 0; u < V; ++u)
#pragma unroll
          for (int i = 0; i < V; ++i) acc[g][i] = mad(taps.x[u], w[i + u], acc[g][i]);
        cur[g] = nxt;
      }
    }
  }

  T* dst = static_cast<T*>(p.dst) + (int64_t)blockIdx.y * p.len + (j0 - p.lo);
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int64_t o = (int64_t)V * (t + THREADS * g) + i;
      if (o < tile_len) dst[o] = (T)acc[g][i];
    }
}

template <typename T, typename E>
__global__ __launch_bounds__(THREADS) void convolve_fold_kernel(FoldArgs p) {
  const T* ws = static_cast<const T*>(p.ws);
  T* out = static_cast<T*>(p.out);
  const int64_t step = (int64_t)gridDim.x * THREADS;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < p.len; i += step) {
    E sum = (E)ws[i];
    for (int s = 1; s < p.S; ++s) sum += (E)ws[(int64_t)s * p.len + i];
    out[i] = (T)sum;
  }
}

inline int64_t tiles_of(int64_t len) { return (len + TILE_OUT - 1) / TILE_OUT; }

// the number of tap splits: from the shapes alone.  The chunks of the taps the whole window touches bound
// what one tile walks; S never exceeds them.
int64_t splits(int64_t m, int64_t n, int64_t lo, int64_t len) {
  const int64_t tiles = tiles_of(len);
  if (tiles == 0 || tiles >= SPLIT_BELOW_TILES) return 1;
  const int64_t kmin = lo - m + 1 > 0 ? lo - m + 1 : 0, kmax = n < lo + len ? n : lo + len;
  const int64_t chunks = (kmax + TAP_CHUNK - 1) / TAP_CHUNK - kmin / TAP_CHUNK;
  const int64_t want = (SPLIT_TARGET + tiles - 1) / tiles;
  return chunks < want ? chunks : want;
}

bool lowered_dtype(int dtype) { return dtype >= AHIP_I8 && dtype <= AHIP_F64; }

bool window_ok(int64_t m, int64_t n, int64_t lo, int64_t len) {
  return n >= 1 && m >= n && m < ((int64_t)1 << 40) && lo >= 0 && len >= 0 && lo + len <= m + n - 1;
}

template <typename T, typename E>
int run(ConvArgs& a, void* out, void* ws, hipStream_t s) {
  const int64_t S = splits(a.m, a.n, a.lo, a.len);
  a.dst = S > 1 ? ws : out;
  AHIP_LAUNCH((convolve_kernel<T, E>), dim3((unsigned)tiles_of(a.len), (unsigned)S), dim3(THREADS), 0, s, a);
  if (S > 1) {
    FoldArgs f;
    f.ws = ws; f.out = out; f.len = a.len; f.S = (int)S;
    const int64_t blocks = (a.len + THREADS - 1) / THREADS;
    AHIP_LAUNCH((convolve_fold_kernel<T, E>), dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(THREADS), 0, s, f);
  }
  return AHIP_OK;
}

}  // namespace

extern "C" {

size_t ahip_convolve_ws_bytes(int dtype, int64_t m, int64_t n, int64_t lo, int64_t len) {
  if (!lowered_dtype(dtype) || !window_ok(m, n, lo, len)) return 0;
  const int64_t S = splits(m, n, lo, len);
  return S > 1 ? (size_t)S * (size_t)len * (size_t)ahip_itemsize(dtype) : 0;
}

int ahip_convolve(int dtype, const void* a, int64_t m, int64_t sa, const void* v, int64_t n, int64_t sv, int64_t lo,
                  int64_t len, void* out, void* ws, size_t ws_bytes, void* stream) {
  AHIP_REQUIRE(lowered_dtype(dtype), "convolve: dtype %d (float32 / float64 and the 8- to 64-bit integers)", dtype);
  AHIP_REQUIRE(window_ok(m, n, lo, len), "convolve: window [%lld, +%lld) of operands of %lld and %lld elements "
               "(the longer one first, neither empty)", (long long)lo, (long long)len, (long long)m, (long long)n);
  if (len == 0) return AHIP_OK;
  AHIP_REQUIRE(a != nullptr && v != nullptr && out != nullptr, "null pointer");
  const size_t need = ahip_convolve_ws_bytes(dtype, m, n, lo, len);
  AHIP_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need), "convolve: workspace of %zu bytes, %zu needed",
               ws_bytes, need);
  ConvArgs p;
  p.a = a; p.v = v; p.dst = nullptr;
  p.m = m; p.n = n; p.sa = sa; p.sv = sv; p.lo = lo; p.len = len;
  hipStream_t s = as_stream(stream);
  switch (dtype) {
    case AHIP_F32: return run<float, float>(p, out, ws, s);
    case AHIP_F64: return run<double, double>(p, out, ws, s);
    case AHIP_I8: case AHIP_U8: return run<uint8_t, uint32_t>(p, out, ws, s);
    case AHIP_I16: case AHIP_U16: return run<uint16_t, uint32_t>(p, out, ws, s);
    case AHIP_I32: case AHIP_U32: return run<uint32_t, uint32_t>(p, out, ws, s);
    default: return run<uint64_t, uint64_t>(p, out, ws, s);
  }
}

}  // extern "C"
