// K25: Images2Neibs, the sliding-window patch extractor, through LDS-staged bands.
//
// Replaces tensor/nnet/neighbours.py:194 Images2Neibs.perform.  x is (N, C, H, W); the result is the
// matrix out[z_row][i c + j] with z_row = b + grid_c (a + grid_r (s + C n)) and
//     out[z_row][i c + j] = x[n, s, a step_r + i + off_r, b step_c + j + off_c],
// zero outside the image (`half`, `full`) or with both indices wrapped once (`wrap_centered`).  The caller
// hands over the grid and the offset of patch (0, 0), which is all that tells the five modes apart
// (exec_neibs.neibs_geometry).  Nothing is computed, so the kernels are templated on the item size only.
//
// The result is r c / (step_r step_c) times the image: the kernel is bound by its stores.  A thread-per-output
// gather would read every image line up to r times through addresses that jump by the image width.
//
// Split of the work.  A workgroup of 256 threads owns a band: one (n, s) image and `band` consecutive patch
// rows a0 .. a1 over all patch columns; when the r image rows of ONE patch row do not fit, band = 1 and the
// workgroup owns `tile` consecutive patch columns of it.  Either way its outputs are one contiguous range of
// the result, `len` elements from element `start`.
//
// Staging.  The workgroup copies the image rows its band touches into LDS, row pitch `pitch` elements, with
// 16-byte global loads where the column stride is 1 and pointer and strides are 16-byte aligned (LDS column 0
// is then the image column rounded down to a 16-byte boundary, `sh` elements left of the band's first one);
// a 16-byte word that hangs over an edge of the image, and every word of an operand that is not aligned,
// is filled element by element.  The mode acts here and nowhere else: rows and columns outside the image are
// zero, or wrapped once.  With step_r > r the rows between two patch rows are not staged: LDS row l holds
// patch row l / r, line l % r.
//
// Stores.  Consecutive lanes own consecutive 16-byte words of the band's range; a lane decodes the first
// element of its word into (a, b, i, j) with three 32-bit divisions, gathers the 16 / itemsize elements from
// LDS at ((a - a0) lr + i, sh + (b - b0) step_c + j) while it steps (j, i, b, a) like an odometer, and issues
// one 16-byte store.  The elements in front of the first aligned word and behind the last are stored one a
// lane, once per band.  No atomics, every output is written exactly once: the same bits on every call.
//
// The caller chooses band, tile and pitch (exec_neibs.band_split, from the shapes alone); this file checks
// them against AHIP_NEIBS_LDS_BYTES.  32 KiB a workgroup rather than the 160 KiB a workgroup can have: five
// workgroups share a compute unit's LDS, so the loads of one hide behind the stores of the others.
//
// A patch whose r rows of c columns do not fit in LDS at all (band = 0) takes the direct kernel: one thread an
// output element.  Its rows are c >= 1000 elements long, so consecutive lanes read consecutive addresses anyway.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int64_t LDS_BYTES = AHIP_NEIBS_LDS_BYTES;

struct NeibsArgs {
  const void* x;
  void* out;
  int64_t sn, sc, sr, sw;        // element strides of x
  int64_t images, C, H, W;       // image index img = (n, s) = (img / C, img % C); image extents
  int64_t grid_r, grid_c;        // patches down and across
  int64_t off_r, off_c;          // image coordinates of element (0, 0) of patch (0, 0)
  int64_t step_r, step_c;
  int64_t r, c;                  // patch extents
  int64_t total;                 // output elements (direct kernel)
  int64_t bands_per_img, tiles_per_row;
  uint32_t band, tile, pitch;
  uint32_t lr;                   // LDS rows between two patch rows: min(step_r, r)
  int wrap, vec;
};
AHIP_PTRS_BEGIN(NeibsArgs) AHIP_PTR1(x) AHIP_PTR1(out) AHIP_PTRS_END

template <typename T>
struct alignas(16) Word {
  T x[16 / sizeof(T)];
};

__device__ __forceinline__ int64_t wrap_once(int64_t i, int64_t n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

template <typename T>
__global__ __launch_bounds__(THREADS) void neibs_kernel(NeibsArgs p) {
  extern __shared__ __align__(16) unsigned char neibs_lds[];
  constexpr uint32_t V = 16 / sizeof(T);
  T* lds = reinterpret_cast<T*>(neibs_lds);
  const uint32_t t = threadIdx.x;

  int64_t bid = blockIdx.x;
  const int64_t tile_id = bid % p.tiles_per_row;
  bid /= p.tiles_per_row;
  const int64_t band_id = bid % p.bands_per_img, img = bid / p.bands_per_img;
  const int64_t a0 = band_id * p.band, b0 = tile_id * p.tile;
  const uint32_t na = (uint32_t)(p.grid_r - a0 < p.band ? p.grid_r - a0 : p.band);
  const uint32_t nb = (uint32_t)(p.grid_c - b0 < p.tile ? p.grid_c - b0 : p.tile);
  const uint32_t r = (uint32_t)p.r, c = (uint32_t)p.c;
  const uint32_t stc = nb > 1 ? (uint32_t)p.step_c : 0;      // (a band with one patch column never multiplies it)
  const int64_t n = img / p.C, s = img - n * p.C;
  const T* src = static_cast<const T*>(p.x) + n * p.sn + s * p.sc;

  // ---- staging: nrows x nvec 16-byte words, the mode applied here ----
  const int64_t col0 = b0 * p.step_c + p.off_c;              // image column of the band's first element
  const uint32_t sh = p.vec ? (uint32_t)(((col0 % V) + V) % V) : 0;
  const int64_t cbase = col0 - sh;                           // image column of LDS column 0
  const uint32_t nvec = (sh + (nb - 1) * stc + c + V - 1) / V;
  const uint32_t nrows = (na - 1) * p.lr + r;
  const int64_t row0 = a0 * p.step_r + p.off_r;
  const bool skip = p.step_r > p.r;
  for (uint32_t u = t; u < nrows * nvec; u += THREADS) {
    const uint32_t l = u / nvec, xv = u - l * nvec;
    int64_t ir = row0 + l;
    if (skip) {
      const uint32_t al = l / r;
      ir = row0 + (int64_t)al * p.step_r + (l - al * r);
    }
    if (p.wrap) ir = wrap_once(ir, p.H);
    const bool row_ok = ir >= 0 && ir < p.H;
    const int64_t ic = cbase + (int64_t)xv * V;
    Word<T> w;
    if (p.vec && row_ok && ic >= 0 && ic + V <= p.W) {
      w = *reinterpret_cast<const Word<T>*>(src + ir * p.sr + ic);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < V; ++k) {
        int64_t jc = ic + k;
        if (p.wrap) jc = wrap_once(jc, p.W);
        w.x[k] = row_ok && jc >= 0 && jc < p.W ? src[ir * p.sr + jc * p.sw] : T(0);
      }
    }
    *reinterpret_cast<Word<T>*>(lds + (size_t)l * p.pitch + xv * V) = w;
  }
  __syncthreads();

  // ---- stores: the band's range [start, start + len) of the result, mode-free ----
  const uint32_t rc = r * c, per_a = nb * rc, len = na * per_a;
  const int64_t start = ((img * p.grid_r + a0) * p.grid_c + b0) * rc;
  T* out = static_cast<T*>(p.out) + start;
  auto at = [&](uint32_t e) {
    const uint32_t al = e / per_a, e1 = e - al * per_a, bl = e1 / rc, e2 = e1 - bl * rc, i = e2 / c, j = e2 - i * c;
    return lds[(al * p.lr + i) * p.pitch + sh + bl * stc + j];
  };
  const uint32_t to_word = (uint32_t)(((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15) / sizeof(T));
  const uint32_t head = to_word < len ? to_word : len;
  const uint32_t nw = (len - head) / V, tail0 = head + nw * V;
  if (t < head) out[t] = at(t);
  if (t < len - tail0) out[tail0 + t] = at(tail0 + t);
  for (uint32_t q = t; q < nw; q += THREADS) {
    const uint32_t e = head + q * V;
    uint32_t al = e / per_a, e1 = e - al * per_a, bl = e1 / rc, e2 = e1 - bl * rc, i = e2 / c, j = e2 - i * c;
    Word<T> w;
#pragma unroll
    for (uint32_t k = 0; k < V; ++k) {
      w.x[k] = lds[(al * p.lr + i) * p.pitch + sh + bl * stc + j];
      const bool cj = ++j == c;
      j = cj ? 0 : j;
      i += cj;
      const bool ci = i == r;
      i = ci ? 0 : i;
      bl += ci;
      const bool cb = bl == nb;
      bl = cb ? 0 : bl;
      al += cb;
    }
    *reinterpret_cast<Word<T>*>(out + e) = w;
  }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void neibs_direct_kernel(NeibsArgs p) {
  const T* x = static_cast<const T*>(p.x);
  T* out = static_cast<T*>(p.out);
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < p.total; e += stride) {
    int64_t q = e / p.c;
    const int64_t j = e - q * p.c;
    const int64_t i = q % p.r;
    q /= p.r;
    const int64_t b = q % p.grid_c;
    q /= p.grid_c;
    const int64_t a = q % p.grid_r, img = q / p.grid_r;
    int64_t ir = a * p.step_r + i + p.off_r, ic = b * p.step_c + j + p.off_c;
    if (p.wrap) {
      ir = wrap_once(ir, p.H);
      ic = wrap_once(ic, p.W);
    }
    const int64_t n = img / p.C, s = img - n * p.C;
    const bool ok = ir >= 0 && ir < p.H && ic >= 0 && ic < p.W;
    out[e] = ok ? x[n * p.sn + s * p.sc + ir * p.sr + ic * p.sw] : T(0);
  }
}

template <typename T>
int run(NeibsArgs& p, hipStream_t s) {
  if (p.band == 0) {
    const int64_t blocks = (p.total + THREADS - 1) / THREADS;
    AHIP_LAUNCH((neibs_direct_kernel<T>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(THREADS), 0, s, p);
    return AHIP_OK;
  }
  const int64_t blocks = p.images * p.bands_per_img * p.tiles_per_row;
  const size_t lds = (size_t)(((int64_t)(p.band - 1) * p.lr + p.r) * p.pitch) * sizeof(T);
  AHIP_LAUNCH((neibs_kernel<T>), dim3((unsigned)blocks), dim3(THREADS), lds, s, p);
  return AHIP_OK;
}

}  // namespace

extern "C" {

int ahip_images2neibs(int dtype, const void* x, const int64_t* shape, const int64_t* strides, const int64_t* geo,
                      void* out, void* stream) {
  const int isz = ahip_itemsize(dtype);
  AHIP_REQUIRE(isz > 0, "images2neibs: dtype %d", dtype);
  AHIP_REQUIRE(shape != nullptr && strides != nullptr && geo != nullptr, "null pointer");
  const int64_t V = 16 / isz, lim = (int64_t)1 << 40;
  NeibsArgs p;
  memset(&p, 0, sizeof(p));
  const int64_t N = shape[0];
  p.C = shape[1]; p.H = shape[2]; p.W = shape[3];
  p.sn = strides[0]; p.sc = strides[1]; p.sr = strides[2]; p.sw = strides[3];
  p.r = geo[0]; p.c = geo[1]; p.step_r = geo[2]; p.step_c = geo[3]; p.grid_r = geo[4]; p.grid_c = geo[5];
  p.off_r = geo[6]; p.off_c = geo[7]; p.wrap = geo[8] != 0;
  const int64_t band = geo[9], tile = geo[10], pitch = geo[11];
  AHIP_REQUIRE(N >= 0 && p.C >= 0 && p.H >= 0 && p.W >= 0 && N < lim && p.C < lim && p.H < lim && p.W < lim,
               "images2neibs: image of shape (%lld, %lld, %lld, %lld)", (long long)N, (long long)p.C, (long long)p.H,
               (long long)p.W);
  AHIP_REQUIRE(p.r >= 1 && p.c >= 1 && p.step_r >= 1 && p.step_c >= 1 && p.r < lim && p.c < lim && p.step_r < lim &&
               p.step_c < lim, "images2neibs: patch (%lld, %lld) at step (%lld, %lld)", (long long)p.r, (long long)p.c,
               (long long)p.step_r, (long long)p.step_c);
  AHIP_REQUIRE(p.grid_r >= 0 && p.grid_c >= 0 && p.grid_r < lim && p.grid_c < lim && -p.off_r < lim && -p.off_c < lim &&
               p.off_r <= 0 && p.off_c <= 0, "images2neibs: grid (%lld, %lld) from (%lld, %lld)", (long long)p.grid_r,
               (long long)p.grid_c, (long long)p.off_r, (long long)p.off_c);
  AHIP_REQUIRE(!p.wrap || (p.H >= p.r && p.W >= p.c), "images2neibs: wrapped patches larger than the image");
  const double count = (double)N * (double)p.C * (double)p.grid_r * (double)p.grid_c * (double)p.r * (double)p.c;
  AHIP_REQUIRE(count < 4.0e18, "images2neibs: %g output elements", count);
  p.total = N * p.C * p.grid_r * p.grid_c * p.r * p.c;
  if (p.total == 0) return AHIP_OK;
  AHIP_REQUIRE(x != nullptr && out != nullptr, "null pointer");
  p.x = x; p.out = out;
  p.images = N * p.C;
  if (N == 1 || p.C == 1 || p.sn == p.sc * p.C) {   // the two leading dimensions merge: img = s, n = 0
    p.sc = p.C > 1 ? p.sc : p.sn;
    p.sn = 0;
    p.C = p.images;
  }
  if (band > 0) {
    const int64_t lr = p.step_r < p.r ? p.step_r : p.r;
    AHIP_REQUIRE(band <= p.grid_r && tile >= 1 && tile <= p.grid_c && (band == 1 || tile == p.grid_c),
                 "images2neibs: bands of %lld patch rows, tiles of %lld patch columns for a grid of (%lld, %lld)",
                 (long long)band, (long long)tile, (long long)p.grid_r, (long long)p.grid_c);
    AHIP_REQUIRE(tile == 1 || p.step_c < LDS_BYTES, "images2neibs: column step %lld", (long long)p.step_c);
    const int64_t cols = V - 1 + (tile - 1) * (tile > 1 ? p.step_c : 0) + p.c;
    AHIP_REQUIRE(pitch % V == 0 && pitch >= (cols + V - 1) / V * V && ((band - 1) * lr + p.r) * pitch * isz <= LDS_BYTES,
                 "images2neibs: %lld rows at a pitch of %lld elements for %lld columns in %lld bytes of LDS",
                 (long long)((band - 1) * lr + p.r), (long long)pitch, (long long)cols, (long long)LDS_BYTES);
    p.band = (uint32_t)band; p.tile = (uint32_t)tile; p.pitch = (uint32_t)pitch; p.lr = (uint32_t)lr;
    p.bands_per_img = (p.grid_r + band - 1) / band;
    p.tiles_per_row = (p.grid_c + tile - 1) / tile;
    const double blocks = (double)p.images * (double)p.bands_per_img * (double)p.tiles_per_row;
    AHIP_REQUIRE(blocks < 2147483647.0, "images2neibs: %g bands", blocks);
    p.vec = V > 1 && p.sw == 1 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && p.sr % V == 0 && p.sc % V == 0 &&
            p.sn % V == 0;
  }
  hipStream_t s = as_stream(stream);
  switch (isz) {
    case 1: return run<uint8_t>(p, s);
    case 2: return run<uint16_t>(p, s);
    case 4: return run<uint32_t>(p, s);
    default: return run<uint64_t>(p, s);
  }
}

}  // extern "C"
