// K20: sparse operands in CSR / CSC form (float32 / float64 data, int32 indices and indptr).
//
// replaces the perform methods of aesara/sparse/basic.py: StructuredDot (:3448), Dot (:3991),
// StructuredDotGradCSR / CSC (:3712 / :3579), DenseFromSparse (:986),
// SparseFromDense (:1068), SpSum (:1748), MulSD (:2348) — SciPy's csr_matvecs / csr_todense /
// csr_tocsc loops.
//
// Every kernel is written for the CSR view of a value (major = rows): a CSC value is the CSR view
// of its transpose, so the caller swaps strides and extents instead of the kernels growing a
// second form.  A product that has to run along the uncompressed axis goes through the orientation
// flip first: a stable argsort of `indices` (K13) and flip_finish below, after which every sum
// again runs over one row in ascending original position.  No float atomics anywhere: each
// output element is owned by one wave (or one lane) and summed in a fixed order, so a call is
// reproducible bit for bit.
//
// Safety: a row range is used only if 0 <= start <= end <= nnz and an entry only if its index is
// in [0, minor); anything else is recorded in the info word (AHIP_SPARSE_* in the header, one
// atomicMax) and the entry / row is skipped.  Nothing traps.
#include "common.h"

namespace {

inline bool float_dtype(int dt) { return dt == AHIP_F32 || dt == AHIP_F64; }
constexpr int64_t MAX_EXT = (int64_t)1 << 31;   // int32 indices: every extent and nnz stay below

__device__ inline void report(unsigned long long* info, int what) {
  if (info != nullptr)
    atomicMax(info, (unsigned long long)AHIP_LINALG_INFO_TAG |
                        ((unsigned long long)AHIP_SPARSE_MALFORMED << 32) | (unsigned long long)what);
}

// [s, e) of row r, or false (recorded) when it is not a range inside [0, nnz]
__device__ inline bool row_range(const int* indptr, int64_t r, int64_t nnz, int64_t& s, int64_t& e,
                                 unsigned long long* info) {
  s = indptr[r];
  e = indptr[r + 1];
  if (s < 0 || e < s || e > nnz) {
    report(info, AHIP_SPARSE_BAD_INDPTR);
    return false;
  }
  return true;
}

// index of entry k, or -1 (recorded) when it is outside [0, minor)
__device__ inline int checked_index(const int* indices, int64_t k, int64_t minor, unsigned long long* info) {
  const int j = indices[k];
  if (j < 0 || (int64_t)j >= minor) {
    report(info, AHIP_SPARSE_BAD_INDEX);
    return -1;
  }
  return j;
}

// sum over the 64 lanes in a fixed order (xor butterfly: every lane ends with the same bits)
template <typename T>
__device__ inline T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

constexpr int WAVES = 4;          // waves (= rows) per workgroup of the row kernels
constexpr int NARROW_MAX = 4;     // dense columns up to which lanes go across a row's entries

struct SpmmArgs {
  const void* data;
  const int64_t* perm;   // null: data[k]; else data[perm[k]] (a flipped operand)
  const int* indices;
  const int* indptr;
  const void* B;
  void* out;
  void* info;
  int64_t M, minor, ncols, nnz, b_rs, b_cs, o_rs, o_cs;
};
AHIP_PTRS_BEGIN(SpmmArgs) AHIP_PTR1(data) AHIP_PTR1(perm) AHIP_PTR1(indices) AHIP_PTR1(indptr) AHIP_PTR1(B)
  AHIP_PTR1(out) AHIP_PTR1(info) AHIP_PTRS_END

template <typename T, int VEC> struct VecOf;
template <> struct VecOf<float, 4> { typedef float4 type; };
template <> struct VecOf<double, 2> { typedef double2 type; };

// Wide form: one wave per row and tile of 64 * VEC columns, each lane owns VEC adjacent columns.
// The wave loads 64 entries at a time (one per lane) and hands them round with a shuffle, so the
// walk over a row is not one dependent load per entry.  VLOAD: B's inner stride is 1 and its rows
// are 16-byte aligned (checked by the launcher): a full lane reads its VEC columns in one load.
template <typename T, int VEC, bool VLOAD>
__global__ __launch_bounds__(64 * WAVES) void spmm_wide_kernel(SpmmArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  auto* info = static_cast<unsigned long long*>(a.info);
  const T* data = static_cast<const T*>(a.data);
  const T* B = static_cast<const T*>(a.B);
  const int64_t c0 = ((int64_t)blockIdx.y * 64 + lane) * VEC;
  int64_t s, e;
  T acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = T(0);
  if (row_range(a.indptr, r, a.nnz, s, e, info)) {
    for (int64_t k0 = s; k0 < e; k0 += 64) {
      const int64_t k = k0 + lane;
      int jl = -1;
      T dl = T(0);
      if (k < e) {
        jl = checked_index(a.indices, k, a.minor, info);
        if (jl >= 0) dl = data[a.perm != nullptr ? a.perm[k] : k];
      }
      const int cnt = (int)((e - k0) < 64 ? (e - k0) : 64);
      for (int t = 0; t < cnt; ++t) {
        const int j = __shfl(jl, t, 64);
        const T d = __shfl(dl, t, 64);
        if (j < 0) continue;                       // (wave-uniform)
        if (c0 >= a.ncols) continue;
        const T* b = B + (int64_t)j * a.b_rs + c0 * a.b_cs;
        if (VLOAD && c0 + VEC <= a.ncols) {
          typedef typename VecOf<T, VEC>::type V;
          const V bv = *reinterpret_cast<const V*>(b);
          const T* bs = reinterpret_cast<const T*>(&bv);
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[v] += d * bs[v];
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            if (c0 + v < a.ncols) acc[v] += d * b[v * a.b_cs];
        }
      }
    }
  }
  T* out = static_cast<T*>(a.out) + r * a.o_rs;
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (c0 + v < a.ncols) out[(c0 + v) * a.o_cs] = acc[v];
}

// Narrow form (ncols <= NARROW_MAX, and the vector case): lanes across a row's entries, each lane
// adds its entries k = start + lane, + 64, ... in that order, then the fixed butterfly.
template <typename T>
__global__ __launch_bounds__(64 * WAVES) void spmm_narrow_kernel(SpmmArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  auto* info = static_cast<unsigned long long*>(a.info);
  const T* data = static_cast<const T*>(a.data);
  const T* B = static_cast<const T*>(a.B);
  const int nc = (int)a.ncols;
  T acc[NARROW_MAX];
#pragma unroll
  for (int c = 0; c < NARROW_MAX; ++c) acc[c] = T(0);
  int64_t s, e;
  if (row_range(a.indptr, r, a.nnz, s, e, info)) {
    for (int64_t k = s + lane; k < e; k += 64) {
      const int j = checked_index(a.indices, k, a.minor, info);
      if (j < 0) continue;
      const T d = data[a.perm != nullptr ? a.perm[k] : k];
      const T* b = B + (int64_t)j * a.b_rs;
#pragma unroll
      for (int c = 0; c < NARROW_MAX; ++c)
        if (c < nc) acc[c] += d * b[c * a.b_cs];
    }
  }
  T* out = static_cast<T*>(a.out) + r * a.o_rs;
#pragma unroll
  for (int c = 0; c < NARROW_MAX; ++c) {
    if (c < nc) {                                  // (wave-uniform)
      const T v = wave_sum(acc[c]);
      if (lane == 0) out[c * a.o_cs] = v;
    }
  }
}

struct SddmmArgs {
  const int* indices;
  const int* indptr;
  const void* G;
  const void* B;
  void* out;
  void* info;
  int64_t M, minor, ncols, nnz, g_rs, g_cs, b_rs, b_cs;
};
AHIP_PTRS_BEGIN(SddmmArgs) AHIP_PTR1(indices) AHIP_PTR1(indptr) AHIP_PTR1(G) AHIP_PTR1(B) AHIP_PTR1(out)
  AHIP_PTR1(info) AHIP_PTRS_END

constexpr int SDDMM_LANE_MAX = 16;   // dense columns up to which one lane computes an entry alone

// Sampled product, few columns: lanes across a row's entries, each lane sums its entry's ncols
// products in ascending column order.
template <typename T>
__global__ __launch_bounds__(64 * WAVES) void sddmm_lane_kernel(SddmmArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  auto* info = static_cast<unsigned long long*>(a.info);
  const T* g = static_cast<const T*>(a.G) + r * a.g_rs;
  const T* B = static_cast<const T*>(a.B);
  T* out = static_cast<T*>(a.out);
  int64_t s, e;
  if (!row_range(a.indptr, r, a.nnz, s, e, info)) return;
  for (int64_t k = s + lane; k < e; k += 64) {
    const int j = checked_index(a.indices, k, a.minor, info);
    T acc = T(0);
    if (j >= 0) {
      const T* b = B + (int64_t)j * a.b_rs;
      for (int64_t c = 0; c < a.ncols; ++c) acc += g[c * a.g_cs] * b[c * a.b_cs];
    }
    out[k] = acc;
  }
}

// Sampled product, many columns: the wave takes a row's entries one after the other, lanes across
// the columns (c = lane, + 64, ...), then the fixed butterfly.
template <typename T>
__global__ __launch_bounds__(64 * WAVES) void sddmm_wave_kernel(SddmmArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  auto* info = static_cast<unsigned long long*>(a.info);
  const T* g = static_cast<const T*>(a.G) + r * a.g_rs;
  const T* B = static_cast<const T*>(a.B);
  T* out = static_cast<T*>(a.out);
  int64_t s, e;
  if (!row_range(a.indptr, r, a.nnz, s, e, info)) return;
  for (int64_t k = s; k < e; ++k) {
    const int j = checked_index(a.indices, k, a.minor, info);   // (wave-uniform)
    T acc = T(0);
    if (j >= 0) {
      const T* b = B + (int64_t)j * a.b_rs;
      for (int64_t c = lane; c < a.ncols; c += 64) acc += g[c * a.g_cs] * b[c * a.b_cs];
    }
    acc = wave_sum(acc);
    if (lane == 0) out[k] = acc;
  }
}

struct DenseArgs {      // to_dense, mul_dense, dense_count, dense_fill
  const void* data;
  const int* indices;
  const int* indptr;
  void* D;              // the dense matrix, (row, col) element strides d_rs / d_cs
  void* out;
  int* out_indices;
  void* info;
  int64_t M, minor, nnz, d_rs, d_cs;
};
AHIP_PTRS_BEGIN(DenseArgs) AHIP_PTR1(data) AHIP_PTR1(indices) AHIP_PTR1(indptr) AHIP_PTR1(D) AHIP_PTR1(out)
  AHIP_PTR1(out_indices) AHIP_PTR1(info) AHIP_PTRS_END

// D (zero-filled by the caller) += the stored entries: one lane per row adds its entries in stored
// order, so duplicates add up in that order and rows need not be sorted.
template <typename T>
__global__ __launch_bounds__(256) void to_dense_kernel(DenseArgs a) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= a.M) return;
  auto* info = static_cast<unsigned long long*>(a.info);
  const T* data = static_cast<const T*>(a.data);
  T* d = static_cast<T*>(a.D) + r * a.d_rs;
  int64_t s, e;
  if (!row_range(a.indptr, r, a.nnz, s, e, info)) return;
  for (int64_t k = s; k < e; ++k) {
    const int j = checked_index(a.indices, k, a.minor, info);
    if (j >= 0) d[(int64_t)j * a.d_cs] += data[k];
  }
}

// out[k] = data[k] * D[row(k), indices[k]]
template <typename T>
__global__ __launch_bounds__(64 * WAVES) void mul_dense_kernel(DenseArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  auto* info = static_cast<unsigned long long*>(a.info);
  const T* data = static_cast<const T*>(a.data);
  const T* d = static_cast<const T*>(a.D) + r * a.d_rs;
  T* out = static_cast<T*>(a.out);
  int64_t s, e;
  if (!row_range(a.indptr, r, a.nnz, s, e, info)) return;
  for (int64_t k = s + lane; k < e; k += 64) {
    const int j = checked_index(a.indices, k, a.minor, info);
    out[k] = j >= 0 ? data[k] * d[(int64_t)j * a.d_cs] : T(0);
  }
}

// number of entries of row r of D with value != 0 (-0.0 is dropped, NaN is kept) -> counts[r]
template <typename T>
__global__ __launch_bounds__(64 * WAVES) void dense_count_kernel(DenseArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  const T* d = static_cast<const T*>(a.D) + r * a.d_rs;
  int n = 0;
  for (int64_t c = lane; c < a.minor; c += 64) n += d[c * a.d_cs] != T(0) ? 1 : 0;
  n = wave_sum(n);
  if (lane == 0) a.out_indices[r] = n;
}

// the kept entries of row r in ascending column order, from position indptr[r] on (indptr: the
// exclusive running sum of the counts above, one more entry than rows)
template <typename T>
__global__ __launch_bounds__(64 * WAVES) void dense_fill_kernel(DenseArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (r >= a.M) return;
  const T* d = static_cast<const T*>(a.D) + r * a.d_rs;
  T* out = static_cast<T*>(a.out);
  int64_t s, e;
  if (!row_range(a.indptr, r, a.nnz, s, e, nullptr)) return;
  int64_t pos = s;
  for (int64_t c0 = 0; c0 < a.minor; c0 += 64) {
    const int64_t c = c0 + lane;
    const T v = c < a.minor ? d[c * a.d_cs] : T(0);
    const bool keep = c < a.minor && v != T(0);
    const unsigned long long mask = __ballot(keep);
    const int64_t p = pos + __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && p < e) {
      out[p] = v;
      a.out_indices[p] = (int)c;
    }
    pos += __popcll(mask);
  }
}

struct FlipArgs {
  const int* keys;        // `indices` in ascending order (stable)
  const int64_t* perm;    // keys[p] = indices[perm[p]]
  const int* indptr;
  int* new_indices;
  int* new_indptr;
  void* info;
  int64_t M, minor, nnz;
};
AHIP_PTRS_BEGIN(FlipArgs) AHIP_PTR1(keys) AHIP_PTR1(perm) AHIP_PTR1(indptr) AHIP_PTR1(new_indices)
  AHIP_PTR1(new_indptr) AHIP_PTR1(info) AHIP_PTRS_END

// The other orientation of a pattern from the stable argsort of its indices: entry p of the
// flipped value is entry perm[p] of the original; its index is the ROW that entry sits in (binary
// search in indptr) and row j of the flipped value starts at the first key >= j.  Entries with a
// key outside [0, minor) end up outside every flipped row; the flipped arrays are in range by
// construction whatever the operand holds, and what is wrong with it is recorded.
__global__ __launch_bounds__(256) void flip_finish_kernel(FlipArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  auto* info = static_cast<unsigned long long*>(a.info);
  if (t < a.nnz) {
    int64_t k = a.perm[t];
    if (k < 0 || k >= a.nnz) k = 0;
    int64_t lo = 0, hi = a.M;                  // first row whose start is beyond k, in [0, M]
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.indptr[mid] <= k) lo = mid + 1; else hi = mid;
    }
    int64_t row = lo - 1;
    if (row < 0) row = 0;
    if (row > a.M - 1) row = a.M - 1;
    if (a.M <= 0) {
      row = 0;
      report(info, AHIP_SPARSE_BAD_INDPTR);
    } else if (!((int64_t)a.indptr[row] <= k && k < (int64_t)a.indptr[row + 1])) {
      report(info, AHIP_SPARSE_BAD_INDPTR);
    }
    a.new_indices[t] = (int)row;
    const int key = a.keys[t];
    if (key < 0 || (int64_t)key >= a.minor) report(info, AHIP_SPARSE_BAD_INDEX);
  }
  if (t <= a.minor) {
    int64_t lo = 0, hi = a.nnz;                // first position whose key is >= t
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.keys[mid] < t) lo = mid + 1; else hi = mid;
    }
    a.new_indptr[t] = (int)lo;
  }
  if (t < a.M) {
    const int64_t s = a.indptr[t], e = a.indptr[t + 1];
    if (s < 0 || e < s || e > a.nnz) report(info, AHIP_SPARSE_BAD_INDPTR);
    // (the flip takes every stored entry: the rows have to cover [0, nnz) exactly)
    if ((t == 0 && s != 0) || (t == a.M - 1 && e != a.nnz)) report(info, AHIP_SPARSE_BAD_INDPTR);
  }
}

inline bool extents_ok(int64_t M, int64_t minor, int64_t nnz) {
  return M >= 0 && M < MAX_EXT && minor >= 0 && minor < MAX_EXT && nnz >= 0 && nnz < MAX_EXT;
}

inline unsigned row_blocks(int64_t M) { return (unsigned)((M + WAVES - 1) / WAVES); }

}  // namespace

extern "C" {

int ahip_csr_narrow_max(void) { return NARROW_MAX; }

int ahip_csr_spmm(int dtype, int64_t M, int64_t minor, int64_t ncols, int64_t nnz, const void* data,
                  const int64_t* perm, const int* indices, const int* indptr, const void* B, int64_t b_rs,
                  int64_t b_cs, void* out, int64_t o_rs, int64_t o_cs, void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "csr_spmm: float32 / float64 only");
  AHIP_REQUIRE(extents_ok(M, minor, nnz) && ncols >= 0 && ncols < MAX_EXT, "csr_spmm: extent out of range");
  if (M == 0 || ncols == 0) return AHIP_OK;
  hipStream_t s = as_stream(stream);
  SpmmArgs a{data, perm, indices, indptr, B, out, info, M, minor, ncols, nnz, b_rs, b_cs, o_rs, o_cs};
  if (ncols <= NARROW_MAX) {
    if (dtype == AHIP_F32) AHIP_LAUNCH(spmm_narrow_kernel<float>, dim3(row_blocks(M)), dim3(64 * WAVES), 0, s, a);
    else AHIP_LAUNCH(spmm_narrow_kernel<double>, dim3(row_blocks(M)), dim3(64 * WAVES), 0, s, a);
    return AHIP_OK;
  }
  const int vec = dtype == AHIP_F32 ? 4 : 2;
  const int64_t tiles = (ncols + 64 * vec - 1) / (64 * vec);
  AHIP_REQUIRE(tiles <= 65535, "csr_spmm: more than 65535 column tiles");
  const bool vload = b_cs == 1 && b_rs % vec == 0 && reinterpret_cast<uintptr_t>(B) % 16 == 0;
  const dim3 grid(row_blocks(M), (unsigned)tiles), block(64 * WAVES);
  if (dtype == AHIP_F32) {
    if (vload) AHIP_LAUNCH((spmm_wide_kernel<float, 4, true>), grid, block, 0, s, a);
    else AHIP_LAUNCH((spmm_wide_kernel<float, 4, false>), grid, block, 0, s, a);
  } else {
    if (vload) AHIP_LAUNCH((spmm_wide_kernel<double, 2, true>), grid, block, 0, s, a);
    else AHIP_LAUNCH((spmm_wide_kernel<double, 2, false>), grid, block, 0, s, a);
  }
  return AHIP_OK;
}

int ahip_csr_sddmm(int dtype, int64_t M, int64_t minor, int64_t ncols, int64_t nnz, const int* indices,
                   const int* indptr, const void* G, int64_t g_rs, int64_t g_cs, const void* B, int64_t b_rs,
                   int64_t b_cs, void* out, void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "csr_sddmm: float32 / float64 only");
  AHIP_REQUIRE(extents_ok(M, minor, nnz) && ncols >= 0 && ncols < MAX_EXT, "csr_sddmm: extent out of range");
  if (M == 0 || nnz == 0) return AHIP_OK;
  hipStream_t s = as_stream(stream);
  SddmmArgs a{indices, indptr, G, B, out, info, M, minor, ncols, nnz, g_rs, g_cs, b_rs, b_cs};
  const dim3 grid(row_blocks(M)), block(64 * WAVES);
  if (ncols <= SDDMM_LANE_MAX) {
    if (dtype == AHIP_F32) AHIP_LAUNCH(sddmm_lane_kernel<float>, grid, block, 0, s, a);
    else AHIP_LAUNCH(sddmm_lane_kernel<double>, grid, block, 0, s, a);
  } else {
    if (dtype == AHIP_F32) AHIP_LAUNCH(sddmm_wave_kernel<float>, grid, block, 0, s, a);
    else AHIP_LAUNCH(sddmm_wave_kernel<double>, grid, block, 0, s, a);
  }
  return AHIP_OK;
}

int ahip_csr_to_dense(int dtype, int64_t M, int64_t minor, int64_t nnz, const void* data, const int* indices,
                      const int* indptr, void* D, int64_t d_rs, int64_t d_cs, void* info, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "csr_to_dense: float32 / float64 only");
  AHIP_REQUIRE(extents_ok(M, minor, nnz), "csr_to_dense: extent out of range");
  if (M == 0 || minor == 0) return AHIP_OK;
  DenseArgs a{data, indices, indptr, D, nullptr, nullptr, info, M, minor, nnz, d_rs, d_cs};
  const dim3 grid((unsigned)((M + 255) / 256)), block(256);
  if (dtype == AHIP_F32) AHIP_LAUNCH(to_dense_kernel<float>, grid, block, 0, as_stream(stream), a);
  else AHIP_LAUNCH(to_dense_kernel<double>, grid, block, 0, as_stream(stream), a);
  return AHIP_OK;
}

int ahip_csr_mul_dense(int dtype, int64_t M, int64_t minor, int64_t nnz, const void* data, const int* indices,
                       const int* indptr, const void* D, int64_t d_rs, int64_t d_cs, void* out, void* info,
                       void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "csr_mul_dense: float32 / float64 only");
  AHIP_REQUIRE(extents_ok(M, minor, nnz), "csr_mul_dense: extent out of range");
  if (M == 0 || nnz == 0) return AHIP_OK;
  DenseArgs a{data, indices, indptr, const_cast<void*>(D), out, nullptr, info, M, minor, nnz, d_rs, d_cs};
  const dim3 grid(row_blocks(M)), block(64 * WAVES);
  if (dtype == AHIP_F32) AHIP_LAUNCH(mul_dense_kernel<float>, grid, block, 0, as_stream(stream), a);
  else AHIP_LAUNCH(mul_dense_kernel<double>, grid, block, 0, as_stream(stream), a);
  return AHIP_OK;
}

int ahip_dense_count_rows(int dtype, int64_t M, int64_t minor, const void* D, int64_t d_rs, int64_t d_cs,
                          int* counts, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "dense_count_rows: float32 / float64 only");
  AHIP_REQUIRE(extents_ok(M, minor, 0), "dense_count_rows: extent out of range");
  if (M == 0) return AHIP_OK;
  DenseArgs a{nullptr, nullptr, nullptr, const_cast<void*>(D), nullptr, counts, nullptr, M, minor, 0, d_rs, d_cs};
  const dim3 grid(row_blocks(M)), block(64 * WAVES);
  if (dtype == AHIP_F32) AHIP_LAUNCH(dense_count_kernel<float>, grid, block, 0, as_stream(stream), a);
  else AHIP_LAUNCH(dense_count_kernel<double>, grid, block, 0, as_stream(stream), a);
  return AHIP_OK;
}

int ahip_dense_fill_csr(int dtype, int64_t M, int64_t minor, int64_t nnz, const void* D, int64_t d_rs,
                        int64_t d_cs, const int* indptr, void* data, int* indices, void* stream) {
  AHIP_REQUIRE(float_dtype(dtype), "dense_fill_csr: float32 / float64 only");
  AHIP_REQUIRE(extents_ok(M, minor, nnz), "dense_fill_csr: extent out of range");
  if (M == 0 || nnz == 0) return AHIP_OK;
  DenseArgs a{nullptr, nullptr, indptr, const_cast<void*>(D), data, indices, nullptr, M, minor, nnz, d_rs, d_cs};
  const dim3 grid(row_blocks(M)), block(64 * WAVES);
  if (dtype == AHIP_F32) AHIP_LAUNCH(dense_fill_kernel<float>, grid, block, 0, as_stream(stream), a);
  else AHIP_LAUNCH(dense_fill_kernel<double>, grid, block, 0, as_stream(stream), a);
  return AHIP_OK;
}

int ahip_csr_flip_finish(int64_t M, int64_t minor, int64_t nnz, const int* keys, const int64_t* perm,
                         const int* indptr, int* new_indices, int* new_indptr, void* info, void* stream) {
  AHIP_REQUIRE(extents_ok(M, minor, nnz), "csr_flip_finish: extent out of range");
  int64_t n = nnz > minor + 1 ? nnz : minor + 1;
  if (M > n) n = M;
  FlipArgs a{keys, perm, indptr, new_indices, new_indptr, info, M, minor, nnz};
  AHIP_LAUNCH(flip_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), a);
  return AHIP_OK;
}

}  // extern "C"
